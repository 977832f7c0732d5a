// ptv_flow.hip — flow analysis of a velocity field: shear-rate magnitude, viscous dissipation,
// vorticity magnitude and the Astarita flow-type parameter in one stencil pass, with the sums and
// extrema the analysis report prints.
//
// Restates velocity_analysis.compute_strain_rate (velocity_analysis.py:10-63),
// compute_viscous_dissipation (:65-92), compute_vorticity (:94-120) and
// compute_astarita_flow_type (:151-188), and accumulates what compute_permeability (:122-149) and
// analyze_flow.py:335-368 reduce from them.  The reference calls np.gradient on u, v and w twice
// (18 full-size arrays); here every derivative lives in registers.
//
// np.gradient with scalar spacings (edge_order = 1), per axis of length n and spacing h:
//     interior   (f[i+1] - f[i-1]) / (2. * h)
//     faces      (f[1] - f[0]) / h,  (f[n-1] - f[n-2]) / h
// With the neighbour index clamped to [0, n-1] both face rules are (f[i+1'] - f[i-1']) / h, so
// every load is unconditional and only the divisor depends on the face.  The difference is in the
// field dtype T.  For float32 fields numpy has two division rules (DIVMODE): a Python-float
// spacing is weak, the divisor becomes (float)(2. * h) and the division is float32; a np.float64
// spacing is strong, the difference is widened, divided in float64 and the quotient rounded to
// float32 when np.gradient stores it.  Everything after the derivatives is in T, in numpy's order
// (x**2 is x*x, sums left to right); the build passes -ffp-contract=off.
//
// Layout and z-slabs as ptv_div.hip: T fields (nz, ny, nx) C order, planes [z_begin, z_end) of the
// buffer are computed, plane 0 / nz-1 is a domain face (edge_lo / edge_hi) or a halo plane.
//
// Kernel shape: a block of 256 lanes is 64 x 4 (x, y); a lane owns VEC consecutive x (16 bytes) of
// one y row and marches kFlowPlanes z planes, carrying planes z-1, z, z+1 of all three fields in
// registers, so the z stencil reads each plane once per column.  The y neighbours are the cache
// lines of the adjacent waves, the x neighbours the lane's own vector and two scalars.
// Algorithmic bytes per voxel: 3 sizeof(T) + 1 + sizeof(T) (outputs written).
//
// Statistics: each lane accumulates in float64 (extrema in T), a block reduces in a fixed order
// (wave64 DPP tree, then the four waves in order) and writes one partial per row; k_flow_final
// reduces each row's partials in a fixed order with one block per row.  No floating-point atomics.
// Outputs at solid voxels are +0, so the sum over the fluid voxels and the sum over all voxels of
// an output are the same additions with the zeros left out: one accumulator serves both.
#include <cmath>
#include <type_traits>

#include "../../include/ptv_api.h"
#include "ptv_grad.hpp"
#include "ptv_kernels.hpp"
#include "ptv_wave.hpp"

namespace ptv {

namespace {

constexpr int kFlowPlanes = 32;  // z planes per thread column
#ifndef PTV_FLOW_BATCH
#define PTV_FLOW_BATCH 2  // dev A/B builds set it through PTV_EXTRA_FLAGS
#endif
constexpr int kFlowBatch = PTV_FLOW_BATCH;  // planes whose loads are all issued before any arithmetic
constexpr int kFlowThreads = 256;
constexpr int kFlowItems = 4;    // element groups per thread of the elementwise kernel

template <typename T, int VEC>
struct Vec {
    T e[VEC];
};
template <typename T, int VEC>
__device__ __forceinline__ Vec<T, VEC> ldv(const T *p) {
    Vec<T, VEC> r;
    if constexpr (VEC * sizeof(T) == 16) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        __builtin_memcpy(r.e, &q, 16);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) r.e[i] = p[i];
    }
    return r;
}
template <typename T, int VEC>
__device__ __forceinline__ void stv(T *p, const Vec<T, VEC> &v) {
    if constexpr (VEC * sizeof(T) == 16) {
        uint4 q;
        __builtin_memcpy(&q, v.e, 16);
        *reinterpret_cast<uint4 *>(p) = q;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) p[i] = v.e[i];
    }
}
template <int VEC>
__device__ __forceinline__ Vec<uint8_t, VEC> ldm(const uint8_t *p) {
    Vec<uint8_t, VEC> r;
    if constexpr (VEC == 4) {
        const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
        __builtin_memcpy(r.e, &q, 4);
    } else if constexpr (VEC == 2) {
        const uint16_t q = *reinterpret_cast<const uint16_t *>(p);
        __builtin_memcpy(r.e, &q, 2);
    } else {
        r.e[0] = p[0];
    }
    return r;
}

// np.max / np.min: a NaN on either side wins
struct NanMax {
    template <typename T>
    __device__ T operator()(T a, T b) const { return b != b ? b : ((a > b || a != a) ? a : b); }
};
struct NanMin {
    template <typename T>
    __device__ T operator()(T a, T b) const { return b != b ? b : ((a < b || a != a) ? a : b); }
};

// what a lane accumulates: rows of the partials (kFlowRows)
template <typename T>
struct Acc {
    double su = 0.0, sv = 0.0, sw = 0.0;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    T mx[4], mn[4];
    unsigned fluid = 0;
    __device__ Acc() {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mx[k] = -(T)INFINITY;
            mn[k] = (T)INFINITY;
        }
    }
    __device__ __forceinline__ void put(int k, T v) {
        sum[k] += (double)v;
        mx[k] = NanMax{}(mx[k], v);
        mn[k] = NanMin{}(mn[k], v);
    }
};

// one value per wave into LDS; after the barrier thread `row` combines the four waves in order
template <typename Op>
__device__ __forceinline__ void wave_to_lds(double (*sh)[kFlowThreads / 64], int row, double v, Op op) {
    v = group_reduce<0x3f>(v, op);
    if ((threadIdx.x & 63) == 0) sh[row][threadIdx.x >> 6] = v;
}

// rows the call does not ask for are skipped (want: bit k = output k; uvw: the field sums)
template <typename T>
__device__ __forceinline__ void block_partials(const Acc<T> &acc, unsigned want, bool uvw, double *__restrict__ part,
                                               unsigned npart, unsigned block) {
    __shared__ double sh[kFlowRows][kFlowThreads / 64];
    if (uvw) {
        wave_to_lds(sh, 0, acc.su, OpAdd{});
        wave_to_lds(sh, 1, acc.sv, OpAdd{});
        wave_to_lds(sh, 2, acc.sw, OpAdd{});
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(want >> k & 1)) continue;
        wave_to_lds(sh, 3 + 3 * k, acc.sum[k], OpAdd{});
        wave_to_lds(sh, 4 + 3 * k, (double)acc.mx[k], NanMax{});
        wave_to_lds(sh, 5 + 3 * k, (double)acc.mn[k], NanMin{});
    }
    wave_to_lds(sh, 15, (double)acc.fluid, OpAdd{});
    __syncthreads();
    const int r = (int)threadIdx.x;
    if (r >= kFlowRows) return;
    const bool live = r < 3 ? uvw : (r == 15 || (want >> ((r - 3) / 3) & 1));
    if (!live) return;
    const int kind = r < 3 || r == 15 ? 0 : (r - 3) % 3;
    double s = sh[r][0];
#pragma unroll
    for (int k = 1; k < kFlowThreads / 64; ++k)
        s = kind == 0 ? s + sh[r][k] : (kind == 1 ? NanMax{}(s, sh[r][k]) : NanMin{}(s, sh[r][k]));
    part[(size_t)r * npart + block] = s;
}

// dissipation and flow type of one voxel from its (unmasked) S and O
template <typename T>
__device__ __forceinline__ T dissipation_of(T S, T visc) {
    return visc * (S * S);
}
template <typename T>
__device__ __forceinline__ T flow_type_of(T S, T O) {
    const T den = S + O;
    return den > (T)1e-15 ? (S - O) / den : (T)0;  // a NaN den compares false
}

template <typename T, bool STRONG, int VEC>
__global__ __launch_bounds__(kFlowThreads) void k_flow(FlowArgs a, const T *__restrict__ U, const T *__restrict__ V,
                                                       const T *__restrict__ W, const uint8_t *__restrict__ M,
                                                       T *__restrict__ oS, T *__restrict__ oD, T *__restrict__ oO,
                                                       T *__restrict__ oF, double *__restrict__ part) {
    using D = Div<T, STRONG>;
    int t = blockIdx.x;
    if (a.xcd) {
        // XCD-aware tile order (ptv_div.hip): hardware block b runs on XCD b % 8, so logical tile
        // (b % 8) * per + b / 8 hands each XCD a contiguous run of tiles
        const int per = (a.ntiles + 7) >> 3;
        t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    }
    const bool tile_ok = t < a.ntiles;
    if (!tile_ok) t = 0;
    const int tx = t % a.ntx, ty = (t / a.ntx) % a.nty, tz = t / (a.ntx * a.nty);
    const int x0 = (tx * 64 + (int)(threadIdx.x & 63)) * VEC;
    const int y = ty * 4 + (int)(threadIdx.x >> 6);
    // a lane outside the grid loads and stores nothing, but stays for the block reduction
    const bool active = tile_ok && x0 < a.nx && y < a.ny;
    const unsigned want = (oS ? 1u : 0u) | (oD ? 2u : 0u) | (oO ? 4u : 0u) | (oF ? 8u : 0u);
    const bool needS = (want & 0xbu) != 0, needO = (want & 0xcu) != 0;
    Acc<T> acc;
    if (active) {
        const int zb = a.z_begin + tz * kFlowPlanes;
        const int ze = min(zb + kFlowPlanes, a.z_end);
        const int64_t plane = (int64_t)a.nx * a.ny;
        const int64_t col = (int64_t)y * a.nx + x0;
        const int xl = x0 + VEC - 1;  // the lane's last x
        const bool ylo = y == 0, yhi = y == a.ny - 1;
        // neighbour offsets clamped at the domain faces: every load below is in bounds
        const int oxm = x0 == 0 ? 0 : 1, oxp = xl == a.nx - 1 ? 0 : 1;
        const int64_t oym = ylo ? 0 : a.nx, oyp = yhi ? 0 : a.nx;
        auto row = [&](int zz) { return (int64_t)min(max(zz, 0), a.nz - 1) * plane + col; };
        const D hy = (D)((ylo || yhi) ? a.dy : 2.0 * a.dy);
        const D hxf = (D)a.dx, hxi = (D)(2.0 * a.dx);
        const T visc = (T)a.viscosity;
        const T *F[3] = {U, V, W};

        // c[f][t] = field f at plane z0 - 1 + t; the last two carry into the next batch
        Vec<T, VEC> c[3][kFlowBatch + 2];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            c[f][0] = ldv<T, VEC>(F[f] + row(zb - 1));
            c[f][1] = ldv<T, VEC>(F[f] + row(zb));
        }
        for (int z0 = zb; z0 < ze; z0 += kFlowBatch) {
#pragma unroll
            for (int f = 0; f < 3; ++f)
#pragma unroll
                for (int q = 2; q < kFlowBatch + 2; ++q) c[f][q] = ldv<T, VEC>(F[f] + row(z0 - 1 + q));
            Vec<T, VEC> ym[3][kFlowBatch], yp[3][kFlowBatch];
            T xm[3][kFlowBatch], xp[3][kFlowBatch];
            Vec<uint8_t, VEC> mk[kFlowBatch];
#pragma unroll
            for (int j = 0; j < kFlowBatch; ++j) {
                const int64_t r = row(z0 + j);
#pragma unroll
                for (int f = 0; f < 3; ++f) {
                    ym[f][j] = ldv<T, VEC>(F[f] + r - oym);
                    yp[f][j] = ldv<T, VEC>(F[f] + r + oyp);
                    xm[f][j] = F[f][r - oxm];
                    xp[f][j] = F[f][r + VEC - 1 + oxp];
                }
                if (M) mk[j] = ldm<VEC>(M + r);
            }
#pragma unroll
            for (int j = 0; j < kFlowBatch; ++j) {
                const int z = z0 + j;
                if (z >= ze) break;
                const bool zface = (z == 0 && a.edge_lo) || (z == a.nz - 1 && a.edge_hi);
                const D hz = (D)(zface ? a.dz : 2.0 * a.dz);
                Vec<T, VEC> vS, vD, vO, vF;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const bool xface = x0 + e == 0 || x0 + e == a.nx - 1;
                    const D hx = xface ? hxf : hxi;
                    T g[3][3];  // g[f][axis]: d field f / d (x, y, z)
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        const T n = e + 1 < VEC ? c[f][j + 1].e[e + 1 < VEC ? e + 1 : e] : xp[f][j];
                        const T p = e > 0 ? c[f][j + 1].e[e > 0 ? e - 1 : 0] : xm[f][j];
                        g[f][0] = quot<T, STRONG>(n - p, hx);
                        g[f][1] = quot<T, STRONG>(yp[f][j].e[e] - ym[f][j].e[e], hy);
                        g[f][2] = quot<T, STRONG>(c[f][j + 2].e[e] - c[f][j].e[e], hz);
                    }
                    const T ux = g[0][0], uy = g[0][1], uz = g[0][2];
                    const T vx = g[1][0], vy = g[1][1], vz = g[1][2];
                    const T wx = g[2][0], wy = g[2][1], wz = g[2][2];
                    T S = (T)0, O = (T)0;
                    if (needS) {
                        const T exx = (T)2 * ux, eyy = (T)2 * vy, ezz = (T)2 * wz;
                        const T exy = uy + vx, exz = uz + wx, eyz = vz + wy;
                        S = sqrt(((((T)0.5 * ((exx * exx + eyy * eyy) + ezz * ezz) + exy * exy) + exz * exz) +
                                  eyz * eyz));
                    }
                    if (needO) {
                        const T ox = wy - vz, oy = uz - wx, oz = vx - uy;
                        O = sqrt((ox * ox + oy * oy) + oz * oz);
                    }
                    const bool fluid = M ? mk[j].e[e] != 0 : true;
                    acc.fluid += fluid ? 1u : 0u;
                    acc.su += (double)c[0][j + 1].e[e];
                    acc.sv += (double)c[1][j + 1].e[e];
                    acc.sw += (double)c[2][j + 1].e[e];
                    if (oS) acc.put(0, vS.e[e] = fluid ? S : (T)0);
                    if (oD) acc.put(1, vD.e[e] = fluid ? dissipation_of(S, visc) : (T)0);
                    if (oO) acc.put(2, vO.e[e] = fluid ? O : (T)0);
                    if (oF) acc.put(3, vF.e[e] = fluid ? flow_type_of(S, O) : (T)0);
                }
                const int64_t dst = (int64_t)(z - a.z_begin) * plane + col;
                if (oS) stv<T, VEC>(oS + dst, vS);
                if (oD) stv<T, VEC>(oD + dst, vD);
                if (oO) stv<T, VEC>(oO + dst, vO);
                if (oF) stv<T, VEC>(oF + dst, vF);
            }
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                c[f][0] = c[f][kFlowBatch];
                c[f][1] = c[f][kFlowBatch + 1];
            }
        }
    }
    block_partials(acc, want, true, part, (unsigned)a.npart, blockIdx.x);
}

// elementwise mode: dissipation and / or flow type from S (and O) planes
template <typename T, int VEC>
__global__ __launch_bounds__(kFlowThreads) void k_flow_derived(FlowArgs a, int64_t n, const T *__restrict__ S,
                                                               const T *__restrict__ O, const uint8_t *__restrict__ M,
                                                               T *__restrict__ oD, T *__restrict__ oF,
                                                               double *__restrict__ part) {
    const unsigned want = (oD ? 2u : 0u) | (oF ? 8u : 0u);
    const T visc = (T)a.viscosity;
    Acc<T> acc;
#pragma unroll
    for (int it = 0; it < kFlowItems; ++it) {
        const int64_t i = (((int64_t)blockIdx.x * kFlowItems + it) * kFlowThreads + threadIdx.x) * VEC;
        if (i >= n) break;
        const Vec<T, VEC> s = ldv<T, VEC>(S + i);
        Vec<T, VEC> o, vD, vF;
        if (O) o = ldv<T, VEC>(O + i);
        Vec<uint8_t, VEC> mk;
        if (M) mk = ldm<VEC>(M + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const bool fluid = M ? mk.e[e] != 0 : true;
            acc.fluid += fluid ? 1u : 0u;
            acc.su += (double)s.e[e];  // rows 0 and 1: the sums of the inputs
            if (O) acc.sv += (double)o.e[e];
            if (oD) acc.put(1, vD.e[e] = fluid ? dissipation_of(s.e[e], visc) : (T)0);
            if (oF) acc.put(3, vF.e[e] = fluid ? flow_type_of(s.e[e], o.e[e]) : (T)0);
        }
        if (oD) stv<T, VEC>(oD + i, vD);
        if (oF) stv<T, VEC>(oF + i, vF);
    }
    block_partials(acc, want, true, part, (unsigned)a.npart, blockIdx.x);
}

// block r reduces row r of the partials in a fixed order (thread t takes t, t + 256, ...; then the
// wave tree and the four waves in order) into res[r]; a row nobody wrote gives 0
__global__ __launch_bounds__(kFlowThreads) void k_flow_final(const double *__restrict__ part, unsigned npart,
                                                             unsigned want, int uvw, double *__restrict__ res) {
    __shared__ double sh[kFlowThreads / 64];
    const int r = (int)blockIdx.x;
    const bool live = r < 3 ? uvw != 0 : (r == 15 || (want >> ((r - 3) / 3) & 1));
    if (!live) {
        if (threadIdx.x == 0) res[r] = 0.0;
        return;
    }
    const int kind = r < 3 || r == 15 ? 0 : (r - 3) % 3;
    const double *p = part + (size_t)r * npart;
    double v = kind == 0 ? 0.0 : (kind == 1 ? -(double)INFINITY : (double)INFINITY);
    for (unsigned k = threadIdx.x; k < npart; k += kFlowThreads)
        v = kind == 0 ? v + p[k] : (kind == 1 ? NanMax{}(v, p[k]) : NanMin{}(v, p[k]));
    if (kind == 0) v = group_reduce<0x3f>(v, OpAdd{});
    else if (kind == 1) v = group_reduce<0x3f>(v, NanMax{});
    else v = group_reduce<0x3f>(v, NanMin{});
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = sh[0];
    for (int k = 1; k < kFlowThreads / 64; ++k)
        s = kind == 0 ? s + sh[k] : (kind == 1 ? NanMax{}(s, sh[k]) : NanMin{}(s, sh[k]));
    res[r] = s;
}

inline bool al(const void *p, size_t n) { return ((uintptr_t)p % n) == 0; }

int64_t stencil_tiles(const FlowArgs &a, int vec, int &ntx, int &nty) {
    ntx = (a.nx + 64 * vec - 1) / (64 * vec);
    nty = (a.ny + 3) / 4;
    return (int64_t)ntx * nty * ((a.z_end - a.z_begin + kFlowPlanes - 1) / kFlowPlanes);
}

unsigned want_of(void *const out[4]) {
    return (out[0] ? 1u : 0u) | (out[1] ? 2u : 0u) | (out[2] ? 4u : 0u) | (out[3] ? 8u : 0u);
}

template <typename T, bool STRONG, int VEC>
int launch_v(const FlowArgs &a, const void *U, const void *V, const void *W, const uint8_t *M, void *const out[4],
             double *part, double *res, hipStream_t s) {
    FlowArgs b = a;
    const int64_t nt = stencil_tiles(a, VEC, b.ntx, b.nty);
    b.ntiles = (int)nt;
    const unsigned nblocks = (unsigned)(((nt + 7) >> 3) << 3);
    b.npart = (int)nblocks;
    hipLaunchKernelGGL((k_flow<T, STRONG, VEC>), dim3(nblocks), dim3(kFlowThreads), 0, s, b, (const T *)U,
                       (const T *)V, (const T *)W, M, (T *)out[0], (T *)out[1], (T *)out[2], (T *)out[3], part);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_flow_final, dim3(kFlowRows), dim3(kFlowThreads), 0, s, part, nblocks, want_of(out), 1, res);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

// 16-byte lanes when every row starts 16-byte aligned, else one element per lane
template <typename T, bool STRONG>
int launch_t(const FlowArgs &a, const void *U, const void *V, const void *W, const uint8_t *M, void *const out[4],
             double *part, double *res, hipStream_t s) {
    constexpr int VEC = 16 / sizeof(T);
    bool vec_ok = a.nx % VEC == 0 && al(U, 16) && al(V, 16) && al(W, 16) && (!M || al(M, VEC));
    for (int k = 0; k < 4; ++k) vec_ok = vec_ok && al(out[k], 16);
    if (vec_ok) return launch_v<T, STRONG, VEC>(a, U, V, W, M, out, part, res, s);
    return launch_v<T, STRONG, 1>(a, U, V, W, M, out, part, res, s);
}

template <typename T, int VEC>
int launch_derived_v(const FlowArgs &a, int64_t n, const void *S, const void *O, const uint8_t *M, void *oD, void *oF,
                     double *part, double *res, hipStream_t s) {
    FlowArgs b = a;
    const int64_t per = (int64_t)kFlowThreads * kFlowItems * VEC;
    const unsigned nblocks = (unsigned)((n + per - 1) / per);
    b.npart = (int)nblocks;
    hipLaunchKernelGGL((k_flow_derived<T, VEC>), dim3(nblocks), dim3(kFlowThreads), 0, s, b, n, (const T *)S,
                       (const T *)O, M, (T *)oD, (T *)oF, part);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_flow_final, dim3(kFlowRows), dim3(kFlowThreads), 0, s, part, nblocks,
                       (oD ? 2u : 0u) | (oF ? 8u : 0u), 1, res);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

template <typename T>
int launch_derived_t(const FlowArgs &a, int64_t n, const void *S, const void *O, const uint8_t *M, void *oD, void *oF,
                     double *part, double *res, hipStream_t s) {
    constexpr int VEC = 16 / sizeof(T);
    const bool vec_ok = n % VEC == 0 && al(S, 16) && al(O, 16) && al(oD, 16) && al(oF, 16) && (!M || al(M, VEC));
    if (vec_ok) return launch_derived_v<T, VEC>(a, n, S, O, M, oD, oF, part, res, s);
    return launch_derived_v<T, 1>(a, n, S, O, M, oD, oF, part, res, s);
}

}  // namespace

size_t flow_partials(const FlowArgs &a) {
    int ntx, nty;
    const int64_t nt = stencil_tiles(a, 1, ntx, nty);  // the scalar path has the most tiles
    return (size_t)kFlowRows * (size_t)(((nt + 7) >> 3) << 3);
}

size_t flow_derived_partials(int64_t n) {
    const int64_t per = (int64_t)kFlowThreads * kFlowItems;
    return (size_t)kFlowRows * (size_t)((n + per - 1) / per);
}

int launch_flow(const FlowArgs &a, const void *U, const void *V, const void *W, const uint8_t *M, void *const out[4],
                double *part, double *res, hipStream_t s) {
    int ntx, nty;
    if (stencil_tiles(a, 1, ntx, nty) > 0x7fffff00LL) {
        set_error("flow analysis: grid too large for one launch");
        return PTV_E_ARG;
    }
    if (!a.field_f32) return launch_t<double, false>(a, U, V, W, M, out, part, res, s);
    if (a.strong) return launch_t<float, true>(a, U, V, W, M, out, part, res, s);
    return launch_t<float, false>(a, U, V, W, M, out, part, res, s);
}

int launch_flow_derived(const FlowArgs &a, int64_t n, const void *S, const void *O, const uint8_t *M, void *oD,
                        void *oF, double *part, double *res, hipStream_t s) {
    if ((n + kFlowThreads * kFlowItems - 1) / (kFlowThreads * kFlowItems) > 0x7fffff00LL) {
        set_error("flow derived: too many voxels for one launch");
        return PTV_E_ARG;
    }
    if (!a.field_f32) return launch_derived_t<double>(a, n, S, O, M, oD, oF, part, res, s);
    return launch_derived_t<float>(a, n, S, O, M, oD, oF, part, res, s);
}

}  // namespace ptv
