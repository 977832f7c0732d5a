// ptv_drag.hip — staircase interface drag over a label mask, and the sums of a pressure field's
// np.gradient components.
//
// Restates velocity_analysis.compute_interface_drag(method='staircase') (velocity_analysis.py:
// 332-511) and the device half of compute_permeability_from_pressure (:659-697).  The reference
// loops over labels x 3 axes x 2 directions and builds full-size boolean arrays at every step;
// here one pass reads the mask once and touches the fields only at interface faces.
//
// Faces.  The int32 mask (nz, ny, nx) C order holds 0 = fluid, a positive label = a phase.  A voxel
// owns the faces to its +x, +y and +z neighbours (none across an array edge).  A face (curr, next)
// counts for label L in direction A when curr == 0 and next == L, in direction B when curr == L and
// next == 0; label-label faces, negative values and labels not asked for give nothing.  Axes are
// numbered as the reference's arrays: 0 = z, 1 = y, 2 = x.
//
// Per face, in float64 whatever the field dtype (float32 fields are widened on load), exactly as
// the reference writes the terms; the build passes -ffp-contract=off:
//     p_face = 0.5 * (p[curr] + p[next]);  pressure term  p_face * area (A),  (-p_face) * area (B)
//     d = (-2.0 * vel[fluid cell]) / step
//     viscous term  ((viscosity * 2) * d) * area  for the component along the face normal,
//                   (viscosity * d) * area        for the other two
// with area = dy*dx, dz*dx, dz*dy and step = dz, dy, dx for axes 0, 1, 2.
//
// Rows.  A (label slot, axis, direction) has kDragVals rows: the face count, then the sums of the
// pressure, u, v and w terms.  The sums are the same bits on every call and do not depend on where
// a label stands in the table: no floating-point atomics anywhere.
//   - A block owns a fixed run of voxels; lane t takes voxels t, t + 256, ... of it.
//   - One label (the bool-mask case): the 30 rows live in registers per lane, a block reduces them
//     in a fixed order (wave64 DPP tree, then the four waves in order).
//   - Several labels: the slot of a face's label comes from a binary search of the sorted label
//     table (only lanes that hold a face search).  A wave ballots the lanes that hold a face, walks
//     the set bits in lane order and adds each face's values into that wave's own LDS rows; the
//     block's waves are then added in order.  kDragChunk label slots fit the LDS at a time
//     (32 x 30 x 8 B x 4 waves = 30 KB); more labels are more passes over the mask, each with the
//     next chunk of the table.
//   - One partial per block and row; k_rows_final reduces each row's partials in a fixed order.
//
// Gradient sums: np.gradient's elementwise formula as ptv_flow.hip restates it (clamped neighbour
// indices, the divisor depends on the face, numpy's two float32 division rules), each quotient
// widened to float64 and summed in the same fixed order.
#include <algorithm>
#include <cmath>

#include "../../include/ptv_api.h"
#include "ptv_grad.hpp"
#include "ptv_kernels.hpp"
#include "ptv_wave.hpp"

namespace ptv {

namespace {

constexpr int kDragThreads = 256;
constexpr int kDragWaves = kDragThreads / 64;
constexpr int kDragMinItems = 16;      // voxels per lane of the smallest block
constexpr int kDragMaxBlocks = 2048;   // beyond it the blocks grow instead (fewer partials)

// where a lane's voxel is, advanced by kDragThreads voxels per item without a division
struct Walk {
    int64_t i;       // linear index
    int x, y, z;
    int sx, sy, sz;  // kDragThreads = sz * plane + sy * nx + sx
    __device__ Walk(int64_t i0, int nx, int ny) : i(i0) {
        const int64_t plane = (int64_t)nx * ny;
        z = (int)(i0 / plane);
        const int64_t r = i0 - (int64_t)z * plane;
        y = (int)(r / nx);
        x = (int)(r - (int64_t)y * nx);
        sz = (int)(kDragThreads / plane);
        const int q = (int)(kDragThreads - sz * plane);
        sy = q / nx;
        sx = q - sy * nx;
    }
    __device__ __forceinline__ void next(int nx, int ny) {
        i += kDragThreads;
        x += sx;
        if (x >= nx) {
            x -= nx;
            ++y;
        }
        y += sy;
        if (y >= ny) {
            y -= ny;
            ++z;
        }
        z += sz;
    }
};

// a face between mask values c (the owner) and n: the label it belongs to, or 0
__device__ __forceinline__ int face_label(int c, int n) {
    return (c == 0 && n > 0) ? n : ((c > 0 && n == 0) ? c : 0);
}

// the four sums' terms of one face; ic / in: the owner and its neighbour, dirB: the owner is the solid
template <typename T>
__device__ __forceinline__ void face_terms(const DragArgs &a, int axis, bool dirB, int64_t ic, int64_t in,
                                           const T *__restrict__ U, const T *__restrict__ V,
                                           const T *__restrict__ W, const T *__restrict__ P, double t[4]) {
    const double area = a.area[axis], step = a.step[axis];
    const double visc = a.viscosity, visc2 = a.viscosity * 2;
    const int64_t f = dirB ? in : ic;  // the fluid cell
    t[0] = 0.0;
    if (P) {
        const double pf = 0.5 * ((double)P[ic] + (double)P[in]);
        t[0] = dirB ? (-pf) * area : pf * area;
    }
    const double du = (-2.0 * (double)U[f]) / step;
    const double dv = (-2.0 * (double)V[f]) / step;
    const double dw = (-2.0 * (double)W[f]) / step;
    t[1] = ((axis == 2 ? visc2 : visc) * du) * area;
    t[2] = ((axis == 1 ? visc2 : visc) * dv) * area;
    t[3] = ((axis == 0 ? visc2 : visc) * dw) * area;
}

// slot of `lab` in tab[0, n) (ascending), or -1
__device__ __forceinline__ int find_slot(const int *tab, int n, int lab) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] < lab) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && tab[lo] == lab) ? lo : -1;
}

// One pass over the mask for the labels tab[0, nlab) (nlab <= kDragChunk; SINGLE: nlab == 1).
// part: (gridDim.x, nlab * kDragSlotRows) doubles, block-major.
template <typename T, bool SINGLE>
__global__ __launch_bounds__(kDragThreads) void k_drag(DragArgs a, const int *__restrict__ M,
                                                       const T *__restrict__ U, const T *__restrict__ V,
                                                       const T *__restrict__ W, const T *__restrict__ P,
                                                       const int *__restrict__ tab, int nlab,
                                                       double *__restrict__ part) {
    __shared__ double sh[SINGLE ? kDragSlotRows * kDragWaves : kDragWaves * kDragChunk * kDragSlotRows];
    __shared__ int stab[kDragChunk];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = nlab * kDragSlotRows;
    if (tid < nlab) stab[tid] = tab[tid];
    if constexpr (!SINGLE)
        for (int r = tid; r < kDragWaves * rows; r += kDragThreads) sh[r] = 0.0;
    __syncthreads();
    const int lab_lo = stab[0], lab_hi = stab[nlab - 1];
    volatile double *mine = sh + (SINGLE ? 0 : wave * rows);  // this wave's rows (!SINGLE)

    double acc[3][2][kDragVals];
    if constexpr (SINGLE) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int k = 0; k < kDragVals; ++k) acc[ax][d][k] = 0.0;
    }

    const int64_t plane = (int64_t)a.nx * a.ny;
    const int64_t base = (int64_t)blockIdx.x * a.span;
    const int64_t end = min(base + a.span, a.nvox);
    const int64_t stride[3] = {plane, (int64_t)a.nx, 1};
    if (base + tid < a.nvox) {  // a block past the grid's end only writes its zero partials
        Walk p(base + tid, a.nx, a.ny);
        for (int it = 0; it < a.items; ++it, p.next(a.nx, a.ny)) {
            const bool in = p.i < end;  // uniform per wave but for the last one
            // a neighbour across an array edge reads as -1: no face (and no load)
            const bool has[3] = {in && p.z + 1 < a.nz, in && p.y + 1 < a.ny, in && p.x + 1 < a.nx};
            const int c = in ? M[p.i] : -1;
            int n[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) n[ax] = has[ax] ? M[p.i + stride[ax]] : -1;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const int lab = face_label(c, n[ax]);
                int slot = -1;
                if (lab >= lab_lo && lab <= lab_hi && lab > 0) slot = SINGLE ? 0 : find_slot(stab, nlab, lab);
                const bool hit = slot >= 0;
                const bool dirB = c != 0;
                double t[4] = {0.0, 0.0, 0.0, 0.0};
                if (hit) face_terms<T>(a, ax, dirB, p.i, p.i + stride[ax], U, V, W, P, t);
                if constexpr (SINGLE) {
                    if (hit) {
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
                            const bool here = dirB == (d == 1);
                            acc[ax][d][0] += here ? 1.0 : 0.0;
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[ax][d][1 + k] += here ? t[k] : 0.0;
                        }
                    }
                } else {
                    // the lanes that hold a face, one at a time in lane order: a row is only ever
                    // added to by one lane at a time, in an order the inputs alone decide
                    unsigned long long b = __ballot(hit);
                    while (b) {
                        const int l = __ffsll((long long)b) - 1;
                        b &= b - 1;
                        if (lane == l) {
                            volatile double *q = mine + (slot * 6 + ax * 2 + (dirB ? 1 : 0)) * kDragVals;
                            const double o0 = q[0], o1 = q[1], o2 = q[2], o3 = q[3], o4 = q[4];
                            q[0] = o0 + 1.0;
                            q[1] = o1 + t[0];
                            q[2] = o2 + t[1];
                            q[3] = o3 + t[2];
                            q[4] = o4 + t[3];
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        }
    }

    double *out = part + (size_t)blockIdx.x * rows;
    if constexpr (SINGLE) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int k = 0; k < kDragVals; ++k) {
                    const double v = group_reduce<0x3f>(acc[ax][d][k], OpAdd{});
                    if (lane == 0) sh[((ax * 2 + d) * kDragVals + k) * kDragWaves + wave] = v;
                }
        __syncthreads();
        if (tid < kDragSlotRows) {
            double s = sh[tid * kDragWaves];
#pragma unroll
            for (int k = 1; k < kDragWaves; ++k) s += sh[tid * kDragWaves + k];
            out[tid] = s;
        }
    } else {
        __syncthreads();
        for (int r = tid; r < rows; r += kDragThreads) {
            double s = sh[r];
#pragma unroll
            for (int k = 1; k < kDragWaves; ++k) s += sh[k * rows + r];
            out[r] = s;
        }
    }
}

// The sums of the three np.gradient components of P; part: (gridDim.x, 3) doubles, block-major,
// rows in np.gradient's order (d/dz, d/dy, d/dx).
template <typename T, bool STRONG>
__global__ __launch_bounds__(kDragThreads) void k_gradient_sums(DragArgs a, const T *__restrict__ P,
                                                                double *__restrict__ part) {
    using D = Div<T, STRONG>;
    __shared__ double sh[3][kDragWaves];
    const int tid = (int)threadIdx.x;
    const int64_t plane = (int64_t)a.nx * a.ny;
    const int64_t base = (int64_t)blockIdx.x * a.span;
    const int64_t end = min(base + a.span, a.nvox);
    const D hxf = (D)a.step[2], hxi = (D)(2.0 * a.step[2]);
    const D hyf = (D)a.step[1], hyi = (D)(2.0 * a.step[1]);
    const D hzf = (D)a.step[0], hzi = (D)(2.0 * a.step[0]);
    double s[3] = {0.0, 0.0, 0.0};
    if (base + tid < a.nvox) {
        Walk p(base + tid, a.nx, a.ny);
        for (int it = 0; it < a.items && p.i < end; ++it, p.next(a.nx, a.ny)) {
            // neighbour offsets clamped at the domain faces: every load is in bounds
            const bool xl = p.x == 0, xh = p.x == a.nx - 1;
            const bool yl = p.y == 0, yh = p.y == a.ny - 1;
            const bool zl = p.z == 0, zh = p.z == a.nz - 1;
            const T gx = quot<T, STRONG>(P[p.i + (xh ? 0 : 1)] - P[p.i - (xl ? 0 : 1)], (xl || xh) ? hxf : hxi);
            const T gy = quot<T, STRONG>(P[p.i + (yh ? 0 : a.nx)] - P[p.i - (yl ? 0 : a.nx)], (yl || yh) ? hyf : hyi);
            const T gz = quot<T, STRONG>(P[p.i + (zh ? 0 : plane)] - P[p.i - (zl ? 0 : plane)], (zl || zh) ? hzf : hzi);
            s[0] += (double)gz;
            s[1] += (double)gy;
            s[2] += (double)gx;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double v = group_reduce<0x3f>(s[r], OpAdd{});
        if ((tid & 63) == 0) sh[r][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 3) {
        double v = sh[tid][0];
#pragma unroll
        for (int k = 1; k < kDragWaves; ++k) v += sh[tid][k];
        part[(size_t)blockIdx.x * 3 + tid] = v;
    }
}

// block r adds row r of the block-major partials in a fixed order (thread t takes blocks t, t + 256,
// ...; then the wave tree and the four waves in order) into res[r]
__global__ __launch_bounds__(kDragThreads) void k_rows_final(const double *__restrict__ part, unsigned npart,
                                                             unsigned rows, double *__restrict__ res) {
    __shared__ double sh[kDragWaves];
    const unsigned r = blockIdx.x;
    double v = 0.0;
    for (unsigned k = threadIdx.x; k < npart; k += kDragThreads) v += part[(size_t)k * rows + r];
    v = group_reduce<0x3f>(v, OpAdd{});
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = sh[0];
    for (int k = 1; k < kDragWaves; ++k) s += sh[k];
    res[r] = s;
}

// the run of voxels a block owns: kDragMinItems per lane, more once the grid would pass kDragMaxBlocks
void tile(DragArgs &a, unsigned &nblocks) {
    a.nvox = (int64_t)a.nx * a.ny * a.nz;
    const int64_t per = (int64_t)kDragThreads * kDragMaxBlocks;
    a.items = (int)std::max<int64_t>(kDragMinItems, (a.nvox + per - 1) / per);
    a.span = (int64_t)a.items * kDragThreads;
    nblocks = (unsigned)((a.nvox + a.span - 1) / a.span);
}

template <typename T>
int launch_drag_t(DragArgs a, const int *M, const void *U, const void *V, const void *W, const void *P,
                  const int *labels, int nlabels, double *part, double *res, hipStream_t s) {
    unsigned nblocks;
    tile(a, nblocks);
    for (int c0 = 0; c0 < nlabels; c0 += kDragChunk) {
        const int nc = std::min(kDragChunk, nlabels - c0);
        if (nlabels == 1)
            hipLaunchKernelGGL((k_drag<T, true>), dim3(nblocks), dim3(kDragThreads), 0, s, a, M, (const T *)U,
                               (const T *)V, (const T *)W, (const T *)P, labels, 1, part);
        else
            hipLaunchKernelGGL((k_drag<T, false>), dim3(nblocks), dim3(kDragThreads), 0, s, a, M, (const T *)U,
                               (const T *)V, (const T *)W, (const T *)P, labels + c0, nc, part);
        PTV_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rows_final, dim3(nc * kDragSlotRows), dim3(kDragThreads), 0, s, part, nblocks,
                           (unsigned)(nc * kDragSlotRows), res + (size_t)c0 * kDragSlotRows);
        PTV_HIP(hipGetLastError());
    }
    return PTV_OK;
}

template <typename T, bool STRONG>
int launch_gradient_t(DragArgs a, const void *P, double *part, double *res, hipStream_t s) {
    unsigned nblocks;
    tile(a, nblocks);
    hipLaunchKernelGGL((k_gradient_sums<T, STRONG>), dim3(nblocks), dim3(kDragThreads), 0, s, a, (const T *)P, part);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rows_final, dim3(3), dim3(kDragThreads), 0, s, part, nblocks, 3u, res);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

}  // namespace

size_t drag_partials(const DragArgs &a, int nlabels) {
    DragArgs b = a;
    unsigned nblocks;
    tile(b, nblocks);
    return (size_t)nblocks * (size_t)std::max(3, std::min(nlabels, kDragChunk) * kDragSlotRows);
}

int launch_drag(const DragArgs &a, const int *M, const void *U, const void *V, const void *W, const void *P,
                const int *labels, int nlabels, double *part, double *res, hipStream_t s) {
    if (a.field_f32) return launch_drag_t<float>(a, M, U, V, W, P, labels, nlabels, part, res, s);
    return launch_drag_t<double>(a, M, U, V, W, P, labels, nlabels, part, res, s);
}

int launch_gradient_sums(const DragArgs &a, const void *P, double *part, double *res, hipStream_t s) {
    if (!a.field_f32) return launch_gradient_t<double, false>(a, P, part, res, s);
    if (a.strong) return launch_gradient_t<float, true>(a, P, part, res, s);
    return launch_gradient_t<float, false>(a, P, part, res, s);
}

}  // namespace ptv
