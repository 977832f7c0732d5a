// ptv_edt.hip — exact 3-D Euclidean distance transform of a byte mask, and the alignment score
// that gathers it at shifted particles.
//
// Meaning (scipy.ndimage.distance_transform_edt, unit spacing): for every nonzero voxel of the
// uint8 mask (nz, ny, nx) C order the distance to the nearest zero voxel, 0 at zero voxels.  The
// squared distance d2 is an integer; the float64 field is sqrt((double)d2), correctly rounded (this
// file is built without fast-math), which is what scipy returns bit for bit.
//
// Three separable passes, integers only:
//   x  k_edt_rows   one wave per row: the distance to the nearest zero along x from two wave scans
//                   (nearest zero at or before x, nearest at or after), stored squared.
//   y  k_edt_cols   the lower envelope  out[j] = min_k f[k] + (j - k)^2  along the axis, by direct
//   z               minimisation: lane = column (the contiguous index: x within a plane for y, the
//                   flattened (y, x) for z), so every load and store of a wave is coalesced.  A
//                   block stages its 64 columns in LDS when they fit (n <= kEdtStagedMax), else it
//                   reads the previous pass's buffer.  Per output the scan walks outwards from j,
//                   r = 1, 2, ..., and stops once r^2 >= the best value so far, because every
//                   candidate further out is at least r^2: the cost is O(distance) per voxel, O(n)
//                   only where the nearest zero is that far.
//
// Width and sentinel.  The host refuses nz^2 + ny^2 + nx^2 >= 2^31, so every true squared distance,
// partial (x only; x and y) or final, is < 2^31, and so is r^2 for r < n.  Values are uint32 and "no
// zero in this row / plane yet" is kEdtInf = 2^31, above every true value.  The only sums formed are
// f[k] + r^2 with f <= 2^31 and r^2 < 2^31, which is < 2^32: no uint32 sum can wrap.  A minimum never
// rises above its start f[j] <= kEdtInf, so the sentinel survives a pass unchanged where a whole
// plane has no zero, and a final maximum equal to kEdtInf says the volume has no zero at all.
//
// The maximum of d2 comes from a wave tree and one integer atomicMax per wave.
//
// Alignment score (auto_align.find_best_offset's objective): per offset o and point p, s = p + o in
// float64, rint (half to even, as np.round), the bounds test in floating point, then the gather of
// the float64 field.  Per offset one record {inside, outside, sum}.  Sums have a fixed order: lane t
// of a block adds points t, t + 256, ... of the block's run, then the wave tree, the four waves in
// order, one partial per block, and k_align_final adds the partials the same way.  No floating-point
// atomics; the order depends on the point count alone, so a batch equals the single calls.
#include <algorithm>
#include <cmath>

#include "../../include/ptv_api.h"
#include "ptv_kernels.hpp"
#include "ptv_wave.hpp"

namespace ptv {

namespace {

constexpr unsigned kEdtInf = 0x80000000u;   // squared distance: no zero seen
constexpr unsigned kEdtFar = 0xFFFFFFFFu;   // 1-D distance inside k_edt_rows: no zero seen
constexpr int kEdtThreads = 256;
constexpr int kNone = (int)0x80000000;      // the identity of wave_incl_scan_max

// x pass.  F[row][x] = (distance along x to the nearest zero of the row)^2, kEdtInf without one.
__global__ __launch_bounds__(kEdtThreads) void k_edt_rows(const uint8_t *__restrict__ M, unsigned *F, int nx,
                                                          int64_t nrows) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * (kEdtThreads / 64);
    // a wave owns a row; the trip counts below are uniform over the wave, so the scans see 64 lanes
    for (int64_t row = (int64_t)blockIdx.x * (kEdtThreads / 64) + ((int)threadIdx.x >> 6); row < nrows; row += step) {
        const uint8_t *m = M + row * nx;
        unsigned *f = F + row * nx;
        int carry = kNone;  // the last zero's index in the chunks before
        for (int b = 0; b < nx; b += 64) {
            const int x = b + lane;
            const bool in = x < nx;
            const int key = (in && m[x] == 0) ? x : kNone;
            const int last = max(wave_incl_scan_max(key), carry);
            if (in) f[x] = last == kNone ? kEdtFar : (unsigned)(x - last);
            carry = __builtin_amdgcn_readlane(last, 63);
        }
        carry = kNone;  // minus the next zero's index in the chunks after
        for (int b = ((nx - 1) >> 6) << 6; b >= 0; b -= 64) {
            const int x = b + lane;
            const bool in = x < nx;
            const int key = (in && m[x] == 0) ? -x : kNone;
            // a suffix maximum: the prefix scan over the lanes in reverse
            const int rev = wave_incl_scan_max(__shfl(key, 63 - lane));
            const int next = max(__shfl(rev, 63 - lane), carry);
            if (in) {  // the lane reads back what it stored itself above
                const unsigned dl = f[x];
                const unsigned dr = next == kNone ? kEdtFar : (unsigned)(-next - x);
                const unsigned d = min(dl, dr);
                f[x] = d == kEdtFar ? kEdtInf : d * d;
            }
            carry = __builtin_amdgcn_readlane(next, 0);
        }
    }
}

// y / z pass over columns c in [0, ncols): element k of column c is at
//     (c / inner) * outer + (c % inner) + k * stride.
// FINAL: writes d2 (int32) and / or the float64 distance instead of the uint32 buffer, and the maximum.
template <bool STAGED, bool FINAL>
__global__ __launch_bounds__(1024) void k_edt_cols(EdtCols a, const unsigned *__restrict__ F, unsigned *__restrict__ G,
                                                   int *__restrict__ d2, double *__restrict__ dist,
                                                   unsigned *__restrict__ vmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned tile[];  // STAGED: (n, 64)
    const int lane = (int)threadIdx.x & 63, seg = (int)threadIdx.x >> 6, nseg = (int)blockDim.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    const bool live = c < a.ncols;
    const int64_t base = live ? (c / a.inner) * a.outer + (c % a.inner) : 0;
    const int n = a.n;
    if constexpr (STAGED) {
        for (int k = seg; k < n; k += nseg) tile[k * 64 + lane] = live ? F[base + (int64_t)k * a.stride] : kEdtInf;
        __syncthreads();
    }
    auto at = [&](int k) -> unsigned {
        if constexpr (STAGED) return tile[k * 64 + lane];
        else return F[base + (int64_t)k * a.stride];
    };
    unsigned top = 0;
    if (live) {
        for (int j = seg; j < n; j += nseg) {
            unsigned best = at(j);
            for (int r = 1;; ++r) {
                const unsigned r2 = (unsigned)r * (unsigned)r;
                const int lo = j - r, hi = j + r;
                if (r2 >= best || (lo < 0 && hi >= n)) break;
                if (lo >= 0) best = min(best, at(lo) + r2);
                if (hi < n) best = min(best, at(hi) + r2);
            }
            const int64_t o = base + (int64_t)j * a.stride;
            if constexpr (FINAL) {
                if (d2) d2[o] = (int)best;
                if (dist) dist[o] = sqrt((double)best);
                top = max(top, best);
            } else {
                G[o] = best;
            }
        }
    }
    if constexpr (FINAL) {
        top = group_reduce<0x3f>(top, OpMax{});
        if (lane == 0) atomicMax(vmax, top);
    }
}

constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;

// One block per (run of points, offset): partial sum and inside count of the run.
__global__ __launch_bounds__(kAlignThreads) void k_align_score(AlignArgs a, const double *__restrict__ P,
                                                               const double *__restrict__ DT,
                                                               const double *__restrict__ off,
                                                               double *__restrict__ psum, int *__restrict__ pcnt) {
    __shared__ double shs[kAlignWaves];
    __shared__ int shc[kAlignWaves];
    const int tid = (int)threadIdx.x;
    const unsigned o = blockIdx.y;
    const double ox = off[3 * o], oy = off[3 * o + 1], oz = off[3 * o + 2];
    const double fx = (double)a.nx, fy = (double)a.ny, fz = (double)a.nz;
    const int64_t base = (int64_t)blockIdx.x * a.span;
    const int64_t end = min(base + a.span, a.n);
    double s = 0.0;
    int cnt = 0;
    for (int64_t i = base + tid; i < end; i += kAlignThreads) {
        const double rx = rint(P[3 * i] + ox), ry = rint(P[3 * i + 1] + oy), rz = rint(P[3 * i + 2] + oz);
        // in floating point first: only an index inside the volume is converted (and -0.0 is index 0)
        if (rx >= 0.0 && rx < fx && ry >= 0.0 && ry < fy && rz >= 0.0 && rz < fz) {
            s += DT[((int64_t)(int)rz * a.ny + (int)ry) * a.nx + (int)rx];
            ++cnt;
        }
    }
    s = group_reduce<0x3f>(s, OpAdd{});
    cnt = group_reduce<0x3f>(cnt, OpAdd{});
    if ((tid & 63) == 0) {
        shs[tid >> 6] = s;
        shc[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < kAlignWaves; ++k) {
        s += shs[k];
        cnt += shc[k];
    }
    psum[(size_t)o * gridDim.x + blockIdx.x] = s;
    pcnt[(size_t)o * gridDim.x + blockIdx.x] = cnt;
}

// block o adds offset o's partials in a fixed order (thread t takes partials t, t + 256, ...; the
// wave tree; the four waves in order) into its record
__global__ __launch_bounds__(kAlignThreads) void k_align_final(const double *__restrict__ psum,
                                                               const int *__restrict__ pcnt, unsigned npart,
                                                               int64_t n, ptv_align_record *__restrict__ rec) {
    __shared__ double shs[kAlignWaves];
    __shared__ int shc[kAlignWaves];
    const int tid = (int)threadIdx.x;
    const unsigned o = blockIdx.x;
    double s = 0.0;
    int cnt = 0;  // the host keeps the point count below 2^31
    for (unsigned k = tid; k < npart; k += kAlignThreads) {
        s += psum[(size_t)o * npart + k];
        cnt += pcnt[(size_t)o * npart + k];
    }
    s = group_reduce<0x3f>(s, OpAdd{});
    cnt = group_reduce<0x3f>(cnt, OpAdd{});
    if ((tid & 63) == 0) {
        shs[tid >> 6] = s;
        shc[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < kAlignWaves; ++k) {
        s += shs[k];
        cnt += shc[k];
    }
    rec[o].n_inside = cnt;
    rec[o].n_outside = n - cnt;
    rec[o].sum = s;
}

template <bool STAGED, bool FINAL>
int launch_cols_t(const EdtCols &a, int threads, size_t lds, const unsigned *F, unsigned *G, int *d2, double *dist,
                  unsigned *vmax, hipStream_t s) {
    if (lds > 65536)  // a tile past the default dynamic LDS limit is asked for by name
        PTV_HIP(hipFuncSetAttribute((const void *)k_edt_cols<STAGED, FINAL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    const unsigned blocks = (unsigned)((a.ncols + 63) / 64);
    hipLaunchKernelGGL((k_edt_cols<STAGED, FINAL>), dim3(blocks), dim3(threads), lds, s, a, F, G, d2, dist, vmax);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

// one envelope pass along an axis of length n
int launch_cols(const EdtCols &a, bool final, const unsigned *F, unsigned *G, int *d2, double *dist, unsigned *vmax,
                hipStream_t s) {
    const bool staged = a.n <= kEdtStagedMax;
    // 64 columns x (threads / 64) runs of the axis; a large tile leaves room for few blocks on a
    // compute unit, so each brings more waves
    const int threads = staged && a.n > kEdtStagedMax / 4 ? 1024 : kEdtThreads;
    const size_t lds = staged ? (size_t)a.n * 64 * sizeof(unsigned) : 0;
    if (staged) {
        if (final) return launch_cols_t<true, true>(a, threads, lds, F, G, d2, dist, vmax, s);
        return launch_cols_t<true, false>(a, threads, lds, F, G, d2, dist, vmax, s);
    }
    if (final) return launch_cols_t<false, true>(a, threads, lds, F, G, d2, dist, vmax, s);
    return launch_cols_t<false, false>(a, threads, lds, F, G, d2, dist, vmax, s);
}

}  // namespace

int launch_edt(int nx, int ny, int nz, const uint8_t *M, unsigned *A, unsigned *B, int *d2, double *dist,
               unsigned *vmax, hipStream_t s) {
    const int64_t plane = (int64_t)nx * ny, nrows = (int64_t)ny * nz;
    PTV_HIP(hipMemsetAsync(vmax, 0, sizeof(unsigned), s));
    const unsigned blocks = (unsigned)std::min<int64_t>((nrows + 3) / 4, 1 << 20);
    hipLaunchKernelGGL(k_edt_rows, dim3(blocks), dim3(kEdtThreads), 0, s, M, A, nx, nrows);
    PTV_HIP(hipGetLastError());
    // y: a column is (z, x); z: a column is the flattened (y, x)
    const EdtCols ya{(int64_t)nz * nx, ny, (int64_t)nx, (int64_t)nx, plane};
    const EdtCols za{plane, nz, plane, plane, 0};
    PTV_TRY(launch_cols(ya, false, A, B, nullptr, nullptr, vmax, s));
    PTV_TRY(launch_cols(za, true, B, nullptr, d2, dist, vmax, s));
    return PTV_OK;
}

void align_tile(AlignArgs &a) {
    const int64_t per = (int64_t)kAlignThreads * kAlignMaxBlocks;
    const int64_t items = std::max<int64_t>(kAlignMinItems, (a.n + per - 1) / per);
    a.span = items * kAlignThreads;
    a.nblocks = (unsigned)std::max<int64_t>(1, (a.n + a.span - 1) / a.span);
}

int launch_align_score(const AlignArgs &a, const double *P, const double *DT, const double *off, int m, double *psum,
                       int *pcnt, ptv_align_record *rec, hipStream_t s) {
    hipLaunchKernelGGL(k_align_score, dim3(a.nblocks, (unsigned)m), dim3(kAlignThreads), 0, s, a, P, DT, off, psum, pcnt);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_align_final, dim3((unsigned)m), dim3(kAlignThreads), 0, s, psum, pcnt, a.nblocks, a.n, rec);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

}  // namespace ptv
