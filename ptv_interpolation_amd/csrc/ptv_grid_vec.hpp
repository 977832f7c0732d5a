// ptv_grid_vec.hpp — what the dense-grid solvers share (ptv_clean.hip, ptv_variational.hip,
// ptv_pressure.hip; the scalar recurrence and the host loop above it are in ptv_grid_solve.hpp):
// the one- or two-wide element groups of a lane, a group's position on the grid, the fixed-order
// block sum and the layout of the per-block partial sums.
//
// A vector of a solver is a dense float64 (nz, ny, nx) grid, x fastest, with the uint8 fluid mask
// applied in the kernels.  A pass gives each thread kItems groups of VEC consecutive x (VEC = 2
// needs an even nx and 16-byte aligned buffers); block b of a pass writes its partial sum to
// part[b] (row r of a multi-sum pass to part[r * npart + b]), and a one-block kernel sums the
// partials in a fixed order: no floating-point atomics anywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ptv_common.hpp"
#include "ptv_wave.hpp"

namespace ptv {

constexpr int kGridThreads = 256;
constexpr int kGridItems = 4;        // element groups per thread (independent loads in flight)
constexpr int kGridFinalThreads = 256;  // threads of the one-block second reduction stage

struct GridDims {
    int nx, ny, nz;
    unsigned n;      // voxels (< 2^31)
    unsigned plane;  // nx * ny
};

template <int VEC>
struct DV {
    double e[VEC];
};
template <int VEC>
__device__ __forceinline__ DV<VEC> ldd(const double *p) {
    DV<VEC> r;
    if constexpr (VEC == 2) {
        const double2 q = *reinterpret_cast<const double2 *>(p);
        r.e[0] = q.x;
        r.e[1] = q.y;
    } else {
        r.e[0] = p[0];
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void std_(double *p, const DV<VEC> &v) {
    if constexpr (VEC == 2) *reinterpret_cast<double2 *>(p) = make_double2(v.e[0], v.e[1]);
    else p[0] = v.e[0];
}
template <int VEC>
struct MV {
    uint8_t e[VEC];
};
template <int VEC>
__device__ __forceinline__ MV<VEC> ldmk(const uint8_t *p) {
    MV<VEC> r;
    if constexpr (VEC == 2) {
        const uint16_t q = *reinterpret_cast<const uint16_t *>(p);
        r.e[0] = (uint8_t)(q & 0xff);
        r.e[1] = (uint8_t)(q >> 8);
    } else {
        r.e[0] = p[0];
    }
    return r;
}

// position of a thread's element group; a group of VEC lies inside one x row (nx % VEC == 0)
struct Pos {
    unsigned i;
    int x, y, z;
};
template <int VEC>
__device__ __forceinline__ bool group_pos(const GridDims &a, int item, Pos &p) {
    const unsigned long long i =
        ((unsigned long long)blockIdx.x * kGridItems + item) * (kGridThreads * VEC) + threadIdx.x * VEC;
    if (i >= a.n) return false;
    p.i = (unsigned)i;
    p.z = (int)(p.i / a.plane);
    const unsigned r = p.i - (unsigned)p.z * a.plane;
    p.y = (int)(r / (unsigned)a.nx);
    p.x = (int)(r - (unsigned)p.y * (unsigned)a.nx);
    return true;
}

// block sum in a fixed order: wave64 DPP tree, then the 4 wave sums in wave order
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double lds[kGridThreads / 64];
    __syncthreads();  // a previous call's reads of lds
    v = group_reduce<0x3f>(v, OpAdd{});
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int k = 1; k < kGridThreads / 64; ++k) s += lds[k];
    return s;
}

// second stage: the sum of npart partials in a fixed order (thread t takes t, t + 256, ...; then
// the block sum); every thread of the one block returns it
__device__ __forceinline__ double partial_sum(const double *__restrict__ part, unsigned npart) {
    double r = 0.0;
    for (unsigned k = threadIdx.x; k < npart; k += kGridFinalThreads) r += part[k];
    return block_sum(r);
}

// partial sums over fluid voxels of div, |div| and 1 (rows 0, 1, 2 of part)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_div_stats(GridDims a, const double *__restrict__ D,
                                                            const uint8_t *__restrict__ M,
                                                            double *__restrict__ part, unsigned npart) {
    double s = 0.0, sa = 0.0, cnt = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i);
        const DV<VEC> d = ldd<VEC>(D + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (!mc.e[e]) continue;
            s += d.e[e];
            sa += fabs(d.e[e]);
            cnt += 1.0;
        }
    }
    s = block_sum(s);
    sa = block_sum(sa);
    cnt = block_sum(cnt);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[npart + blockIdx.x] = sa;
        part[2 * npart + blockIdx.x] = cnt;
    }
}

inline bool aligned(const void *p, size_t n) { return ((uintptr_t)p % n) == 0; }
template <typename... P>
bool all_aligned16(P... p) {
    return (aligned(p, 16) && ...);
}

// blocks of a pass over n voxels with VEC elements per lane
inline unsigned blocks_for(unsigned n, int vec) {
    const unsigned per = (unsigned)(kGridThreads * kGridItems * vec);
    return (n + per - 1) / per;
}

// median of the per-iteration times of the polling batches all of whose iterations ran before the
// solve stopped at iteration itn; batch b lies between events ev[first + b] and ev[first + b + 1]
template <typename Events>
int median_iter_ms(const Events &ev, size_t first, const std::vector<int> &batch_iters, int itn, double ms_solve,
                   double &median) {
    std::vector<double> per;
    int seen = 0;
    for (size_t b = 0; b < batch_iters.size(); ++b) {
        seen += batch_iters[b];
        if (seen > itn) break;
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, ev[first + b], ev[first + b + 1]));
        per.push_back((double)ms / batch_iters[b]);
    }
    if (per.empty()) {
        median = itn > 0 ? ms_solve / itn : 0.0;
    } else {
        std::sort(per.begin(), per.end());
        median = per[per.size() / 2];
    }
    return PTV_OK;
}

}  // namespace ptv
