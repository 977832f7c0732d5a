// ptv_label.hip — connected-component labelling of a 3-D byte mask, numbered as
// scipy.ndimage.label numbers it.
//
// Union-find on an int32 parent array over the linear voxel index (z slowest, x fastest), -1 at
// background voxels.  ONE INVARIANT holds in every kernel of this file:
//
//     parent[v] <= v, and a write only ever lowers a parent (atomicMin, or a store of a found root).
//
// What follows from it:
//   * find() walks strictly decreasing indices, so it ends under any interleaving, and on any value
//     it may read: a stale one is an earlier parent, which is still <= v.
//   * unite() retries only from the value its atomicMin returned, which is below the node it tried
//     to link; every retry strictly lowers an index.  No loop here waits for another thread.
//   * a link that an atomicMin displaces is re-made by the thread that displaced it (it goes on with
//     the old parent), so when a kernel ends every union asked for holds.
//   * the final root of a component is its smallest linear index, i.e. its first voxel in raster
//     order; partition and roots are unique, so the output is the same bytes on every call
//     although atomics are used.  scipy numbers components in the raster order of their first
//     voxels (tests/test_label_oracle.py holds that), hence label = rank of the root + 1.
//
// Passes: (1) k_label_tiles: one block per 8 x 8 x 64 tile, the forest in LDS; (2) k_label_borders:
// the low faces of every tile unite with the adjacent tiles, global atomics; (3) k_label_flatten:
// parent[v] = find(v) and the root flags; (4) an exclusive scan of the flags (hipCUB) and
// k_label_number: labels = rank[parent] + 1, the sizes by integer atomics.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <string>

#include "ptv_common.hpp"
#include "ptv_label.hpp"

namespace ptv {

namespace {

constexpr int kLabelThreads = 256;
constexpr int kLabelWaves = kLabelThreads / 64;
constexpr int kTileRows = kLabelTileY * kLabelTileZ;
constexpr int kTileVoxels = kTileRows * kLabelTileX;
constexpr unsigned kMaxGrid = 1u << 20;  // every kernel strides over its work from at most this many blocks

static_assert(kLabelTileX == 64, "a tile row is one wave: the run starts and the neighbour masks are ballots");

typedef unsigned long long u64;

// the four rows in front of a voxel's own in raster order, (dz, dy): (0, -1), (-1, -1), (-1, 0), (-1, 1)
__device__ __forceinline__ int back_dz(int k) { return k == 0 ? 0 : -1; }
__device__ __forceinline__ int back_dy(int k) { return k < 2 ? -1 : k - 2; }

// relaxed loads that the compiler may not keep in a register; `Lds` picks the scope
template <bool Lds>
__device__ __forceinline__ int load_parent(const int *p) {
    return Lds ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above v: strictly decreasing indices (the invariant), so it ends
template <bool Lds>
__device__ __forceinline__ int find_root(const int *parent, int v) {
    int p;
    while ((p = load_parent<Lds>(parent + v)) != v) v = p;
    return v;
}

// Unites the components of the foreground voxels a and b.  Each turn either ends or goes on from the
// old parent of the larger root, which is below it: a + b strictly falls.
template <bool Lds>
__device__ __forceinline__ void unite(int *parent, int a, int b) {
    for (;;) {
        a = find_root<Lds>(parent, a);
        b = find_root<Lds>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);  // only ever lowers parent[a]
        if (old == a) return;                      // a was a root and now hangs under b
        a = old;  // a hung under `old` already (old < a): whichever of old, b the link kept, join the two
    }
}

// Which lanes unite with the voxel at dx = 0, -1, +1 of a neighbour row, from the two rows' foreground
// masks.  m_left / m_right: the neighbour row's mask seen from one voxel to the right / left.  A lane
// skips what other links imply: dx = 0 when the pair to its left is joined too (both rows run on), and
// a diagonal when the voxel straight across is foreground (it joins, and the neighbour row runs on).
struct Needs {
    u64 straight, left, right;
};
__device__ __forceinline__ Needs needs_of(u64 m_row, u64 m_nbr, u64 m_left, u64 m_right, bool straight, bool diagonal) {
    const u64 both = straight ? (m_row & m_nbr) : 0;
    Needs n;
    n.straight = both & ~(both << 1);
    n.left = diagonal ? (m_row & m_left & ~m_nbr) : 0;
    n.right = diagonal ? (m_row & m_right & ~m_nbr) : 0;
    return n;
}

// ---- pass 1: tile-local labelling in LDS ----
__global__ __launch_bounds__(kLabelThreads) void k_label_tiles(const uint8_t *__restrict__ mask,
                                                               int *__restrict__ parent, LabelDims d, int tx_n,
                                                               int ty_n, int64_t n_tiles) {
    __shared__ int lp[kTileVoxels];  // the tile's forest over local indices (row * 64 + lane), -1 = background
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int x0 = (int)(tile % tx_n) * kLabelTileX;
        const int y0 = (int)((tile / tx_n) % ty_n) * kLabelTileY;
        const int z0 = (int)(tile / ((int64_t)tx_n * ty_n)) * kLabelTileZ;
        const int x = x0 + lane;
        // every foreground voxel starts at the first voxel of its x-run: local order is raster order
        for (int r = wave; r < kTileRows; r += kLabelWaves) {
            const int y = y0 + (r % kLabelTileY), z = z0 + (r / kLabelTileY);
            const bool fg = x < d.nx && y < d.ny && z < d.nz && mask[((int64_t)z * d.ny + y) * d.nx + x] != 0;
            const u64 m = __ballot(fg);
            const u64 gaps = ~m & (((u64)1 << lane) - 1);  // background voxels in front of this lane
            const int start = gaps ? 64 - __clzll(gaps) : 0;
            lp[r * 64 + lane] = fg ? r * 64 + start : -1;
        }
        __syncthreads();
        for (int r = wave; r < kTileRows; r += kLabelWaves) {
            const int ty = r % kLabelTileY, tz = r / kLabelTileY;
            const int mine = r * 64 + lane;
            const u64 m_row = __ballot(lp[mine] >= 0);
            if (!m_row) continue;
            for (int k = 0; k < 4; ++k) {
                const int nonzero = (back_dz(k) != 0) + (back_dy(k) != 0);
                const int nty = ty + back_dy(k), ntz = tz + back_dz(k);
                if (nonzero > d.max_nonzero || nty < 0 || nty >= kLabelTileY || ntz < 0) continue;
                const int nbr = (ntz * kLabelTileY + nty) * 64 + lane;
                const u64 m_nbr = __ballot(lp[nbr] >= 0);  // -1 or not: unions do not change it
                const Needs n = needs_of(m_row, m_nbr, m_nbr << 1, m_nbr >> 1, true, nonzero + 1 <= d.max_nonzero);
                if ((n.straight >> lane) & 1) unite<true>(lp, mine, nbr);
                if ((n.left >> lane) & 1) unite<true>(lp, mine, nbr - 1);    // never lane 0: bit 0 of m << 1 is 0
                if ((n.right >> lane) & 1) unite<true>(lp, mine, nbr + 1);   // never lane 63
            }
        }
        __syncthreads();
        for (int r = wave; r < kTileRows; r += kLabelWaves) {
            const int y = y0 + (r % kLabelTileY), z = z0 + (r / kLabelTileY);
            if (x < d.nx && y < d.ny && z < d.nz) {
                int g = -1;
                if (lp[r * 64 + lane] >= 0) {
                    const int root = find_root<true>(lp, r * 64 + lane), rr = root >> 6;
                    g = (int)(((int64_t)(z0 + rr / kLabelTileY) * d.ny + (y0 + rr % kLabelTileY)) * d.nx + x0 + (root & 63));
                }
                parent[((int64_t)z * d.ny + y) * d.nx + x] = g;
            }
        }
        __syncthreads();  // the next tile of this block reuses lp
    }
}

// ---- pass 2: unions across tile boundaries ----
// One wave per 64-voxel x-segment of a row (a tile row's extent in x).  Per backward row the wave
// decides uniformly whether that row lies in another tile; if not, only lane 0 (dx = -1) and lane 63
// (dx = +1) look across a boundary.  k = -1 is the voxel's own row: its dx = -1 at lane 0.
__global__ __launch_bounds__(kLabelThreads) void k_label_borders(int *__restrict__ parent, LabelDims d, int seg_n,
                                                                 int64_t n_segs) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kLabelWaves;
    for (int64_t s = (int64_t)blockIdx.x * kLabelWaves + (threadIdx.x >> 6); s < n_segs; s += waves) {
        const int64_t row = s / seg_n;
        const int x = (int)(s % seg_n) * 64 + lane, y = (int)(row % d.ny), z = (int)(row / d.ny);
        const bool in = x < d.nx;
        const int v = (int)(row * d.nx + x);  // below 2^31 wherever `in`
        const u64 m_row = __ballot(in && load_parent<false>(parent + v) >= 0);
        if (!m_row) continue;
        for (int k = -1; k < 4; ++k) {
            const int dz = k < 0 ? 0 : back_dz(k), dy = k < 0 ? 0 : back_dy(k);
            const int nonzero = (dz != 0) + (dy != 0);
            const int nz_ = z + dz, ny_ = y + dy;
            if (nonzero > d.max_nonzero || nz_ < 0 || ny_ < 0 || ny_ >= d.ny) continue;
            const bool diagonal = nonzero + 1 <= d.max_nonzero;
            const bool other_tile = nz_ / kLabelTileZ != z / kLabelTileZ || ny_ / kLabelTileY != y / kLabelTileY;
            if (!other_tile && !diagonal) continue;
            const int nbr = (int)(((int64_t)nz_ * d.ny + ny_) * d.nx + x);
            // the neighbour row's mask; of the voxel's own row only the step to the left matters
            const u64 m_nbr = k < 0 ? 0 : __ballot(in && load_parent<false>(parent + nbr) >= 0);
            u64 edge_l = 0, edge_r = 0;  // the neighbour row's voxels next to this segment's ends
            if (diagonal) {
                edge_l = __ballot(lane == 0 && x > 0 && load_parent<false>(parent + nbr - 1) >= 0);
                if (k >= 0) edge_r = __ballot(lane == 63 && x + 1 < d.nx && load_parent<false>(parent + nbr + 1) >= 0);
            }
            const u64 m_left = other_tile ? ((m_nbr << 1) | edge_l) : edge_l;
            const u64 m_right = other_tile ? ((m_nbr >> 1) | edge_r) : edge_r;
            const Needs n = needs_of(m_row, m_nbr, m_left, m_right, other_tile, diagonal);
            if ((n.straight >> lane) & 1) unite<false>(parent, v, nbr);
            if ((n.left >> lane) & 1) unite<false>(parent, v, nbr - 1);
            if ((n.right >> lane) & 1) unite<false>(parent, v, nbr + 1);
        }
    }
}

// ---- pass 3: every foreground voxel points at its root; the roots are flagged ----
__global__ __launch_bounds__(kLabelThreads) void k_label_flatten(int *__restrict__ parent, uint8_t *__restrict__ flag,
                                                                 int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kLabelThreads;
    for (int64_t i = (int64_t)blockIdx.x * kLabelThreads + threadIdx.x; i < n; i += stride) {
        const int p = load_parent<false>(parent + i);
        uint8_t f = 0;
        if (p >= 0) {
            const int root = find_root<false>(parent, p);
            if (root != p) parent[i] = root;  // lowers it; a root's own entry never changes here
            f = root == (int)i;
        }
        flag[i] = f;
    }
}

struct Widen {
    __host__ __device__ uint32_t operator()(uint8_t v) const { return v; }
};

// ---- pass 4: labels = rank of the root + 1; sizes and the foreground count by integer atomics ----
__global__ __launch_bounds__(kLabelThreads) void k_label_number(const int *__restrict__ parent,
                                                                const uint32_t *__restrict__ rank,
                                                                int32_t *__restrict__ labels, u64 *__restrict__ sizes,
                                                                u64 *__restrict__ n_foreground, int64_t n) {
    __shared__ unsigned block_fg, block_bg;
    if (threadIdx.x == 0) block_fg = block_bg = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kLabelThreads;
    unsigned wave_fg = 0, wave_all = 0;
    for (int64_t base = (int64_t)blockIdx.x * kLabelThreads; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        int label = 0;
        if (i < n) {
            const int p = parent[i];
            label = p >= 0 ? (int)rank[p] + 1 : 0;
            labels[i] = label;
        }
        const u64 m_fg = __ballot(label > 0);
        wave_fg += (unsigned)__popcll(m_fg);
        wave_all += (unsigned)__popcll(__ballot(i < n));
        if (sizes && m_fg) {
            // the lanes that share the first foreground lane's label add once; the others one by one
            const int first = __shfl(label, __ffsll((long long)m_fg) - 1);
            const u64 m_same = __ballot(label == first);
            if (label == first) {
                if (lane == __ffsll((long long)m_same) - 1) atomicAdd(sizes + first, (u64)__popcll(m_same));
            } else if (label > 0) {
                atomicAdd(sizes + label, (u64)1);
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&block_fg, wave_fg);
        atomicAdd(&block_bg, wave_all - wave_fg);
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_fg) atomicAdd(n_foreground, (u64)block_fg);
    if (threadIdx.x == 0 && sizes && block_bg) atomicAdd(sizes, (u64)block_bg);
}

unsigned grid_for(int64_t items, int per_block) {
    const int64_t blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 1 ? 1 : (blocks > (int64_t)kMaxGrid ? (int64_t)kMaxGrid : blocks));
}

}  // namespace

int run_label(LabelWork &w, const LabelDims &d, const uint8_t *mask, int32_t *labels, int64_t *sizes, bool own_sizes,
              hipStream_t s, Event ev[3], unsigned long long *pinned, int64_t *n_components, int64_t *n_foreground) {
    const int64_t n = d.voxels();
    PTV_TRY(w.parent.ensure((size_t)n));
    PTV_TRY(w.flag.ensure((size_t)n));
    PTV_TRY(w.rank.ensure((size_t)n));
    PTV_TRY(w.counts.ensure(1));
    const int tx_n = (d.nx + kLabelTileX - 1) / kLabelTileX, ty_n = (d.ny + kLabelTileY - 1) / kLabelTileY;
    const int tz_n = (d.nz + kLabelTileZ - 1) / kLabelTileZ;
    const int64_t n_tiles = (int64_t)tx_n * ty_n * tz_n, n_segs = (int64_t)tx_n * d.ny * d.nz;
    hipcub::TransformInputIterator<uint32_t, Widen, const uint8_t *> flags(w.flag.p, Widen());
    size_t tb = 0;
    PTV_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flags, w.rank.p, (int)n, s));
    PTV_TRY(w.temp.ensure(tb));
    pinned[0] = pinned[1] = pinned[2] = 0;

    PTV_TRY(ev[0].record(s));
    hipLaunchKernelGGL(k_label_tiles, dim3(grid_for(n_tiles, 1)), dim3(kLabelThreads), 0, s, mask, w.parent.p, d, tx_n,
                       ty_n, n_tiles);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_label_borders, dim3(grid_for(n_segs, kLabelWaves)), dim3(kLabelThreads), 0, s, w.parent.p, d,
                       tx_n, n_segs);
    PTV_HIP(hipGetLastError());
    PTV_TRY(ev[1].record(s));
    hipLaunchKernelGGL(k_label_flatten, dim3(grid_for(n, kLabelThreads)), dim3(kLabelThreads), 0, s, w.parent.p,
                       w.flag.p, n);
    PTV_HIP(hipGetLastError());
    PTV_HIP(hipcub::DeviceScan::ExclusiveSum(w.temp.p, tb, flags, w.rank.p, (int)n, s));
    // the component count: the last voxel's rank, plus one if it is a root itself
    PTV_HIP(hipMemcpyAsync(&pinned[0], w.rank.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipMemcpyAsync(&pinned[1], w.flag.p + (n - 1), sizeof(uint8_t), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));  // the count sizes `sizes`
    const int64_t nc = (int64_t)(pinned[0] & 0xffffffffull) + (int64_t)(pinned[1] & 0xffull);
    if (own_sizes) {
        PTV_TRY(w.sizes.ensure((size_t)nc + 1));
        sizes = w.sizes.p;
    }
    if (sizes) PTV_HIP(hipMemsetAsync(sizes, 0, ((size_t)nc + 1) * sizeof(int64_t), s));
    PTV_HIP(hipMemsetAsync(w.counts.p, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_label_number, dim3(grid_for(n, kLabelThreads)), dim3(kLabelThreads), 0, s, w.parent.p,
                       w.rank.p, labels, reinterpret_cast<u64 *>(sizes), w.counts.p, n);
    PTV_HIP(hipGetLastError());
    PTV_HIP(hipMemcpyAsync(&pinned[2], w.counts.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PTV_TRY(ev[2].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    *n_components = nc;
    *n_foreground = (int64_t)pinned[2];
    return PTV_OK;
}

}  // namespace ptv
