// ptv_surface.hip — marching cubes of a label mask on the device: every requested label's indicator
// (mask == label, level 0.5) triangulated by the project's own rule in one
// pass over the volume, whatever the number of labels.
//
// One lane per lattice point, x fastest across the wave, so the eight corner loads are runs of
// rows.  The lane owns the point's three edges (towards +z, +y, +x) and the cube whose origin the
// point is.
//   classify  per point the vertices it owns per axis (0..2: an edge between two requested labels
//             carries one vertex for each) and the triangles of its cube, summed over the at most 8
//             distinct requested labels among the corners; one byte each.
//   scan      exclusive sums of both (hipCUB) and their totals; the host reads the totals (the one
//             synchronisation that sizes the outputs) and allocates.
//   emit      the same lanes write their vertices and triangles at their offsets, with the label slot
//             as key: the emitted order is (point, axis) and (cube, table order), across labels.
//   sort      a stable radix sort by slot brings each label together and keeps that order inside it;
//             the vertex permutation is inverted and the faces rewritten.
// No atomic assigns a position and no floating-point atomic exists here: two calls give the same
// bytes.  The mask is read once in classify and, around the interfaces only, once more in emit.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <string>

#include "ptv_common.hpp"
#include "ptv_mc_table.hpp"
#include "ptv_surface.hpp"

namespace ptv {

namespace {

constexpr int kSurfThreads = 256;

// the slot of label v in the ascending table, -1 if it is not requested (0 and below never are)
__device__ inline int find_slot(const int32_t *__restrict__ labels, int nl, int v) {
    if (v <= 0) return -1;
    int lo = 0, hi = nl;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (labels[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nl && labels[lo] == v) ? lo : -1;
}

// What one lattice point sees: its cube's corner values (a corner beyond the lattice repeats corner
// 0, so its edge never crosses), their slots, and which corners are the first of a requested label.
struct PointView {
    int v[8], sl[8];
    unsigned first;  // bit c: corner c holds a requested label that no earlier corner holds
    unsigned req;    // bit c: corner c holds a requested label
    bool cube;       // the point is the origin of a cube
    bool flat;       // all eight corners hold the same value: nothing to do
};

__device__ inline void view_point(const SurfDims &d, const int32_t *__restrict__ mask,
                                  const int32_t *__restrict__ labels, int nl, int iz, int iy, int ix, PointView &pv) {
    const bool hz = iz + 1 < d.lz, hy = iy + 1 < d.ly, hx = ix + 1 < d.lx;
    pv.cube = hz && hy && hx;
    const int64_t st = d.step;
    const int64_t base = ((int64_t)iz * st * d.ny + (int64_t)iy * st) * d.nx + (int64_t)ix * st;
    const int64_t oz = st * d.ny * (int64_t)d.nx, oy = st * d.nx, ox = st;
    bool same = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool ok = (!(c & 4) || hz) && (!(c & 2) || hy) && (!(c & 1) || hx);
        pv.v[c] = ok ? mask[base + ((c & 4) ? oz : 0) + ((c & 2) ? oy : 0) + ((c & 1) ? ox : 0)] : (c ? pv.v[0] : 0);
        same = same && pv.v[c] == pv.v[0];
    }
    pv.flat = same;
    pv.first = pv.req = 0;
    if (same) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int dup = -1;
#pragma unroll
        for (int k = 0; k < c; ++k)
            if (dup < 0 && pv.v[k] == pv.v[c]) dup = k;
        if (dup >= 0) {
            pv.sl[c] = pv.sl[dup];
        } else {
            pv.sl[c] = find_slot(labels, nl, pv.v[c]);
            if (pv.sl[c] >= 0) pv.first |= 1u << c;
        }
        if (pv.sl[c] >= 0) pv.req |= 1u << c;
    }
}

// vertices the point owns on its edge towards corner `far` (4: z, 2: y, 1: x)
__device__ inline int edge_verts(const PointView &pv, int far) {
    if (pv.v[0] == pv.v[far]) return 0;
    return (int)(pv.sl[0] >= 0) + (int)(pv.sl[far] >= 0);
}

__device__ inline unsigned case_of(const PointView &pv, int label) {
    unsigned cs = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cs |= (unsigned)(pv.v[k] == label) << k;
    return cs;
}

__device__ inline void point_of(const SurfDims &d, int64_t p, int &iz, int &iy, int &ix) {
    ix = (int)(p % d.lx);
    const int64_t r = p / d.lx;
    iy = (int)(r % d.ly);
    iz = (int)(r / d.ly);
}

// entry np (one past the last point) is written as zero: the scans run over np + 1 entries and
// leave the totals there
__global__ __launch_bounds__(kSurfThreads) void k_mc_classify(SurfDims d, const int32_t *__restrict__ mask,
                                                              const int32_t *__restrict__ labels, int nl,
                                                              uint8_t *__restrict__ vpack, uint8_t *__restrict__ tcnt) {
    __shared__ unsigned char s_cnt[256];
    s_cnt[threadIdx.x] = kMcCount[threadIdx.x];
    __syncthreads();
    const int64_t np = d.points();
    const int64_t p = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
    if (p > np) return;
    unsigned pack = 0, nt = 0;
    if (p < np) {
        int iz, iy, ix;
        point_of(d, p, iz, iy, ix);
        PointView pv;
        view_point(d, mask, labels, nl, iz, iy, ix, pv);
        if (!pv.flat) {
            pack = (unsigned)edge_verts(pv, 4) | ((unsigned)edge_verts(pv, 2) << 2) | ((unsigned)edge_verts(pv, 1) << 4);
            if (pv.cube) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (pv.first >> c & 1u) nt += s_cnt[case_of(pv, pv.v[c])];
            }
        }
    }
    vpack[p] = (uint8_t)pack;
    tcnt[p] = (uint8_t)nt;  // at most 8 labels x 5 triangles
}

struct PackCount {
    __host__ __device__ uint32_t operator()(uint8_t p) const { return (p & 3u) + ((p >> 2) & 3u) + ((p >> 4) & 3u); }
};
struct PackCount64 {
    __host__ __device__ unsigned long long operator()(uint8_t p) const {
        return (p & 3u) + ((p >> 2) & 3u) + ((p >> 4) & 3u);
    }
};
struct Widen {
    __host__ __device__ uint32_t operator()(uint8_t p) const { return p; }
};
struct Widen64 {
    __host__ __device__ unsigned long long operator()(uint8_t p) const { return p; }
};

__global__ __launch_bounds__(kSurfThreads) void k_mc_emit(SurfDims d, const int32_t *__restrict__ mask,
                                                          const int32_t *__restrict__ labels, int nl,
                                                          const uint8_t *__restrict__ vpack,
                                                          const uint8_t *__restrict__ tcnt,
                                                          const uint32_t *__restrict__ voff,
                                                          const uint32_t *__restrict__ toff, uint32_t nv, uint32_t ntri,
                                                          uint32_t *__restrict__ vkey, uint32_t *__restrict__ vval,
                                                          float *__restrict__ vtmp, uint32_t *__restrict__ tkey,
                                                          uint32_t *__restrict__ tval, uint32_t *__restrict__ tfaces) {
    __shared__ unsigned char s_cnt[256];
    __shared__ unsigned char s_edges[256 * 16];
    s_cnt[threadIdx.x] = kMcCount[threadIdx.x];
    for (int i = threadIdx.x; i < 256 * 16; i += kSurfThreads) s_edges[i] = kMcEdges[i >> 4][i & 15];
    __syncthreads();
    const int64_t np = d.points();
    const int64_t p = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
    if (p >= np) return;
    const unsigned pack = vpack[p], nt = tcnt[p];
    if (pack == 0 && nt == 0) return;  // away from every interface: the mask is not read again
    int iz, iy, ix;
    point_of(d, p, iz, iy, ix);
    PointView pv;
    view_point(d, mask, labels, nl, iz, iy, ix, pv);
    if (pv.flat) return;
    // vertices: axis z, y, x; on an edge the lower end's label first
    uint32_t vi = voff[p];
    const float half = 0.5f * (float)d.step;
    const float pz = (float)((int64_t)iz * d.step), py = (float)((int64_t)iy * d.step),
                px = (float)((int64_t)ix * d.step);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int far = 4 >> a;
        if (pv.v[0] == pv.v[far]) continue;
#pragma unroll
        for (int end = 0; end < 2; ++end) {
            const int slot = end ? pv.sl[far] : pv.sl[0];
            if (slot < 0) continue;
            if (vi < nv) {
                vkey[vi] = (uint32_t)slot;
                vval[vi] = vi;
                vtmp[3 * (size_t)vi + 0] = pz + (a == 0 ? half : 0.f);
                vtmp[3 * (size_t)vi + 1] = py + (a == 1 ? half : 0.f);
                vtmp[3 * (size_t)vi + 2] = px + (a == 2 ? half : 0.f);
            }
            ++vi;
        }
    }
    if (!pv.cube || nt == 0) return;
    uint32_t ti = toff[p];
    const int64_t sy = d.lx, sz = (int64_t)d.lx * d.ly;
#pragma unroll  // keeps pv.v / pv.sl in registers (no dynamic index)
    for (int c = 0; c < 8; ++c) {
        if (!(pv.first >> c & 1u)) continue;
        const unsigned cs = case_of(pv, pv.v[c]);
        const int n = s_cnt[cs];
        const uint32_t slot = (uint32_t)pv.sl[c];
        for (int t = 0; t < n; ++t, ++ti) {
            if (ti >= ntri) continue;
            tkey[ti] = slot;
            tval[ti] = ti;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = s_edges[cs * 16 + 3 * t + j];
                // edge e: axis a = e / 4, lower corner = the e % 4-th corner whose bit of that axis is clear
                const int a = e >> 2, r = e & 3;
                const int lc = a == 0 ? r : a == 1 ? ((r & 2) << 1) | (r & 1) : r << 1;
                const int64_t q = p + ((lc & 4) ? sz : 0) + ((lc & 2) ? sy : 0) + (lc & 1);
                const unsigned pk = vpack[q];
                const uint32_t rank = a == 0 ? 0u : a == 1 ? (pk & 3u) : (pk & 3u) + ((pk >> 2) & 3u);
                // the label is the edge's lower end, or its upper end behind the lower end's own vertex
                const uint32_t behind = (cs >> lc & 1u) ? 0u : (pv.req >> lc & 1u);
                tfaces[3 * (size_t)ti + j] = voff[q] + rank + behind;
            }
        }
    }
}

// first[l] = the first sorted entry whose key is >= l, for l in [0, nl]
__global__ void k_mc_bounds(const uint32_t *__restrict__ keys, int64_t n, int nl, int64_t *__restrict__ first) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > nl) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < (uint32_t)l) lo = mid + 1;
        else hi = mid;
    }
    first[l] = lo;
}

__global__ __launch_bounds__(kSurfThreads) void k_mc_gather_verts(const uint32_t *__restrict__ vperm, uint32_t nv,
                                                                  const float *__restrict__ vtmp,
                                                                  float *__restrict__ verts,
                                                                  uint32_t *__restrict__ vinv) {
    const int64_t j = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
    if (j >= nv) return;
    const uint32_t i = vperm[j];
    if (i >= nv) return;
    verts[3 * j + 0] = vtmp[3 * (size_t)i + 0];
    verts[3 * j + 1] = vtmp[3 * (size_t)i + 1];
    verts[3 * j + 2] = vtmp[3 * (size_t)i + 2];
    vinv[i] = (uint32_t)j;
}

__global__ __launch_bounds__(kSurfThreads) void k_mc_gather_faces(const uint32_t *__restrict__ tperm, uint32_t ntri,
                                                                  const uint32_t *__restrict__ tfaces,
                                                                  const uint32_t *__restrict__ vinv, uint32_t nv,
                                                                  int32_t *__restrict__ faces) {
    const int64_t j = (int64_t)blockIdx.x * kSurfThreads + threadIdx.x;
    if (j >= ntri) return;
    const uint32_t i = tperm[j];
    if (i >= ntri) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = tfaces[3 * (size_t)i + k];
        faces[3 * j + k] = v < nv ? (int32_t)vinv[v] : 0;
    }
}

int sort_by_slot(SurfWork &w, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals, uint32_t *vals_out,
                 uint32_t n, int nl, hipStream_t s) {
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < nl) ++bits;
    size_t tb = 0;
    PTV_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, keys_out, vals, vals_out, (int)n, 0, bits, s));
    PTV_TRY(w.temp.ensure(tb));
    PTV_HIP(hipcub::DeviceRadixSort::SortPairs(w.temp.p, tb, keys, keys_out, vals, vals_out, (int)n, 0, bits, s));
    return PTV_OK;
}

}  // namespace

int run_marching_cubes(SurfWork &w, const SurfDims &d, const int32_t *mask, const int32_t *labels, int nl,
                       hipStream_t s, Event ev[3], unsigned long long *pinned) {
    w.n_labels = 0;  // nothing valid until the passes are through
    const int64_t np = d.points();
    const size_t n1 = (size_t)np + 1;
    const unsigned grid1 = (unsigned)((n1 + kSurfThreads - 1) / kSurfThreads);
    PTV_TRY(w.labels.ensure((size_t)nl));
    PTV_TRY(w.vpack.ensure(n1));
    PTV_TRY(w.tcnt.ensure(n1));
    PTV_TRY(w.voff.ensure(n1));
    PTV_TRY(w.toff.ensure(n1));
    PTV_TRY(w.totals.ensure(2));
    PTV_TRY(w.bounds.ensure(2 * ((size_t)nl + 1)));
    PTV_HIP(hipMemcpyAsync(w.labels.p, labels, (size_t)nl * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PTV_TRY(ev[0].record(s));
    hipLaunchKernelGGL(k_mc_classify, dim3(grid1), dim3(kSurfThreads), 0, s, d, mask, w.labels.p, nl, w.vpack.p,
                       w.tcnt.p);
    PTV_HIP(hipGetLastError());
    {
        hipcub::TransformInputIterator<uint32_t, PackCount, const uint8_t *> vin(w.vpack.p, PackCount());
        hipcub::TransformInputIterator<uint32_t, Widen, const uint8_t *> tin(w.tcnt.p, Widen());
        hipcub::TransformInputIterator<unsigned long long, PackCount64, const uint8_t *> vin64(w.vpack.p, PackCount64());
        hipcub::TransformInputIterator<unsigned long long, Widen64, const uint8_t *> tin64(w.tcnt.p, Widen64());
        size_t tb = 0, tb2 = 0;
        PTV_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, vin, w.voff.p, (int)n1, s));
        PTV_HIP(hipcub::DeviceReduce::Sum(nullptr, tb2, vin64, w.totals.p, (int)n1, s));
        PTV_TRY(w.temp.ensure(tb > tb2 ? tb : tb2));
        // 64-bit totals first: the 32-bit offsets are used only when both are below 2^31
        PTV_HIP(hipcub::DeviceReduce::Sum(w.temp.p, tb2, vin64, w.totals.p + 0, (int)n1, s));
        PTV_HIP(hipcub::DeviceReduce::Sum(w.temp.p, tb2, tin64, w.totals.p + 1, (int)n1, s));
        PTV_HIP(hipcub::DeviceScan::ExclusiveSum(w.temp.p, tb, vin, w.voff.p, (int)n1, s));
        PTV_HIP(hipcub::DeviceScan::ExclusiveSum(w.temp.p, tb, tin, w.toff.p, (int)n1, s));
    }
    PTV_TRY(ev[1].record(s));
    PTV_HIP(hipMemcpyAsync(pinned, w.totals.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));  // the totals size the outputs
    const unsigned long long nv = pinned[0], nt = pinned[1];
    if (nv >= (1ull << 31) || nt >= (1ull << 31)) {
        set_error("marching cubes: 2^31 or more vertices or triangles");
        return PTV_E_UNSUPPORTED;
    }
    w.vstart.assign((size_t)nl + 1, 0);
    w.tstart.assign((size_t)nl + 1, 0);
    if (nv == 0 || nt == 0) {  // no interface of a requested label inside the lattice
        PTV_TRY(ev[2].record(s));
        PTV_HIP(hipStreamSynchronize(s));
        w.n_labels = nl;
        return PTV_OK;
    }
    for (DevBuf<uint32_t> *b : {&w.vkey, &w.vkey2, &w.vval, &w.vperm, &w.vinv}) PTV_TRY(b->ensure((size_t)nv));
    for (DevBuf<uint32_t> *b : {&w.tkey, &w.tkey2, &w.tval, &w.tperm}) PTV_TRY(b->ensure((size_t)nt));
    PTV_TRY(w.tfaces.ensure(3 * (size_t)nt));
    PTV_TRY(w.vtmp.ensure(3 * (size_t)nv));
    PTV_TRY(w.verts.ensure(3 * (size_t)nv));
    PTV_TRY(w.faces.ensure(3 * (size_t)nt));
    const unsigned grid = (unsigned)((np + kSurfThreads - 1) / kSurfThreads);
    hipLaunchKernelGGL(k_mc_emit, dim3(grid), dim3(kSurfThreads), 0, s, d, mask, w.labels.p, nl, w.vpack.p, w.tcnt.p,
                       w.voff.p, w.toff.p, (uint32_t)nv, (uint32_t)nt, w.vkey.p, w.vval.p, w.vtmp.p, w.tkey.p, w.tval.p,
                       w.tfaces.p);
    PTV_HIP(hipGetLastError());
    PTV_TRY(sort_by_slot(w, w.vkey.p, w.vkey2.p, w.vval.p, w.vperm.p, (uint32_t)nv, nl, s));
    PTV_TRY(sort_by_slot(w, w.tkey.p, w.tkey2.p, w.tval.p, w.tperm.p, (uint32_t)nt, nl, s));
    const unsigned gl = (unsigned)((nl + 1 + 255) / 256);
    hipLaunchKernelGGL(k_mc_bounds, dim3(gl), dim3(256), 0, s, w.vkey2.p, (int64_t)nv, nl, w.bounds.p);
    hipLaunchKernelGGL(k_mc_bounds, dim3(gl), dim3(256), 0, s, w.tkey2.p, (int64_t)nt, nl, w.bounds.p + nl + 1);
    hipLaunchKernelGGL(k_mc_gather_verts, dim3((unsigned)((nv + kSurfThreads - 1) / kSurfThreads)), dim3(kSurfThreads),
                       0, s, w.vperm.p, (uint32_t)nv, w.vtmp.p, w.verts.p, w.vinv.p);
    hipLaunchKernelGGL(k_mc_gather_faces, dim3((unsigned)((nt + kSurfThreads - 1) / kSurfThreads)), dim3(kSurfThreads),
                       0, s, w.tperm.p, (uint32_t)nt, w.tfaces.p, w.vinv.p, (uint32_t)nv, w.faces.p);
    PTV_HIP(hipGetLastError());
    PTV_TRY(ev[2].record(s));
    PTV_HIP(hipMemcpyAsync(w.vstart.data(), w.bounds.p, ((size_t)nl + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipMemcpyAsync(w.tstart.data(), w.bounds.p + nl + 1, ((size_t)nl + 1) * sizeof(int64_t),
                           hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    w.n_labels = nl;
    return PTV_OK;
}

}  // namespace ptv
