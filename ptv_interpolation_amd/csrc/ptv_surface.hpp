// ptv_surface.hpp — host-side launcher of ptv_surface.hip: marching cubes of all requested labels'
// indicators in one pass over the label mask, by the project's own triangulation rule (DESIGN.md
// section 23, table ptv_mc_table.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "ptv_own.hpp"

namespace ptv {

// the mask (nz, ny, nx) and its lattice: the voxels whose indices are multiples of `step`
struct SurfDims {
    int nx, ny, nz, step;
    int lx, ly, lz;  // lattice points per axis; cubes per axis = points - 1
    __host__ __device__ int64_t points() const { return (int64_t)lx * ly * lz; }
};

// scratch of the passes and the resident mesh they leave (owned by the context)
struct SurfWork {
    DevBuf<int32_t> labels;                   // the sorted label table
    DevBuf<uint8_t> vpack, tcnt, temp;        // per lattice point: vertices per axis (2 bits each), triangles
    DevBuf<uint32_t> voff, toff;              // their exclusive sums
    DevBuf<unsigned long long> totals;        // vertices, triangles
    DevBuf<uint32_t> vkey, vkey2, vval, vperm, vinv;  // per vertex: label slot (emitted, sorted), index, order
    DevBuf<uint32_t> tkey, tkey2, tval, tperm, tfaces;  // the same per triangle; faces in emitted vertex numbers
    DevBuf<float> vtmp;                       // vertices as emitted
    DevBuf<int64_t> bounds;                   // 2 (n_labels + 1): first vertex, first triangle per label
    // the resident mesh: vertices [z, y, x] float32 by label, faces indexing all labels' vertices together
    DevBuf<float> verts;
    DevBuf<int32_t> faces;
    std::vector<int64_t> vstart, tstart;      // n_labels + 1 each (host copies of `bounds`)
    int n_labels = 0;                         // 0: the context holds no mesh
};

// Triangulates the `nl` labels (host, ascending, distinct, positive) of the device int32 `mask` into
// w.verts / w.faces / w.vstart / w.tstart.  Synchronises the stream twice: once for the two totals
// that size the output buffers (allocated between the passes), once for the per-label offsets it
// returns.  ev[0..2] are recorded before the counting passes, between them and the emission, and at
// the end.  pinned: two words of pinned host memory.
int run_marching_cubes(SurfWork &w, const SurfDims &d, const int32_t *mask, const int32_t *labels, int nl,
                       hipStream_t s, Event ev[3], unsigned long long *pinned);

}  // namespace ptv
