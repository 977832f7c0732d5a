// ptv_label.hpp — host-side launcher of ptv_label.hip: connected-component labelling of a 3-D byte
// mask with scipy.ndimage.label's numbering.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ptv_own.hpp"

namespace ptv {

// The tile of the tile-local pass: one block labels kLabelTileZ x kLabelTileY x kLabelTileX voxels
// with its parent array in LDS; x spans exactly one wave.  The tests derive their tile-edge shapes
// from these three numbers (ptv_interpolation_amd.labelling.TILE repeats them).
constexpr int kLabelTileX = 64;
constexpr int kLabelTileY = 8;
constexpr int kLabelTileZ = 8;

// the volume (nz, ny, nx), C order, and how many neighbour offsets may be nonzero at once:
// 1, 2, 3 for 6, 18, 26 neighbours
struct LabelDims {
    int nx, ny, nz, max_nonzero;
    __host__ __device__ int64_t voxels() const { return (int64_t)nx * ny * nz; }
};

// scratch of the passes (owned by the context, grow-only)
struct LabelWork {
    DevBuf<int32_t> parent;             // the union-find forest over linear voxel indices, -1 = background
    DevBuf<uint8_t> flag, temp;         // 1 at a root; the scan's scratch
    DevBuf<uint32_t> rank;              // exclusive sum of the flags: a root's rank in raster order
    DevBuf<unsigned long long> counts;  // foreground voxels
    DevBuf<int64_t> sizes;              // component sizes of a host call
};

// Labels the device uint8 `mask` (nonzero = foreground) into the device int32 `labels`.  sizes (device,
// may be NULL) receives n_components + 1 counts, background first; own_sizes puts them into w.sizes
// instead (grown once the count is known).  Synchronises the stream twice: once for the component
// count (it sizes `sizes`), once at the end.  ev[0..2] are recorded at the start, after the border
// merge and at the end.  pinned: four words of pinned host memory.
int run_label(LabelWork &w, const LabelDims &d, const uint8_t *mask, int32_t *labels, int64_t *sizes, bool own_sizes,
              hipStream_t s, Event ev[3], unsigned long long *pinned, int64_t *n_components, int64_t *n_foreground);

}  // namespace ptv
