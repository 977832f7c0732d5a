// ptv_mesh.hpp — host-side launchers of ptv_mesh.hip: the cubic B-spline prefilter, the order 0 / 1 /
// 3 sampling and the mesh interface drag's traction integration.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptv {

constexpr int kMeshThreads = 256;  // triangles per block of the traction kernel
constexpr int kMeshSums = 21;      // PTV_MESH_SUMS

// the raw field (nz, ny, nx) and what its padded coefficient array measures
struct SplineDims {
    int nx, ny, nz;
    __host__ __device__ int64_t px() const { return (int64_t)nx + 24; }
    __host__ __device__ int64_t py() const { return (int64_t)ny + 24; }
    __host__ __device__ int64_t pz() const { return (int64_t)nz + 24; }
    __host__ __device__ size_t padded() const { return (size_t)px() * (size_t)py() * (size_t)pz(); }
};

// coef = the cubic B-spline coefficients of `field` (float32 when f32, else float64) padded by 12
// edge-replicated samples; coef must not alias field
int launch_spline_prefilter(const SplineDims &d, const void *field, bool f32, double *coef, hipStream_t s);

// out[i] = the sample at (coords[i], coords[n + i], coords[2n + i]); order 3 reads `src` as padded
// coefficients (float64), orders 0 and 1 as the raw field (float32 when f32)
int launch_map_coordinates(const SplineDims &d, int order, const void *src, bool f32, const double *coords,
                           int64_t n, double *out, hipStream_t s);

struct MeshArgs {
    SplineDims d;
    int field_f32, vert_f32;
    int64_t n_verts, n_tris;
    int n_labels;
    double h[3];  // dz, dy, dx
    double viscosity;
};
// blocks of the traction kernel for the host's tri_offsets (n_labels + 1): a block never spans two labels
int64_t mesh_blocks(const int64_t *tri_offsets, int n_labels);
// coef[3]: the padded coefficients of U, V, W; P and bg may be NULL.  blk_label / blk_first: per
// block its label slot and first triangle; lab_blk0: n_labels + 1 first blocks per label;
// tri_offsets: the device copy.  part: nblocks * kMeshSums doubles; res: n_labels * kMeshSums.
int launch_mesh_drag(const MeshArgs &a, const void *U, const void *V, const void *W, const void *P,
                     const uint8_t *bg, const double *const coef[3], const void *verts, const int32_t *faces,
                     const int64_t *tri_offsets, const int32_t *blk_label, const int64_t *blk_first,
                     const int64_t *lab_blk0, int64_t nblocks, double *part, double *res, hipStream_t s);

}  // namespace ptv
