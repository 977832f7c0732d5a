/*
 * ptv_api.h — C ABI of the MI355X-native PTV scattered-to-grid interpolator.
 *
 * Drop-in boundary for the per-voxel neighbour search + weighted average of
 * the reference `interpolator.interpolate_field` (tombultreys/ptv_interpolation,
 * interpolator.py:65-203).  Plain C types only: pointers + sizes, no torch or
 * HIP types in any signature.  Every entry point returns 0 on success and a
 * negative PTV_E* code on failure; `ptv_last_error()` then holds a message
 * (thread-local).  The Python mirror of the reference interface lives in
 * ptv_interpolation_amd/interpolator.py and binds these symbols with ctypes.
 *
 * Threading: one ptv_ctx per (process, device).  A ctx is not re-entrant;
 * calls on one ctx are synchronous with respect to the host unless the
 * *_dev variant is given a stream, in which case all work is enqueued on
 * that stream and the call returns after the enqueue (the stats fields
 * are filled at the next synchronising call).
 */
#ifndef PTV_API_H
#define PTV_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTV_API_VERSION 11

/* error codes */
#define PTV_OK 0
#define PTV_E_ARG -1      /* invalid argument (Python: ValueError)          */
#define PTV_E_HIP -2      /* HIP runtime / launch failure (RuntimeError)    */
#define PTV_E_NOMEM -3    /* device allocation failed (MemoryError)         */
#define PTV_E_UNSUPPORTED -4 /* valid but not implemented on the GPU path  */
#define PTV_E_INEXACT -5  /* slab_halo too small to prove the culled set exact (see ptv_knn_params) */
#define PTV_E_SINGULAR -6 /* local RBF system singular (Python: LinAlgError) */

/* interpolation methods (interpolator.py:83, :126, :157, :197) */
#define PTV_METHOD_IDW 0
#define PTV_METHOD_SIBSON 1
#define PTV_METHOD_NEAREST 2
/* Extension (no reference counterpart; parity unpinned): IDW over every particle
 * within ptv_knn_params.radius of the voxel (scipy query_ball_point's d2 <= r*r test), weights
 * 1/(d**power + eps) as interpolator.py:142-147, out = sum w u / sum w; an empty ball gives NaN.
 * k is ignored.  BASELINE config 2 ("IDW radius-search"). */
#define PTV_METHOD_IDW_RADIUS 3

/* local RBF kernels (scipy RBFInterpolator names, _rbfinterp.py:19-28) */
#define PTV_RBF_LINEAR 0
#define PTV_RBF_THIN_PLATE_SPLINE 1
#define PTV_RBF_CUBIC 2
#define PTV_RBF_QUINTIC 3
#define PTV_RBF_MULTIQUADRIC 4
#define PTV_RBF_INVERSE_MULTIQUADRIC 5
#define PTV_RBF_INVERSE_QUADRATIC 6
#define PTV_RBF_GAUSSIAN 7

/* flags for ptv_knn_params.flags / ptv_rbf_params.flags */
#define PTV_FLAG_NAN_TO_NUM 1u  /* fused main.py:195-199 nan_to_num on the outputs */
/* k-NN methods: write U, V, W as float32 (the buffers passed as `double *` then hold float):
 * the fused `U.astype(np.float32)` of main.py:230, applied after the float64 result, the
 * nan_to_num and the mask (half the output bytes).  Arithmetic stays float64. */
#define PTV_FLAG_OUT_F32 2u
/* local RBF, diagnostics: SPD systems through the LDS-broadcast kernel (k_rbf_spd, the one the
 * register kernel's out-of-range-pivot rerun uses) instead of k_rbf_spd16 (ABI v8) */
#define PTV_FLAG_RBF_SPD_LDS 4u
/* local RBF, diagnostics: the scale-invariant kernels through the partial-pivoting solver
 * (k_rbf_local) instead of the null-space solver k_rbf_ns (ABI v9) */
#define PTV_FLAG_RBF_PIVOTING 8u
/* k-NN, diagnostics (k >= 13): near-tie repair list of one entry, so that a launch with two or more
 * tiles to repair takes the whole-launch exact rerun (the path past the 2^22-tile list) (ABI v9) */
#define PTV_FLAG_KNN_REPAIR_ALL 16u
/* k-NN interpolation on a z-slab of a separable grid (z_begin > 0 or z_end < nz): bin only the
 * particles that can be among a slab voxel's k nearest, by a per-(x, y)-column cull map (ABI v10).
 * Replaces the scalar slab_halo (ignored under this flag) for the multi-GPU z-slab split with the
 * particle set replicated (interpolator.py:173-182 fanned out over GPUs).  The
 * context derives the map from the slab's own finest lattice bounds: every voxel v of a lattice
 * cell Q has d_k(v) <= U(Q) = max over Q's corners of D(c) + Q's half diagonal, so only particles
 * within U(Q) of some cell Q are needed; per column that is a height above / depth below the slab.
 * The first call for a (particle arrays, n, 96-value fingerprint, grid, slab, k, method) key bins
 * every particle and caches the map; later calls cull with it and PROVE on the device, from the
 * lattice of the kept particles, that the map covers what the slab needs before the main kernel
 * runs (a failed proof -- the particles changed under the same arrays -- reruns the call without
 * the cull and refreshes the map).  Results are bit-identical to the unculled call.
 * ptv_stats.n_binned reports the particles kept. */
#define PTV_FLAG_SLAB_CULL_AUTO 32u

typedef struct ptv_ctx ptv_ctx;

/*
 * Particles, structure of arrays, float64 (the reference upcasts every input
 * to float64: interpolator.py:78-79 -> cKDTree / numpy arithmetic).
 * Replaces: `points = df[['x','y','z']].values; values = df[['u','v','w']].values`
 *           (interpolator.py:78-79).
 */
typedef struct {
    int64_t n;
    const double *x, *y, *z; /* positions */
    const double *u, *v, *w; /* velocity components */
} ptv_particles;

/*
 * Query grid.  Separable regular grid: the 1-D axes returned by
 * `create_grid` (interpolator.py:54-56) — voxel (iz, iy, ix) sits at
 * (ax[ix], ay[iy], az[iz]), C order (nz, ny, nx) with x fastest exactly as
 * `np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)` (interpolator.py:135).
 * Point-list mode: ax/ay/az NULL and px/py/pz hold nx*ny*nz coordinates in
 * the same C order (any grid shape the caller passes, interpolator.py:77).
 * Only planes [z_begin, z_end) are computed (multi-GPU z-slab).
 */
typedef struct {
    int64_t nx, ny, nz;
    const double *ax, *ay, *az;
    const double *px, *py, *pz;
    int64_t z_begin, z_end;
} ptv_grid;

/*
 * k-NN interpolation parameters (interpolate_field kwargs, interpolator.py:65).
 * fluid_mask: optional uint8 (nz, ny, nx) over the FULL grid, nonzero = fluid
 * (interpolator.py:37); solid voxels are written as 0 and skipped
 * (fused main.py:202-207).  NULL = compute every voxel.
 */
typedef struct {
    int method;          /* PTV_METHOD_* */
    int k;               /* idw_neighbors / sibson_neighbors, 1 <= k <= n (k >= 128: the large-k path) */
    double power;        /* idw_power (interpolator.py:143) */
    double eps;          /* 1e-10 (interpolator.py:102, :142) */
    const uint8_t *fluid_mask;
    uint32_t flags;      /* PTV_FLAG_* */
    double cell_occupancy; /* target particles per binning cell, <=0: default */
    double r0_scale;       /* first search radius / expected k-NN radius, <=0: default */
    int lattice_bounds;    /* >=0: coarse-lattice k-th distance bounds (default), <0: off */
    /* Multi-GPU z-slab with the particle set replicated: > 0 bins only the
     * particles whose z lies within slab_halo of the slab's z extent [az[z_begin], az[z_end-1]]
     * (separable grids; order-preserving on-device compaction).  Exactness is then PROVEN
     * before the main kernel: from the finest lattice's k-th distance bounds D(c) every slab
     * voxel v has d_k(v) <= D(c) + |v - c|, and a particle outside the window is farther than
     * slab_halo + (v's distance to the nearer slab face); the call computes the halo that
     * guarantees this (ptv_stats.halo_required) and returns PTV_E_INEXACT without running the
     * interpolation when slab_halo is smaller (retry with halo_required, or 0 = no cull).
     * <= 0: every particle is binned (no check needed).  k-NN interpolation entry points only. */
    double slab_halo;
    double radius;         /* PTV_METHOD_IDW_RADIUS: the search radius (> 0) */
} ptv_knn_params;

/*
 * Local RBF parameters (interpolate_field rbf kwargs, interpolator.py:162-167, and the
 * RBFInterpolator constructor they feed, _rbfinterp.py:258-345).  The caller resolves
 * scipy's defaults and validation first (ptv_interpolation_amd/rbf.py): k is
 * min(neighbors, n) (:322), epsilon is 1.0 for the scale-invariant kernels (:300-309),
 * degree defaults to max(min_degree, 0) (:311-313).
 */
typedef struct {
    int k;                /* rbf_neighbors, 1 <= k <= n */
    int kernel;           /* PTV_RBF_* */
    double epsilon;       /* shape parameter */
    int degree;           /* polynomial degree, -1 = no polynomial (systems k + C(degree+3, 3) > 128:
                           * solved in global memory, k_rbf_huge) */
    double smoothing;     /* scalar smoothing, used when smoothing_per_point is NULL */
    const double *smoothing_per_point; /* optional (n,) array, same memory space as the particles */
    const uint8_t *fluid_mask;        /* as ptv_knn_params.fluid_mask */
    uint32_t flags;       /* PTV_FLAG_* */
    int chunk_planes;     /* z planes per k-NN + solve chunk (multiple of 4), <= 0: automatic */
} ptv_rbf_params;

/* Per-call timings (ms, hipEvent based) and sizes. */
typedef struct {
    double ms_h2d, ms_bin, ms_lattice, ms_knn, ms_d2h, ms_total;
    int64_t n_particles, n_voxels, n_cells;
    int32_t cells[3];
    double cell_size[3];
    double r0;
    double ms_solve;     /* local RBF: the per-voxel solve kernels (ms_knn = their k-NN passes) */
    int64_t n_singular;  /* local RBF: voxels whose system had an exactly zero pivot */
    double ms_stencil;   /* ptv_divergence*: the stencil kernel */
    int64_t n_binned;    /* particles binned (after the slab_halo cull; = n_particles without) */
    double halo_required;/* slab_halo cull: the smallest halo this call proves exact (-1: no cull) */
    double ms_cull;      /* slab_halo cull + exactness check (inside ms_bin / before ms_knn) */
    int64_t n_repair_tiles; /* k >= 13: 4x4x4 tiles rerun with exact (d2, slot) lists because two
                             * distinct distances shared a packed key's truncation (ABI v8) */
    int64_t n_rbf_pivoted;  /* local RBF, scale-invariant kernels: voxels the null-space solver handed
                             * to the partial-pivoting solver (rank-deficient polynomial block, a
                             * non-positive pivot, ...; ABI v9) */
} ptv_stats;

/*
 * Consistent divergence (physics.compute_consistent_divergence, physics.py:6-53).
 * Fields U, V, W and the uint8 fluid mask (nonzero = fluid, required: the reference
 * np.roll()s it, physics.py:31-32) are (nz, ny, nx) C order.  Planes [z_begin, z_end)
 * are written to `out` as (z_end - z_begin, ny, nx).  Plane 0 / nz-1 of the buffer is
 * a domain z edge when edge_lo / edge_hi is set, else a one-plane halo of the
 * neighbouring z-slab that is read but not computed (z-slab multi-GPU).
 * Types follow numpy: field_dtype is the fields' dtype; result_dtype the dtype of
 * (field difference) / spacing — PTV_F32 only for float32 fields with Python-float
 * spacings, PTV_F64 when a spacing is a numpy float64 scalar (view_divergence.py:22).
 */
#define PTV_F64 0
#define PTV_F32 1
typedef struct {
    int64_t nx, ny, nz;
    int64_t z_begin, z_end;
    int edge_lo, edge_hi;
    int field_dtype;     /* PTV_F64 | PTV_F32 */
    int result_dtype;    /* PTV_F64 | PTV_F32 */
    double dx, dy, dz;
    const uint8_t *fluid_mask;
} ptv_div_params;

/*
 * Raw pore mask for sample_mask_on_grid (interpolator.py:205-238).  `raw` is
 * (nz, ny, nx) C order, one byte per voxel, nonzero where the raw value
 * `mask_raw.astype(float)` is > 0.5 (for a bool mask: the mask itself).  The axes are
 * the raw voxel coordinates `linspace(min, max-1, n)` (or `[min]` when n == 1) and are
 * always HOST arrays (n doubles each); `raw` lives in the call's memory space.
 */
typedef struct {
    int64_t nx, ny, nz;
    const uint8_t *raw;
    const double *ax, *ay, *az;
} ptv_mask_grid;

/*
 * Boundary particles (extract_boundary_particles, interpolator.py:240-284).
 * mask: (nz, ny, nx) bytes.  encoding PTV_MASK_BOOL: bytes are 0/1 (a numpy bool mask);
 * PTV_MASK_BITS: bit 1 = (value != 0), bit 0 = (value & 1) (an integer mask, for which
 * numpy's `dilated & ~mask` keeps the low bit only).  Coordinates per axis (x, y, z):
 * lo + (index * span) / den with span = max - 1 - min and den = n - 1
 * (interpolator.py:278-280; the caller handles n == 1, where the reference returns ints).
 */
#define PTV_MASK_BOOL 0
#define PTV_MASK_BITS 1
typedef struct {
    int64_t nx, ny, nz;
    const uint8_t *mask;
    int encoding;          /* PTV_MASK_BOOL | PTV_MASK_BITS */
    int thickness;         /* binary_dilation iterations, >= 1 */
    int64_t sampling_step; /* take every Nth boundary voxel (C order), >= 1 */
    double lo[3], span[3], den[3];
} ptv_boundary_params;

/*
 * k-NN median/MAD outlier filter (filtering.py:5-58 remove_outliers_knn).
 * k: neighbours excluding the point itself (the reference queries k+1, :26), 1 <= k < n
 * (k >= 127: the large-k path);
 * threshold: MAD units (:47-51); mad_eps: 1e-6 (:46).
 */
typedef struct {
    int k;
    double threshold;
    double mad_eps;
} ptv_filter_params;

/*
 * Linear interpolation over a Delaunay triangulation: method='linear', the reference's default
 * (interpolator.py:196-197 `griddata(points, values, grid_coords, method='linear',
 * fill_value=0.0)` -> scipy LinearNDInterpolator).  The caller builds
 * `tri = scipy.spatial.Delaunay(points)` on the host, exactly as LinearNDInterpolator does (Qhull),
 * and passes its arrays; the GPU locates every voxel in it (walk from a simplex incident to the
 * voxel's nearest particle, scipy's brute-force scan where the walk meets a degenerate simplex)
 * and interpolates with scipy's barycentric arithmetic.  Arrays follow numpy's C layouts
 * (int32 / float64) and live in the call's memory space.
 */
typedef struct {
    int64_t nsimplex;
    const int32_t *simplices;         /* (nsimplex, 4) particle indices: tri.simplices */
    const int32_t *neighbors;         /* (nsimplex, 4) tri.neighbors (-1 = hull face) */
    const double *transform;          /* (nsimplex, 4, 3) tri.transform (NaN rows: degenerate) */
    const int32_t *vertex_to_simplex; /* (n,) a simplex incident to each particle (walk start;
                                         tri.vertex_to_simplex with tri.coplanar points filled in) */
    double min_bound[3], max_bound[3];/* tri.min_bound, tri.max_bound */
    double fill_value;                /* griddata fill_value (0.0 in interpolator.py:197) */
    const uint8_t *fluid_mask;        /* as ptv_knn_params.fluid_mask */
    uint32_t flags;                   /* PTV_FLAG_NAN_TO_NUM only */
    int chunk_planes;                 /* z planes per nearest-particle + walk chunk (multiple of 4), <= 0: auto */
} ptv_linear_params;

/*
 * Projection-method divergence cleaning (physics.clean_divergence_projection, physics.py:149-209;
 * ABI v11).  Fields and the uint8 fluid mask (nonzero = fluid, required) are float64 / uint8
 * (nz, ny, nx) C order.  Per outer iteration: the consistent divergence, b = div[fluid] -
 * mean(div[fluid]), scipy.sparse.linalg.lsqr(A, b, damp, atol, btol, iter_lim) (conlim at scipy's
 * default 1e8) on the masked 7-point Laplacian of build_laplacian_matrix (physics.py:55-108) applied
 * matrix-free, and apply_consistent_correction (physics.py:110-147).  The reference passes
 * iterations = 3, damp = 1e-8, atol = btol = 1e-10, iter_lim = 3000 (physics.py:186).
 */
typedef struct {
    int64_t nx, ny, nz;
    double dx, dy, dz;
    const uint8_t *fluid_mask;
    int iterations;          /* outer iterations, >= 0 */
    double damp, atol, btol; /* lsqr arguments */
    int iter_lim;            /* lsqr iteration limit, >= 0 */
} ptv_clean_params;

#define PTV_CLEAN_MAX_OUTER 16 /* outer iterations with per-solve statistics (later ones still run) */
typedef struct {
    int32_t n_outer;   /* solves run */
    int32_t nan_stop;  /* 1: the last solve returned a NaN and ended the loop (physics.py:189-191) */
    int64_t n_fluid;   /* fluid voxels (the order of A) */
    int32_t istop[PTV_CLEAN_MAX_OUTER], itn[PTV_CLEAN_MAX_OUTER]; /* lsqr's istop and itn per solve */
    double rnorm[PTV_CLEAN_MAX_OUTER];          /* lsqr's r2norm per solve */
    double mean_abs_div[PTV_CLEAN_MAX_OUTER];   /* mean |div| over fluid before each solve */
    double ms_iter_median[PTV_CLEAN_MAX_OUTER]; /* median ms per LSQR iteration (over polling batches) */
    double mean_abs_div_final;
    double flux_initial, flux_final; /* sum(u[:, :, nx // 2]) * dy * dz (physics.py:160-165) */
    double ms_total, ms_solve;       /* the call on the device; the LSQR solves alone */
} ptv_clean_stats;

/*
 * Variational divergence cleaning (physics.clean_divergence_variational, physics.py:440-514).
 * Solves (I + lambda_reg D^T D) x = (u, v, w)[fluid] with D = [Dx Dy Dz] of
 * build_divergence_operators (physics.py:356-438) applied matrix-free, by
 * scipy.sparse.linalg.cg(A, b, rtol, atol=0, maxiter).  The reference passes rtol (its `tol`) =
 * 1e-8 and maxiter = 2000 (physics.py:485).  Fields and mask as for ptv_clean_params.
 * PTV_API_VERSION is not raised for these entry points: the presence of ptv_abi_sizes5 in the
 * library is the capability probe.
 */
typedef struct {
    int64_t nx, ny, nz;
    double dx, dy, dz;          /* positive */
    const uint8_t *fluid_mask;
    double lambda_reg;          /* >= 0 (negative: PTV_E_UNSUPPORTED, the system is not positive definite) */
    double rtol;                /* stop when ||r|| < rtol * ||b|| at the top of an iteration */
    int maxiter;                /* >= 0 */
} ptv_variational_params;

typedef struct {
    int64_t n_fluid;  /* fluid voxels (A is 3 n_fluid x 3 n_fluid) */
    int32_t itn;      /* CG iterations completed */
    int32_t info;     /* scipy's: 0 converged, maxiter when the iterations ran out */
    double bnorm, rnorm;  /* ||b||; ||r|| as last summed */
    double mean_abs_div_initial, mean_abs_div_final; /* mean |div| over fluid of the input / the result */
    double ms_total, ms_solve; /* the call on the device; the CG solve alone */
    double ms_iter_median;     /* median ms per CG iteration (over polling batches) */
} ptv_variational_stats;

/*
 * Flow analysis (velocity_analysis.py: compute_strain_rate :10-63, compute_viscous_dissipation
 * :65-92, compute_vorticity :94-120, compute_astarita_flow_type :151-188; the sums feed
 * compute_permeability :122-149 and the report of analyze_flow.py:335-368).  Fields, outputs and
 * the uint8 fluid mask (nonzero = fluid; NULL = nothing is zeroed) are (nz, ny, nx) C order; the
 * slab and halo fields mean exactly what they mean in ptv_div_params.  Outputs have the fields'
 * dtype.  spacing_strong selects numpy's division rule for float32 fields: 0 = Python-float
 * spacings (float32 division by (float)h), 1 = np.float64 spacings (float64 division, the quotient
 * rounded to float32); float64 fields ignore it.  Results are bit-identical to the reference.
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes6 is the capability probe.
 */
#define PTV_FLOW_STRAIN 0
#define PTV_FLOW_DISSIPATION 1
#define PTV_FLOW_VORTICITY 2
#define PTV_FLOW_TYPE 3
typedef struct {
    int64_t nx, ny, nz;
    int64_t z_begin, z_end;
    int edge_lo, edge_hi;
    int field_dtype;      /* PTV_F64 | PTV_F32 */
    int spacing_strong;   /* float32 fields: 0 weak (Python float), 1 strong (np.float64) */
    double dx, dy, dz;    /* positive and finite */
    double viscosity;     /* dissipation = (T)viscosity * S * S */
    const uint8_t *fluid_mask; /* may be NULL */
} ptv_flow_params;

/* Sums are float64 whatever the field dtype and the same bits on every call (fixed order, no
 * atomics).  Indices of the arrays: PTV_FLOW_*; entries of outputs not requested are 0.  max / min
 * propagate NaN as np.max / np.min do.  Outputs are 0 at solid voxels, so sum_fluid[k] (the sum of
 * out[mask]) equals sum[k] bit for bit; both are given because the report divides them by
 * different counts. */
typedef struct {
    int64_t n_voxels, n_fluid;       /* voxels of the computed planes; fluid ones (= n_voxels without a mask) */
    double sum_u, sum_v, sum_w;      /* over the computed planes; the elementwise mode: the sums of its strain
                                      * and vorticity_mag inputs in sum_u and sum_v (0 when not given) */
    double sum[4], sum_fluid[4], max[4], min[4];
    double ms_stencil;               /* the kernels of the call, hipEvent based */
} ptv_flow_stats;

/*
 * Staircase interface drag (velocity_analysis.compute_interface_drag, method='staircase',
 * velocity_analysis.py:332-511) and the gradient sums of compute_permeability_from_pressure
 * (:659-697).  The int32 label mask (0 = fluid, a positive label = a phase), the fields u, v, w and
 * the optional pressure are (nz, ny, nx) C order; the fields share field_dtype.  Along every axis
 * each pair of adjacent voxels (curr, next) is a face of label L in direction A when curr == 0 and
 * next == L, in direction B when curr == L and next == 0; faces between two labels, faces that
 * touch a negative value or a label not in the table, and pairs across an array edge give nothing.
 * Per face, in float64 (float32 fields are widened on load), as the reference writes them:
 *     pressure term  (0.5 * (p[curr] + p[next])) * area in direction A, its negation * area in B
 *     d = (-2.0 * vel[fluid cell]) / step
 *     viscous term   ((viscosity * 2) * d) * area along the face normal, (viscosity * d) * area else
 * with area = dy*dx, dz*dx, dz*dy and step = dz, dy, dx for axes 0 (z), 1 (y), 2 (x).
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes7 is the capability probe.
 */
typedef struct {
    int64_t nx, ny, nz;    /* positive; an axis of length 1 has no faces */
    int field_dtype;       /* PTV_F64 | PTV_F32 */
    int n_labels;          /* >= 1 */
    double dx, dy, dz;     /* positive and finite */
    double viscosity;      /* finite */
    const int32_t *labels; /* n_labels positive labels, strictly ascending; HOST memory in both calls */
} ptv_drag_params;

/* One record per (label, axis, direction): records[(l * 3 + axis) * 2 + dir], dir 0 = A, 1 = B.
 * sum_u, sum_v, sum_w are the sums of the viscous terms of the three velocity components (the one
 * along the axis carries the factor 2); sum_p is 0 without a pressure field.  Sums are float64
 * whatever the field dtype, the same bits on every call and independent of which other labels the
 * table holds alongside (fixed order, no atomics). */
typedef struct {
    int64_t count;                     /* faces */
    double sum_p, sum_u, sum_v, sum_w;
} ptv_drag_stats;

/*
 * Exact Euclidean distance transform of a byte mask and the alignment score that reads it
 * (auto_align.find_best_offset, auto_align.py:10-62).  The mask is uint8 (nz, ny, nx) C order; the
 * meaning is scipy.ndimage.distance_transform_edt's with unit spacing: for every nonzero voxel the
 * distance to the nearest zero voxel, 0 at zero voxels.  d2 is the integer squared distance and the
 * float64 field is sqrt((double)d2), correctly rounded: both equal scipy's bit for bit.  The
 * passes work in uint32, so nz^2 + ny^2 + nx^2 must stay below 2^31 (PTV_E_UNSUPPORTED, decided
 * before any allocation or copy).  A mask without a zero voxel is PTV_E_ARG (scipy measures to a
 * voxel that is not there).
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes8 is the capability probe.
 */
typedef struct {
    int64_t nx, ny, nz;  /* positive */
    int keep_distance;   /* nonzero: the float64 field also stays in the context for ptv_align_score */
} ptv_edt_params;

typedef struct {
    int64_t max_d2;      /* the maximum of d2 over the volume (an integer reduction) */
    double ms;           /* the kernels of the call, hipEvent based */
} ptv_edt_stats;

/*
 * The alignment objective for a batch of offsets.  points: float64 (n_points, 3) as x, y, z; dt: the
 * float64 distance field (nz, ny, nx); offsets: float64 (n_offsets, 3) as dx, dy, dz, HOST memory
 * in both calls.  Per offset o and point p, in the reference's arithmetic: s = p + o in float64,
 * rint(s) (half to even, as np.round: -0.5 gives index 0), the test against [0, nx) x [0, ny) x
 * [0, nz) in floating point, and a point inside adds dt[iz, iy, ix].  Coordinates must be finite
 * (the caller checks).  The reference's value is 1e9 when n_inside == 0, else
 * sum + n_outside * max(dt); the caller forms it.
 */
typedef struct {
    int64_t nx, ny, nz;  /* positive */
    int64_t n_points;    /* 0 <= n_points < 2^31 */
    int n_offsets;       /* >= 1 */
} ptv_align_params;

/* One record per offset.  sum is float64 in a fixed order (no atomics): the same bits on every
 * call, and a batch of m offsets gives the bits of m single calls. */
typedef struct {
    int64_t n_inside, n_outside;
    double sum;
} ptv_align_record;

/*
 * Pressure recovery (velocity_analysis.compute_pressure_field, velocity_analysis.py:190-330, with
 * physics.compute_force_divergence and physics.solve_poisson, physics.py:211-345).  All grids are
 * float64 (nz, ny, nx) C order; the uint8 fluid mask (nonzero = fluid) is required.
 *   force field   f = mu * laplacian_mask_aware(vel) - rho * (vel . grad) vel, at every voxel,
 *                 bit-identical to the reference (the fill's np.roll wrap-around included);
 *   divergence    the face-flux divergence of f at every voxel, bit-identical;
 *   Poisson       with a Dirichlet grid: scipy's cg(A, b, rtol, atol=0, maxiter) on the masked 7-point
 *                 Laplacian whose Dirichlet rows and columns are eliminated (values 0: what the
 *                 reference's matrix computes, bit for bit, from x0 = 0); without one: lsqr on the
 *                 Neumann system with b - mean(b), the solver of ptv_clean_divergence.
 * Both solves agree with the host's normwise, not bit for bit (sums in another order).
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes9 is the capability probe.
 */
#define PTV_WALL_ZERO_NEUMANN 0
#define PTV_WALL_INHOMOGENEOUS 1
#define PTV_ANCHOR_NONE 0
#define PTV_ANCHOR_OUTLET 1
#define PTV_ANCHOR_INLET 2
typedef struct {
    int64_t nx, ny, nz;
    double dx, dy, dz;          /* positive and finite */
    double mu, rho;             /* finite; the advection term is computed for rho > 0 (every extent >= 2) */
    int wall_bc;                /* PTV_WALL_* */
    int anchor;                 /* ptv_pressure_recover: PTV_ANCHOR_* */
    int flow_direction;         /* ptv_pressure_recover: 0 auto (the sign of sum w over fluid), 1 positive, -1 negative */
    int maxiter;                /* CG, >= 0 */
    double rtol;                /* CG: stop when ||r|| < rtol * ||b|| at the top of an iteration */
    double lsqr_damp, lsqr_atol, lsqr_btol; /* the solve without a Dirichlet grid */
    int lsqr_iter_lim;
    const uint8_t *fluid_mask;
} ptv_pressure_params;

typedef struct {
    int64_t n_fluid, n_dirichlet;
    int32_t itn;          /* iterations completed */
    int32_t info;         /* CG: scipy's info (0, or maxiter); LSQR: istop */
    int32_t solver;       /* 0 CG, 1 LSQR */
    int32_t anchor_plane; /* ptv_pressure_recover: the z index of the Dirichlet plane, -1 without one */
    double bnorm, rnorm;  /* ||b||; ||r|| as last summed (LSQR: r2norm) */
    double sum_abs_fx, sum_abs_fy, sum_abs_fz, sum_w; /* over the fluid voxels (fixed order, no atomics) */
    double ms_force, ms_divergence, ms_solve; /* hipEvent based; 0 for a stage the call did not run */
    double ms_iter_median;                    /* CG: median ms per iteration (over polling batches) */
    double ms_total;
} ptv_pressure_stats;

/*
 * Multigrid-preconditioned CG for the anchored Poisson solve (scipy's cg(A, b, M=...), DESIGN.md
 * section 25).  M is one symmetric V-cycle on the active (fluid, not Dirichlet) voxels: levels of
 * ceil(n / 2) cells per axis by piecewise-constant aggregation of 2 x 2 x 2 cells until every extent is
 * at most 2 (or max_levels levels exist), exact Galerkin operators, nu damped-Jacobi sweeps before and
 * after the coarse correction, coarse_sweeps sweeps on the coarsest level.  Every operation is
 * elementwise or a sum of at most eight terms in a stated order, so z = M r is the same bits as the
 * numpy restatement's.  Opt-in: no existing entry point changes.
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes13 is the capability probe.
 */
#define PTV_MG_MAX_LEVELS 32
typedef struct {
    int max_levels;    /* >= 0; 0: as many as the coarsening rule gives */
    int nu;            /* >= 0; 0: 2 sweeps before and 2 after */
    int coarse_sweeps; /* >= 0; 0: 16 */
    double omega;      /* finite, >= 0; 0: 2/3 */
} ptv_mg_params;

typedef struct {
    int32_t levels;     /* levels built, level 0 (the grid) included */
    int32_t tail_level; /* the first level that runs inside the one-workgroup launch */
    int64_t cells[PTV_MG_MAX_LEVELS];  /* per level */
    int64_t active[PTV_MG_MAX_LEVELS]; /* per level: cells with a non-zero diagonal (the cells a sweep moves) */
    double ms_setup;                   /* the coarse operators, hipEvent based */
    double ms_vcycle_median;           /* median ms of the V-cycles timed (one per polling batch; the one of an apply) */
} ptv_mg_stats;

/*
 * Cubic B-spline sampling and the mesh interface drag (scipy.ndimage.spline_filter and
 * map_coordinates with mode='nearest'; velocity_analysis.compute_interface_drag_mesh from the
 * triangulation onward, velocity_analysis.py:547-655).  Fields are (nz, ny, nx) C order.
 *   prefilter     the float64 cubic B-spline coefficients of the field padded by PTV_SPLINE_PAD
 *                 edge-replicated samples on every side, (nz + 24, ny + 24, nx + 24): what scipy
 *                 builds for mode='nearest' (np.pad(..., 12, mode='edge'), then spline_filter(...,
 *                 3, mode='nearest')).  Along axis 0, 1, 2 in turn, on the padded length n, with
 *                 the pole z = sqrt(3) - 2: the line times (1 - z)(1 - 1/z); scipy's reflect start
 *                 c0 += z / (1 - z^2n) * (c0 + z^n c[n-1] + sum_i z^i (c[i] + z^n c[n-1-i])), the
 *                 sum cut after PTV_SPLINE_HORIZON terms (|z|^40 = 1.3e-23); c[i] += z c[i-1];
 *                 c[n-1] *= z / (z - 1); c[i] = z (c[i+1] - c[i]).
 *   sampling      coordinates are (3, n_points) float64 rows z, y, x in index units.
 *                 order 3: at coordinate + 12 in the padded coefficients, clamped to the padded
 *                 extent only, weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 on
 *                 the 4 x 4 x 4 block from floor(x) - 1 (indices clamped to the padded extent).
 *                 order 1: trilinear on the raw field, the coordinate clamped to [0, n - 1].
 *                 order 0: the sample at floor(x + 0.5) clamped to [0, n - 1].
 *                 A NaN coordinate gives NaN (orders 1, 3) or reads index 0 (order 0).
 *   mesh drag     per triangle the reference's terms in its own arithmetic (the centroid and the
 *                 edge differences in the vertices' dtype, everything else float64), summed per
 *                 label in a fixed order (no atomics): the same bits on every call.
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes10 is the capability probe.
 */
#define PTV_SPLINE_PAD 12
#define PTV_SPLINE_HORIZON 40
typedef struct {
    int64_t nx, ny, nz;  /* the raw field, positive */
    int field_dtype;     /* PTV_F64 | PTV_F32 (widened exactly on load) */
    int order;           /* ptv_map_coordinates: 0, 1 or 3 */
    int64_t n_points;    /* ptv_map_coordinates: >= 0 */
} ptv_spline_params;

/* The sums of one label, in the order of the reference's result (velocity_analysis.py:621-643). */
#define PTV_MESH_SUMS 21
typedef struct {
    int64_t nx, ny, nz;         /* the fields, positive */
    int field_dtype;            /* PTV_F64 | PTV_F32: u, v, w and the pressure */
    int vert_dtype;             /* PTV_F64 | PTV_F32: the vertices (skimage's are float32) */
    int64_t n_verts, n_tris;    /* of all labels together; n_tris >= 1 */
    int n_labels;               /* >= 1 */
    double dx, dy, dz;          /* positive and finite */
    double viscosity;           /* finite */
    int reuse;                  /* nonzero: no prefilter, the context holds the coefficients of u, v, w from
                                 * its last mesh drag call (the same nx, ny, nz, PTV_E_ARG otherwise); the
                                 * host-buffer call then also keeps the fields, the pressure and the
                                 * background mask it uploaded last and reads none of those pointers */
    const int64_t *tri_offsets; /* n_labels + 1 ascending, [0] = 0, [n_labels] = n_tris: label l owns
                                 * triangles [tri_offsets[l], tri_offsets[l + 1]); HOST memory in both calls */
    int mesh_resident;          /* nonzero: the mesh is the one the context's last ptv_marching_cubes left on
                                 * the device (PTV_E_ARG if it holds none or one without a triangle): verts,
                                 * faces, vert_dtype, n_verts, n_tris and tri_offsets are not read, n_labels
                                 * must be that call's (PTV_E_ARG otherwise) and one record per label of that
                                 * call is returned (n_tris 0, sums 0 for a label without a surface).  After the
                                 * older members: a caller that zeroes the struct keeps its behaviour */
} ptv_mesh_params;

/* sums: Fx_v Fy_v Fz_v, Fx_v_tan Fy_v_tan Fz_v_tan, Fx_v_nor Fy_v_nor Fz_v_nor, Fx_p Fy_p Fz_p, Area,
 * Fx_water Fy_water Fz_water, Fx_solid Fy_solid Fz_solid, Area_water, Area_solid. */
typedef struct {
    int64_t n_tris;
    double sums[PTV_MESH_SUMS];
} ptv_mesh_record;

/*
 * Marching cubes of a label mask (velocity_analysis.py:547-552 calls skimage.measure.marching_cubes per
 * label): every requested label's indicator mask == label at level 0.5, all labels in one pass over
 * the volume.  skimage's triangle set is NOT reproduced (on a 0/1 indicator its face tests are exact
 * ties, and its tables are not available to this project); the triangulation follows the project's
 * own rule, stated in DESIGN.md section 23 and pinned by tools/make_mc_table.py:
 *   lattice     the voxels whose indices are multiples of step_size; a cube has its origin o at a
 *               lattice point with o + step_size <= n - 1 on every axis.  No padding: a label that
 *               touches the volume's edge has an open surface there.  An axis with n - 1 < step_size
 *               gives no cubes and every count is 0.
 *   vertices    one per lattice edge whose ends differ in the indicator, at its midpoint, float32
 *               [z, y, x] in index units (exact), shared by the triangles that use it; per label in
 *               the order of the owner lattice point (the edge's lower end; z slowest, x fastest), then
 *               axis z, y, x.
 *   triangles   per label by cube in the same linear order, then in the table's order; normals
 *               cross(v1 - v0, v2 - v0) point into the label.  Faces are int32 indices into the label's
 *               own vertices.
 * The output is the same bytes on every call (no atomic assigns a position).  Lattice points must
 * stay below 2^31 - 1, and so must the vertices and the triangles of all labels together
 * (PTV_E_UNSUPPORTED).  The call synchronises twice: after the counting passes (the totals size the
 * buffers, which are allocated then) and at the end (the counts are returned).
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes11 is the capability probe.
 */
typedef struct {
    int64_t nx, ny, nz;    /* the mask, positive */
    int step_size;         /* >= 1 */
    int n_labels;          /* >= 1 */
    const int32_t *labels; /* n_labels ascending, distinct, positive; HOST memory in both calls */
} ptv_surface_params;

/*
 * Connected-component labelling of a byte mask: scipy.ndimage.label for 3-D inputs, bit for bit.  The
 * mask is uint8 (nz, ny, nx) C order, nonzero = foreground.  Two foreground voxels are neighbours when
 * their offset has at most 1, 2 or 3 nonzero components (each +-1): connectivity 6, 18 or 26, scipy's
 * generate_binary_structure(3, 1 / 2 / 3).  labels is int32 of the mask's shape: 0 at background, and
 * the components numbered from 1 in the raster order (z slowest, x fastest) of their first voxels,
 * which is scipy's numbering.  The output is the same bytes on every call.
 * sizes (may be NULL) receives n_components + 1 voxel counts, the background's at index 0, i.e.
 * np.bincount(labels); the count is not known before the call, so the buffer must have room for
 * (nx * ny * nz + 1) / 2 + 1 entries, which no mask exceeds.  The voxel count must stay below 2^31
 * (PTV_E_UNSUPPORTED); a connectivity other than 6, 18, 26, a NULL pointer or a non-positive extent is
 * PTV_E_ARG; all are decided before any device work.  The call synchronises twice: for the component
 * count (it sizes `sizes`) and at the end.
 * PTV_API_VERSION is not raised: the presence of ptv_abi_sizes12 is the capability probe.
 */
typedef struct {
    int64_t nz, ny, nx;  /* positive */
    int connectivity;    /* 6, 18 or 26 */
} ptv_label_params;

typedef struct {
    int64_t n_components;
    int64_t n_foreground; /* nonzero voxels of the mask */
    double ms_merge;      /* tile-local labelling and border merge, hipEvent based */
    double ms_number;     /* flatten, scan and numbering (with the sizes) */
} ptv_label_stats;

/* Library / device management. */
int ptv_version(void);
/* sizeof(ptv_particles, ptv_grid, ptv_knn_params, ptv_stats, ptv_rbf_params, ptv_div_params):
 * binding self-check */
int ptv_abi_sizes(int64_t out6[6]);
/* sizeof(ptv_mask_grid, ptv_boundary_params, ptv_filter_params): the same self-check */
int ptv_abi_sizes2(int64_t out3[3]);
/* sizeof(ptv_linear_params): the same self-check */
int ptv_abi_sizes3(int64_t out1[1]);
/* sizeof(ptv_clean_params, ptv_clean_stats): the same self-check */
int ptv_abi_sizes4(int64_t out2[2]);
/* sizeof(ptv_variational_params, ptv_variational_stats): the same self-check.  A library that has
 * this symbol has the variational entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes5(int64_t out2[2]);
/* sizeof(ptv_flow_params, ptv_flow_stats): the same self-check.  A library that has this symbol has
 * the flow analysis entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes6(int64_t out2[2]);
/* sizeof(ptv_drag_params, ptv_drag_stats): the same self-check.  A library that has this symbol has
 * the interface drag and gradient sums entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes7(int64_t out2[2]);
/* sizeof(ptv_edt_params, ptv_edt_stats, ptv_align_params, ptv_align_record): the same self-check.  A
 * library that has this symbol has the distance transform and alignment score entry points
 * (PTV_API_VERSION stays 11). */
int ptv_abi_sizes8(int64_t out4[4]);
/* sizeof(ptv_pressure_params, ptv_pressure_stats): the same self-check.  A library that has this
 * symbol has the pressure recovery entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes9(int64_t out2[2]);
/* sizeof(ptv_spline_params, ptv_mesh_params, ptv_mesh_record): the same self-check.  A library that
 * has this symbol has the spline sampling and mesh drag entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes10(int64_t out3[3]);
/* sizeof(ptv_surface_params): the same self-check.  A library that has this symbol has the marching
 * cubes entry points and ptv_mesh_params.mesh_resident (PTV_API_VERSION stays 11). */
int ptv_abi_sizes11(int64_t out1[1]);
/* sizeof(ptv_label_params, ptv_label_stats): the same self-check.  A library that has this symbol has
 * the component labelling entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes12(int64_t out2[2]);
/* sizeof(ptv_mg_params, ptv_mg_stats): the same self-check.  A library that has this symbol has the
 * multigrid-preconditioned Poisson entry points (PTV_API_VERSION stays 11). */
int ptv_abi_sizes13(int64_t out2[2]);
const char *ptv_last_error(void);
int ptv_device_count(int *out);
int ptv_init(int device, ptv_ctx **out);
int ptv_free(ptv_ctx *ctx);

/*
 * k-NN IDW / Sibson interpolation, host buffers.
 * Replaces the `method == 'idw'` branch (interpolator.py:126-155) and the
 * `method == 'sibson'` branch (interpolator.py:83-124): KDTree build
 * (:90,:132), query (:97,:139), weights (:102-116,:142-147), gather-sum
 * (:119-122,:150-153), reshape (:124,:155,:199-203).
 * Outputs U, V, W: caller-owned float64 (z_end-z_begin, ny, nx) C order.
 */
int ptv_interp_knn(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                   const ptv_knn_params *prm, double *U, double *V, double *W,
                   ptv_stats *st);

/*
 * Same, every pointer (particles, axes/points, mask, outputs) is DEVICE
 * memory on the ctx's device; work is enqueued on `stream` (hipStream_t,
 * NULL = the ctx's own stream) and the call returns after the enqueue.
 */
int ptv_interp_knn_dev(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                       const ptv_knn_params *prm, double *U, double *V, double *W,
                       void *stream, ptv_stats *st);

/*
 * Local RBF interpolation, host buffers.
 * Replaces the `method == 'rbf'` branch (interpolator.py:157-195) through scipy's
 * RBFInterpolator(neighbors=k) evaluation (_rbfinterp.py:463-556): the KDTree build and
 * query (:345, :513), the sort of each neighbourhood (:521), the per-neighbourhood
 * system build (_build_system) and dgesv solve (:82-127), and the evaluation
 * (_build_evaluation_coefficients @ coeffs, :384-418).  A system with an exactly zero
 * pivot returns PTV_E_SINGULAR (scipy: LinAlgError "Singular matrix.", :115-127);
 * the outputs are then undefined.
 */
int ptv_interp_rbf_local(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                         const ptv_rbf_params *prm, double *U, double *V, double *W,
                         ptv_stats *st);

/* Same on device pointers; enqueued on `stream`, but synchronises once at the end to
 * read the singular-system count (the return code depends on it). */
int ptv_interp_rbf_local_dev(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                             const ptv_rbf_params *prm, double *U, double *V, double *W,
                             void *stream, ptv_stats *st);

/*
 * Linear (Delaunay) interpolation, host buffers.  Replaces the griddata branch for
 * method='linear' (interpolator.py:196-197): LinearNDInterpolator's point location
 * (_find_simplex: bounding-box test, directed walk, brute force) and barycentric
 * interpolation (interpnd _do_evaluate), fill_value outside the hull.  Outputs as
 * ptv_interp_knn (float64).
 */
int ptv_interp_linear(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                      const ptv_linear_params *prm, double *U, double *V, double *W,
                      ptv_stats *st);

/* Same on device pointers (particles, grid, triangulation arrays, mask, outputs); enqueued on
 * `stream`, synchronises once at the end (the brute-force count decides a second kernel). */
int ptv_interp_linear_dev(ptv_ctx *ctx, const ptv_particles *p, const ptv_grid *g,
                          const ptv_linear_params *prm, double *U, double *V, double *W,
                          void *stream, ptv_stats *st);

/*
 * Consistent divergence, host buffers: H2D of the fields and mask, one stencil kernel,
 * D2H of the slab.  Replaces compute_consistent_divergence(u, v, w, mask, dx, dy, dz)
 * (physics.py:6-53; callers view_divergence.py:39,42, physics.py:173,193-194).
 */
int ptv_divergence(ptv_ctx *ctx, const ptv_div_params *prm, const void *U, const void *V,
                   const void *W, void *out, ptv_stats *st);

/* Same on device pointers (fields, mask, out), enqueued on `stream` (NULL = ctx's). */
int ptv_divergence_dev(ptv_ctx *ctx, const ptv_div_params *prm, const void *U, const void *V,
                       const void *W, void *out, void *stream, ptv_stats *st);

/*
 * Nearest-neighbour resampling of a raw mask onto the grid, host buffers.  Replaces
 * sample_mask_on_grid (interpolator.py:205-238): RegularGridInterpolator((z, y, x),
 * mask_raw.astype(float), method='nearest', bounds_error=False, fill_value=0) at every
 * grid voxel, then `> 0.5`.  out: (z_end - z_begin, ny, nx) bytes, 1 = fluid.
 */
int ptv_sample_mask(ptv_ctx *ctx, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out);

/* Same; src->raw, the grid arrays and `out` are DEVICE memory (src axes stay host). */
int ptv_sample_mask_dev(ptv_ctx *ctx, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out,
                        void *stream);

/*
 * Boundary particles, host buffers.  Replaces extract_boundary_particles
 * (interpolator.py:240-284): binary_dilation(mask, 6-connected, iterations=thickness)
 * & ~mask, np.where in C order, [::sampling_step], physical coordinates.
 * *count receives the number of particles; x, y, z (cap entries each) are written only
 * when cap >= *count (call once with cap = 0 to size them).
 */
int ptv_boundary_particles(ptv_ctx *ctx, const ptv_boundary_params *prm, double *x, double *y,
                           double *z, int64_t cap, int64_t *count);

/* Same; prm->mask and x, y, z are DEVICE memory.  Synchronises (the count is returned). */
int ptv_boundary_particles_dev(ptv_ctx *ctx, const ptv_boundary_params *prm, double *x,
                               double *y, double *z, int64_t cap, int64_t *count, void *stream);

/*
 * k-NN outlier filter, host buffers.  Replaces remove_outliers_knn (filtering.py:5-58):
 * KDTree(points).query(points, k+1) minus the point itself (:20-30), the median and MAD
 * of the neighbours' speeds (:38-44) and the z-score test (:47-51).
 * keep: n bytes, 1 = keep (original particle order).  kth_dist: optional (NULL) n
 * doubles, the distance to the (k+1)-th neighbour counting the point itself
 * (`dist[:, -1]`, whose median the reference prints, :33-35).  Requires n > k
 * (the reference skips the filter otherwise, :12-14).
 */
int ptv_filter_outliers_knn(ptv_ctx *ctx, const ptv_particles *p, const ptv_filter_params *prm,
                            uint8_t *keep, double *kth_dist, ptv_stats *st);

/* Same on device pointers, enqueued on `stream` (NULL = the ctx's own stream). */
int ptv_filter_outliers_knn_dev(ptv_ctx *ctx, const ptv_particles *p, const ptv_filter_params *prm,
                                uint8_t *keep, double *kth_dist, void *stream, ptv_stats *st);

/*
 * Divergence cleaning, host buffers: H2D of the fields and mask, the solves on the device, D2H of
 * the cleaned fields Uo, Vo, Wo (float64 (nz, ny, nx); may be U, V, W themselves).  Replaces
 * clean_divergence_projection (physics.py:149-209).  Solid voxels of the outputs are 0 once a
 * correction ran.  A mask without fluid returns PTV_E_ARG.  Results agree with the host solver
 * normwise, not bit for bit (the norms are summed in another order); two calls on the same input
 * agree bit for bit.
 */
int ptv_clean_divergence(ptv_ctx *ctx, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, double *Uo, double *Vo, double *Wo, ptv_clean_stats *st);

/* Same on device pointers (fields, mask, outputs), enqueued on `stream` (NULL = the ctx's own);
 * synchronises (the stop flag of each solve is polled, and the statistics are returned). */
int ptv_clean_divergence_dev(ptv_ctx *ctx, const ptv_clean_params *prm, const double *U, const double *V,
                             const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                             ptv_clean_stats *st);

/*
 * apply_consistent_correction (physics.py:110-147) with phi scattered on the grid (phi_grid,
 * float64 (nz, ny, nx), 0 at solid voxels), host buffers.  Bit-identical to the reference.
 * Only nx, ny, nz, dx, dy, dz and fluid_mask of prm are read.
 */
int ptv_apply_correction(ptv_ctx *ctx, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, const double *phi_grid, double *Uo, double *Vo, double *Wo);

/*
 * y = A x for the masked Laplacian of build_laplacian_matrix (physics.py:55-108), x and y on the
 * grid (float64 (nz, ny, nx); solid entries of x are ignored, of y written as 0), host buffers.
 */
int ptv_laplacian_apply(ptv_ctx *ctx, const ptv_clean_params *prm, const double *x_grid, double *y_grid);

/*
 * Variational divergence cleaning, host buffers: H2D of the fields and mask, the CG solve on the
 * device, D2H of the cleaned fields Uo, Vo, Wo (float64 (nz, ny, nx); may be U, V, W themselves).
 * Replaces clean_divergence_variational (physics.py:440-514).  Solid voxels of the outputs are 0;
 * solid entries of the inputs are never read by the solve.  A mask without fluid, non-positive
 * spacings, a non-finite lambda_reg or rtol return PTV_E_ARG, lambda_reg < 0 PTV_E_UNSUPPORTED; the
 * outputs are not written on any error.  Results agree with the host solver normwise, not bit for
 * bit; two calls on the same input agree bit for bit.
 */
int ptv_clean_variational(ptv_ctx *ctx, const ptv_variational_params *prm, const double *U, const double *V,
                          const double *W, double *Uo, double *Vo, double *Wo, ptv_variational_stats *st);

/* Same on device pointers (fields, mask, outputs), enqueued on `stream` (NULL = the ctx's own);
 * synchronises (the stop flag is polled, and the statistics are returned). */
int ptv_clean_variational_dev(ptv_ctx *ctx, const ptv_variational_params *prm, const double *U, const double *V,
                              const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                              ptv_variational_stats *st);

/*
 * (yu, yv, yw) = A (xu, xv, xw) for A = I + lambda_reg D^T D, every array on the grid (float64
 * (nz, ny, nx); solid entries of x are ignored, of y written as 0), host buffers.  rtol and maxiter
 * of prm are not read.
 */
int ptv_variational_apply(ptv_ctx *ctx, const ptv_variational_params *prm, const double *xu, const double *xv,
                          const double *xw, double *yu, double *yv, double *yw);

/* d = Dx xu + Dy xv + Dz xw of build_divergence_operators (physics.py:356-438), on the grid, host
 * buffers.  lambda_reg, rtol and maxiter of prm are not read. */
int ptv_divergence_operator_apply(ptv_ctx *ctx, const ptv_variational_params *prm, const double *xu,
                                  const double *xv, const double *xw, double *d_grid);

/*
 * Flow analysis, host buffers: H2D of the fields and mask, one stencil pass, D2H of the requested
 * outputs.  strain, dissipation, vorticity, flow_type: (z_end - z_begin, ny, nx) of the fields'
 * dtype, each may be NULL (not computed, not stored).  nx, ny or nz below 2 returns PTV_E_ARG
 * (np.gradient raises ValueError); an empty plane range returns PTV_OK and zero statistics.
 */
int ptv_flow_analysis(ptv_ctx *ctx, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                      void *strain, void *dissipation, void *vorticity, void *flow_type, ptv_flow_stats *st);

/* Same on device pointers (fields, mask, outputs), enqueued on `stream` (NULL = the ctx's own);
 * synchronises (the statistics are returned). */
int ptv_flow_analysis_dev(ptv_ctx *ctx, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                          void *strain, void *dissipation, void *vorticity, void *flow_type, void *stream,
                          ptv_flow_stats *st);

/*
 * Elementwise mode for a caller that holds S (and O) rather than u, v, w: dissipation =
 * (T)viscosity * S * S (compute_viscous_dissipation) and / or flow_type = (S - O) / (S + O) where
 * S + O > (T)1e-15, else 0 (compute_astarita_flow_type), 0 at solid voxels, over all nz * ny * nx
 * voxels; the slab, halo and spacing fields of prm are not read.  vorticity_mag is needed for
 * flow_type only.  The statistics of the outputs and the counts are filled as above.
 */
int ptv_flow_derived(ptv_ctx *ctx, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                     void *dissipation, void *flow_type, ptv_flow_stats *st);

int ptv_flow_derived_dev(ptv_ctx *ctx, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                         void *dissipation, void *flow_type, void *stream, ptv_flow_stats *st);

/*
 * Interface drag, host buffers: H2D of the mask and the fields, one pass over the mask per 32
 * labels, D2H of the records.  P may be NULL (no pressure read, sum_p = 0).  records: n_labels * 6
 * entries, filled in the table's order.  ms (may be NULL) receives the kernels' time, hipEvent
 * based.
 */
int ptv_interface_drag(ptv_ctx *ctx, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
                       const void *W, const void *P, ptv_drag_stats *records, double *ms);

/* Same on device pointers (mask, fields; prm->labels and records stay host memory), enqueued on
 * `stream` (NULL = the ctx's own); synchronises (the records are returned). */
int ptv_interface_drag_dev(ptv_ctx *ctx, const ptv_drag_params *prm, const int32_t *mask, const void *U,
                           const void *V, const void *W, const void *P, void *stream, ptv_drag_stats *records,
                           double *ms);

/*
 * sums3 = the float64 sums over the whole volume of the three components of
 * np.gradient(P, dz, dy, dx), in that order: central differences inside, one-sided at the two ends,
 * each quotient in the field dtype under numpy's division rule (prm->spacing_strong, as for the
 * flow analysis) before it is widened and added, in a fixed order.  Reads nx, ny, nz, field_dtype,
 * spacing_strong and the spacings of prm; the plane range must be the whole buffer.  An axis
 * shorter than 2 returns PTV_E_ARG (np.gradient raises ValueError).  Host buffer.
 */
int ptv_gradient_sums(ptv_ctx *ctx, const ptv_flow_params *prm, const void *P, double sums3[3]);

/* Same on a device pointer, enqueued on `stream` (NULL = the ctx's own); synchronises. */
int ptv_gradient_sums_dev(ptv_ctx *ctx, const ptv_flow_params *prm, const void *P, void *stream, double sums3[3]);

/*
 * Distance transform, host buffers: H2D of the mask, the x pass and two envelope passes, D2H of what
 * was asked for.  d2 (int32, nx * ny * nz) and dist (float64, the same count) may each be NULL.
 * With prm->keep_distance the float64 field is computed in any case and stays in the context, where
 * a later ptv_align_score with dt == NULL reads it.  st may be NULL.
 */
int ptv_edt(ptv_ctx *ctx, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist,
            ptv_edt_stats *st);

/* Same on device pointers, enqueued on `stream` (NULL = the ctx's own); synchronises (the maximum
 * is returned, and decides the no-zero error). */
int ptv_edt_dev(ptv_ctx *ctx, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist,
                void *stream, ptv_edt_stats *st);

/*
 * Alignment score, host buffers.  points and dt are uploaded into the context and stay there: a
 * later call may pass NULL for either to score against what the context holds (the dimensions and
 * the point count must be those of the upload, PTV_E_ARG otherwise), so that an optimiser's calls
 * move only the offsets and the records.  dt == NULL also reads the field a ptv_edt with
 * keep_distance left.  records: n_offsets entries.  ms (may be NULL): the kernels' time.
 */
int ptv_align_score(ptv_ctx *ctx, const ptv_align_params *prm, const double *points, const double *dt,
                    const double *offsets, ptv_align_record *records, double *ms);

/* Same on device pointers (points, dt; offsets and records stay host memory), enqueued on `stream`
 * (NULL = the ctx's own); synchronises (the records are returned). */
int ptv_align_score_dev(ptv_ctx *ctx, const ptv_align_params *prm, const double *points, const double *dt,
                        const double *offsets, void *stream, ptv_align_record *records, double *ms);

/*
 * Force field, host buffers: F = mu * laplacian_mask_aware(U, V, W) - rho * advection, written at
 * every voxel.  st (may be NULL) receives n_fluid, the four sums and ms_force.
 */
int ptv_force_field(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                    double *Fx, double *Fy, double *Fz, ptv_pressure_stats *st);

/* Same on device pointers (prm->fluid_mask too), enqueued on `stream` (NULL = the ctx's own);
 * synchronises (the sums are returned).  The outputs must not alias the inputs. */
int ptv_force_field_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V,
                        const double *W, double *Fx, double *Fy, double *Fz, void *stream, ptv_pressure_stats *st);

/* Force divergence under prm->wall_bc, host buffers; D is written at every voxel (under
 * PTV_WALL_INHOMOGENEOUS solid voxels next to fluid get non-zero values, as in the reference). */
int ptv_force_divergence(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                         const double *Fz, double *D);

/* Same on device pointers, enqueued on `stream`; does not synchronise.  D must not alias F. */
int ptv_force_divergence_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                             const double *Fz, double *D, void *stream);

/*
 * Poisson solve, host buffers.  The right-hand side is rhs, or, when rhs is NULL, the divergence
 * of the force field Fx, Fy, Fz under prm->wall_bc.  dirichlet: a uint8 grid (nonzero = the voxel
 * is fixed to 0; only fluid voxels count) selects CG; NULL selects LSQR on b - mean(b).  X is 0 at
 * solid and Dirichlet voxels.  A NaN in the right-hand side of the CG solve gives NaN at every
 * fluid voxel, info = itn = maxiter (what scipy's recurrence returns).
 */
int ptv_poisson_solve(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                      const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X,
                      ptv_pressure_stats *st);

/* Same on device pointers, enqueued on `stream`; synchronises.  X may alias rhs. */
int ptv_poisson_solve_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                          const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X, void *stream,
                          ptv_pressure_stats *st);

/*
 * The whole chain of compute_pressure_field, resident on the device: one copy in (U, V, W, the
 * mask), the force field, its divergence, the solve, one copy out (P).  The Dirichlet set is the
 * fluid voxels of the plane prm->anchor and prm->flow_direction select (outlet = the last z plane
 * for a positive flow; auto takes the sign of sum w over the fluid voxels, >= 0 is positive);
 * PTV_ANCHOR_NONE runs the LSQR solve.
 */
int ptv_pressure_recover(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V,
                         const double *W, double *P, ptv_pressure_stats *st);

/* Same on device pointers, enqueued on `stream`; synchronises.  P may alias none of the inputs. */
int ptv_pressure_recover_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V,
                             const double *W, double *P, void *stream, ptv_pressure_stats *st);

/*
 * z = M r, host buffers: one V-cycle of the multigrid preconditioner for the mask, the Dirichlet grid
 * (may be NULL: no Dirichlet voxel) and the spacings of prm; mg may be NULL (the defaults).  r is read
 * at active voxels only; z is 0 at every other voxel.  Of prm only nx, ny, nz, dx, dy, dz and
 * fluid_mask are read.  mst (may be NULL) receives the hierarchy, ms_setup and the V-cycle's time.
 */
int ptv_poisson_mg_apply(ptv_ctx *ctx, const ptv_pressure_params *prm, const ptv_mg_params *mg,
                         const uint8_t *dirichlet, const double *r, double *z, ptv_mg_stats *mst);

/* Same on device pointers, enqueued on `stream`; synchronises.  z must not alias r. */
int ptv_poisson_mg_apply_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const ptv_mg_params *mg,
                             const uint8_t *dirichlet, const double *r, double *z, void *stream,
                             ptv_mg_stats *mst);

/*
 * ptv_poisson_solve with scipy's preconditioned recurrence, cg(A, b, M=V-cycle, rtol, atol=0,
 * maxiter): the same right-hand side, outputs, stopping rules and NaN outcome.  The Dirichlet grid is
 * required: NULL (the LSQR branch) returns PTV_E_UNSUPPORTED.  mg may be NULL (the defaults); mst may
 * be NULL.
 */
int ptv_poisson_solve_mg(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                         const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X,
                         const ptv_mg_params *mg, ptv_pressure_stats *st, ptv_mg_stats *mst);

/* Same on device pointers, enqueued on `stream`; synchronises.  X may alias rhs. */
int ptv_poisson_solve_mg_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                             const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X, void *stream,
                             const ptv_mg_params *mg, ptv_pressure_stats *st, ptv_mg_stats *mst);

/*
 * The chain of ptv_pressure_recover with the anchored solve preconditioned.  prm->anchor ==
 * PTV_ANCHOR_NONE (the LSQR solve) returns PTV_E_UNSUPPORTED before anything is written.
 */
int ptv_pressure_recover_mg(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V,
                            const double *W, double *P, const ptv_mg_params *mg, ptv_pressure_stats *st,
                            ptv_mg_stats *mst);

/* Same on device pointers, enqueued on `stream`; synchronises.  P may alias none of the inputs. */
int ptv_pressure_recover_mg_dev(ptv_ctx *ctx, const ptv_pressure_params *prm, const double *U, const double *V,
                                const double *W, double *P, void *stream, const ptv_mg_params *mg,
                                ptv_pressure_stats *st, ptv_mg_stats *mst);

/*
 * Cubic B-spline prefilter, host buffers: H2D of the field, the three passes, D2H of the
 * (nz + 24) * (ny + 24) * (nx + 24) float64 coefficients.  Reads nx, ny, nz and field_dtype of prm.
 * ms (may be NULL) receives the kernels' time, hipEvent based.
 */
int ptv_spline_prefilter(ptv_ctx *ctx, const ptv_spline_params *prm, const void *field, double *coef, double *ms);

/* Same on device pointers, enqueued on `stream` (NULL = the ctx's own); synchronises (for ms).
 * coef must not alias field. */
int ptv_spline_prefilter_dev(ptv_ctx *ctx, const ptv_spline_params *prm, const void *field, double *coef,
                             void *stream, double *ms);

/*
 * out[i] = the order-prm->order sample of the field at (coords[i], coords[n_points + i],
 * coords[2 * n_points + i]) = (z, y, x), host buffers.  Order 3 filters the field into the context's
 * coefficient buffer first; field == NULL samples the coefficients the last order-3 call left there
 * (the same nx, ny, nz, PTV_E_ARG otherwise), so that repeated calls on one field filter it once.
 * Orders 0 and 1 read the raw field.  ms (may be NULL): the kernels' time.
 */
int ptv_map_coordinates(ptv_ctx *ctx, const ptv_spline_params *prm, const void *field, const double *coords,
                        double *out, double *ms);

/* Same on device pointers, enqueued on `stream` (NULL = the ctx's own); synchronises (for ms). */
int ptv_map_coordinates_dev(ptv_ctx *ctx, const ptv_spline_params *prm, const void *field, const double *coords,
                            double *out, void *stream, double *ms);

/*
 * Mesh interface drag, host buffers: H2D of the fields, one prefilter each of U, V, W into the
 * context's coefficient buffers, one launch over all labels' triangles, D2H of one record per
 * label.  P (the pressure, field_dtype) may be NULL (its samples are 0); bg (uint8, nonzero = pore
 * space) may be NULL (every triangle is 'water').  verts: (n_verts, 3) as z, y, x in index units;
 * faces: (n_tris, 3) int32 indices into verts (checked here).  ms2 (may be NULL) receives the
 * prefilters' and the traction kernels' times.
 */
int ptv_mesh_drag(ptv_ctx *ctx, const ptv_mesh_params *prm, const void *U, const void *V, const void *W,
                  const void *P, const uint8_t *bg, const void *verts, const int32_t *faces,
                  ptv_mesh_record *records, double ms2[2]);

/* Same on device pointers (fields, bg, verts, faces; prm->tri_offsets and records stay host memory),
 * enqueued on `stream` (NULL = the ctx's own); synchronises (the records are returned).  A face
 * index outside [0, n_verts) reads the nearest valid vertex. */
int ptv_mesh_drag_dev(ptv_ctx *ctx, const ptv_mesh_params *prm, const void *U, const void *V, const void *W,
                      const void *P, const uint8_t *bg, const void *verts, const int32_t *faces, void *stream,
                      ptv_mesh_record *records, double ms2[2]);

/*
 * Marching cubes, host mask (int32, (nz, ny, nx) C order).  vert_counts / tri_counts (n_labels each,
 * host) receive the vertices and triangles per label; the mesh stays in the context until the next
 * call.  ms2 (may be NULL): the counting passes' (classify, scans) and the emitting passes' (emit,
 * sorts, gathers) times, hipEvent based.
 */
int ptv_marching_cubes(ptv_ctx *ctx, const ptv_surface_params *prm, const int32_t *mask, int64_t *vert_counts,
                       int64_t *tri_counts, double ms2[2]);

/* Same for a mask resident in HBM, enqueued on `stream` (NULL = the ctx's own). */
int ptv_marching_cubes_dev(ptv_ctx *ctx, const ptv_surface_params *prm, const int32_t *mask, void *stream,
                           int64_t *vert_counts, int64_t *tri_counts, double ms2[2]);

/* Copies the context's mesh out: verts (sum of vert_counts, 3) float32 and faces (sum of tri_counts, 3)
 * int32 (host), label after label; a label's faces index its own vertices.  Either may be NULL.
 * PTV_E_ARG when the context holds no mesh. */
int ptv_surface_fetch(ptv_ctx *ctx, float *verts, int32_t *faces);

/*
 * Component labelling, host buffers: H2D of the mask, the four passes, D2H of the labels and, when
 * sizes is not NULL, of its first n_components + 1 entries.  st may be NULL.
 */
int ptv_label(ptv_ctx *ctx, const ptv_label_params *prm, const uint8_t *mask, int32_t *labels, int64_t *sizes,
              ptv_label_stats *st);

/* Same on device pointers (mask, labels, sizes), enqueued on `stream` (NULL = the ctx's own);
 * synchronises (the counts are returned).  The labels stay on the device, where ptv_interface_drag_dev
 * and ptv_marching_cubes_dev take them as their int32 mask. */
int ptv_label_dev(ptv_ctx *ctx, const ptv_label_params *prm, const uint8_t *mask, int32_t *labels, int64_t *sizes,
                  void *stream, ptv_label_stats *st);

/*
 * Last-launch k-NN kernel duration in ms (hipEvent pair recorded around the
 * kernel on the stream it ran on) and the synchronised phase stats.
 */
int ptv_last_stats(ptv_ctx *ctx, ptv_stats *st);

/*
 * Diagnostics: mode 1 = enable + zero per-wave phase stamps of the k-NN kernel (k <= 8
 * launches switch to an s_memtime-stamped build), 0 = disable, other = leave.  If out
 * != NULL (23 doubles) it receives {waves recorded, mean[11], max[11]} over the fields
 * {setup, seeds, rows, copy, compute, epilogue cycles, gathered candidates, merge
 * iterations, rounds, passes, candidates kept by the sub-ball filter}.
 * Profiling only: stamps perturb the schedule; never time a stamped run.
 */
int ptv_debug_stamps(ptv_ctx *ctx, int mode, double *out23);

/*
 * Diagnostics: per-wave XCD records of the stamped launch (ptv_debug_stamps mode 1 first):
 * out receives up to cap records of 3 u64 {XCD the wave ran on, its first and its last value
 * of the device's real-time clock (100 MHz)} in dispatch order (wave = block * 4 + wave of the
 * block); *n_out = records copied.  Waves that wrote nothing have first == last == 0.
 */
int ptv_debug_xcd_stamps(ptv_ctx *ctx, unsigned long long *out, long long cap, long long *n_out);

/*
 * Diagnostics and tests: the chunk length, in blocks, of the map that deals the blocks of a k-NN
 * launch without a dispatch order to the XCDs (chunks of consecutive blocks round-robin; results
 * do not depend on it).  blocks > 0 sets it for every later launch of the process, 0 = one
 * contiguous range per XCD, < 0 = back to the launcher's own choice.
 */
int ptv_debug_xcd_chunk(int blocks);

/*
 * That map on the host: out[lb] = the block that dispatch slot lb runs, lb in [0, nblocks).
 * A bijection of [0, nblocks) for every chunk; slot lb runs on XCD lb % 8.
 */
int ptv_xcd_chunk_map(int nblocks, int chunk, int *out);

#ifdef __cplusplus
}
#endif

#endif /* PTV_API_H */
