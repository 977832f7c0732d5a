// ptv_ctx.hpp — the context behind the C ABI (include/ptv_api.h) and the host layer's interfaces.
//
// One context = one device + one stream + grow-only device buffers reused across calls (the
// reference rebuilds its KDTree on every call, interpolator.py:90/:132; here the binning runs every
// call too, but no allocation does once the buffers are warm).  Every member that holds a HIP
// resource is an owner from ptv_own.hpp: deleting the context frees them all.  DESIGN.md section 16
// says which file of the host layer holds what.
#pragma once

#include <vector>

#include "../../include/ptv_api.h"
#include "ptv_clean.hpp"
#include "ptv_kernels.hpp"
#include "ptv_knn_big.hpp"
#include "ptv_label.hpp"
#include "ptv_mesh.hpp"
#include "ptv_own.hpp"
#include "ptv_pressure.hpp"
#include "ptv_surface.hpp"
#include "ptv_variational.hpp"

namespace ptv {

constexpr int kMaxLattice = 6;
// Slots of the context's staging pool: the largest host call, flow analysis, stages three fields
// and four results.
constexpr int kStageSlots = 7;

// PTV_FLAG_SLAB_CULL_AUTO: the key of the cached cull map, and what the last proven culled call
// under that key kept (the speculative reuse checks both on the device)
struct CullCache {
    std::vector<double> key;       // the map's key: data part (fingerprint, axis values) ++ host part
    std::vector<double> key_host;  // the host part: the arrays, n, the grid, the slab, k, method
    DevBuf<double> key_dev;        // the data part on the device
    bool kept_valid = false;       // a proven culled call ran under this key:
    int64_t kept = 0;              //   its kept count
    double bbox[6] = {0, 0, 0, 0, 0, 0};  //   and bounding box (the same particles give the same)
};

}  // namespace ptv

// Members are destroyed in reverse order: the stream is declared first, so it outlives every
// buffer and event that work enqueued on it may use.
struct ptv_ctx {
    int device = 0;
    ptv::Stream stream;
    ptv::Event ev_knn0, ev_knn1, ev_bin0, ev_bin1, ev_lat1;
    ptv::Event ev_main0, ev_cull0, ev_cull1;  // main-kernel start; slab cull
    bool cull_timed = false;
    bool timed_pending = false;
    ptv::BigScratch big;  // the large-k path (ptv_knn_big.hip)
    ptv::DevBuf<double> pin[6], axes, qpts[3], out[3];
    ptv::DevBuf<double> rbf_huge;  // k_rbf_huge's per-workgroup slices (m > 128)
    ptv::DevBuf<uint8_t> mask;
    ptv::DevBuf<uint32_t> code, perm, count, start, scanp;
    ptv::DevBuf<uint32_t> bin_keys;                                   // sort-based binning: sorted cell codes
    ptv::DevBuf<uint8_t> bin_temp;                                    //   and the radix sort's scratch
    ptv::DevBuf<double4> prec, pval;
    ptv::DevBuf<double> bbox_part, bbox_out;
    ptv::DevBuf<unsigned long long> dbg;
    ptv::DevBuf<double> lat_axes[ptv::kMaxLattice], lat_dk[ptv::kMaxLattice];  // coarse-lattice bound levels
    ptv::DevBuf<float4> lat_recs[ptv::kMaxLattice];                   // their k-NN records (seeds, fp32 relative)
    ptv::DevBuf<int> lat_order[ptv::kMaxLattice];                     // longest-first block order per level
    ptv::DevBuf<double> lat_okeys;                                    // its block keys (scratch)
    ptv::DevBuf<uint32_t> lat_split;                                  // split lattice launch: partial lists
    // PTV_FLAG_SLAB_CULL_AUTO: the cached per-column cull map (top, bot), its key, the proof's
    // need map and scratch
    ptv::DevBuf<double> cmap[2], cdk, ccols, cfp;  // map (top, bot), the lattice bounds it came from, scratch
    ptv::DevBuf<unsigned long long> ckeys;
    ptv::CullMap cmap_geo{};
    int cdk_n[3] = {0, 0, 0};
    bool cmap_valid = false;
    ptv::CullCache ccache;
    ptv::DevBuf<uint32_t> slots;                                      // local RBF: chunk k-NN slots
    ptv::DevBuf<int> rbf_pw, rbf_status;                              // monomial exponents, singular count
    ptv::DevBuf<uint32_t> rbf_nslist;                                 // local RBF: voxels k_rbf_ns hands over
    ptv::DevBuf<int> rbf_cflag;                                       // local RBF: per chunk flagged / overflow
    ptv::DevBuf<double> smooth;                                       // per-particle smoothing (host calls)
    // The one pool of the grid-field host calls (ptv_stage.hpp), slots sized in bytes.  A call
    // stages its host arrays and results here and leaves nothing that a later call reads.
    ptv::DevBuf<uint8_t> stage[ptv::kStageSlots];
    ptv::DevBuf<double> mask_axes;                                    // sample_mask: raw axes (ascending)
    ptv::DevBuf<int> mask_tabs;                                       // sample_mask: per-axis index tables
    ptv::DevBuf<uint8_t> mask_raw, mask_out;                          // sample_mask host calls
    ptv::DevBuf<uint8_t> bnd_ping, bnd_pong;                          // boundary: dilation passes
    ptv::DevBuf<unsigned long long> bnd_counts;                       // boundary: per-block counts / offsets
    ptv::DevBuf<double> bnd_xyz;                                      // boundary host calls: coordinates
    ptv::DevBuf<uint8_t> flt_keep;                                    // outlier filter host calls
    ptv::DevBuf<uint32_t> flt_code, flt_perm, flt_count, flt_start, flt_scanp;  // filter: Morton keys/ids, sort temp
    ptv::DevBuf<double> flt_kth, flt_spd;
    ptv::DevBuf<double> cull[6], cull_win;                            // slab cull: kept particles, z window
    ptv::DevBuf<uint32_t> cull_cnt;                                   // slab cull: per-block counts
    ptv::DevBuf<unsigned long long> cull_mask;                        // slab cull: keep masks (pass 1 -> pass 2)
    ptv::DevBuf<unsigned long long> halo_need;                        // slab cull: proven halo (double bits)
    ptv::DevBuf<unsigned int> rep_cnt;                                // key-list near-tie repair: count
    ptv::DevBuf<uint32_t> rep_list;                                   //   and the listed tiles
    ptv::Event ev_div0, ev_div1;                                      // around the divergence stencil
    bool div_pending = false;
    std::vector<ptv::Event> rbf_ev;                                   // 3 per chunk: knn start, solve start, end
    int rbf_chunks = 0;
    ptv::DevBuf<int> lin_simp, lin_nbr, lin_v2s, lin_count;           // linear: triangulation (host calls), flags
    ptv::DevBuf<double> lin_tr;
    ptv::DevBuf<long long> lin_flags;                                 // linear: voxels left to the brute force
    ptv::CleanWork clean;                                             // divergence cleaning: LSQR vectors, state
    ptv::VarWork var;                                                 // variational cleaning: CG vectors, state
    ptv::PressWork press;                                             // pressure recovery: stencil scratch, CG vectors
    ptv::Event ev_press[4];                                           // chain start, around the divergence, end
    ptv::MgWork mg;                                                   // multigrid preconditioner: operators, coarse vectors
    ptv::DevBuf<double> flow_part, flow_res;                          // flow analysis: per-block partials, reduced rows
    ptv::Event ev_flow0, ev_flow1;                                    // around its kernels
    ptv::DevBuf<double> drag_part, drag_res;                          // interface drag / gradient sums: partials, rows
    ptv::DevBuf<int> drag_labels;                                     // the label table
    ptv::Event ev_drag0, ev_drag1;                                    // around its kernels
    ptv::DevBuf<unsigned> edt_a, edt_b, edt_max;                      // distance transform: pass buffers, max(d2)
    ptv::DevBuf<double> align_dt, align_pts;                          // alignment score: resident field and points
    int64_t align_dt_dims[3] = {0, 0, 0};                             //   what they hold (nx, ny, nz; 0: nothing)
    int64_t align_pts_n = -1;                                         //   (-1: nothing)
    ptv::DevBuf<double> align_off, align_psum;                        // offsets, per-block partial sums
    ptv::DevBuf<int> align_pcnt;                                      //   and inside counts
    ptv::DevBuf<ptv_align_record> align_rec;                          // one record per offset
    ptv::Event ev_edt0, ev_edt1;                                      // around the kernels of either
    ptv::DevBuf<double> spl_coef;                                     // map_coordinates: resident coefficients
    int64_t spl_dims[3] = {0, 0, 0};                                  //   what they hold (nx, ny, nz; 0: nothing)
    ptv::DevBuf<double> mesh_coef[3];                                 // mesh drag: resident coefficients of U, V, W
    int64_t mesh_dims[3] = {0, 0, 0};                                 //   what they hold (nx, ny, nz; 0: nothing)
    ptv::DevBuf<uint8_t> mesh_fld[4], mesh_bg, mesh_verts;            // its host calls: U, V, W, P, mask, vertices,
    int mesh_fld_dtype = -1;                                          //   resident for prm->reuse; what the fields
    bool mesh_has_p = false, mesh_has_bg = false;                     //   are (-1: nothing)
    ptv::DevBuf<int32_t> mesh_faces, mesh_blk_label;                  // faces (host calls); block -> label slot
    ptv::DevBuf<int64_t> mesh_blk_first, mesh_lab_blk0, mesh_off;     // block -> first triangle; per-label tables
    ptv::DevBuf<double> mesh_part, mesh_res;                          // per-block partials, per-label sums
    ptv::Event ev_mesh[3];                                            // prefilter start, traction start, end
    ptv::SurfWork surf;                                               // marching cubes: scratch, the resident mesh
    ptv::Event ev_surf[3];                                            // counting start, emission start, end
    ptv::LabelWork label;                                             // component labelling: forest, flags, ranks
    ptv::Event ev_label[3];                                           // start, after the border merge, end
    ptv::PinnedBuf<double> h_bbox;                                    // pinned, kHostWords doubles
    ptv::PinnedBuf<unsigned long long> h_misc;  // pinned scratch words (cull count, halo bound, repair count)
    ptv_stats last{};
};

namespace ptv {

constexpr size_t kHostWords = 8;  // entries of each pinned block of the context

// The query coordinates of a grid: its three axes (separable), or its three point lists.
struct Queries {
    const double *ax, *ay, *az;  // all NULL unless separable
    const double *qx, *qy, *qz;  // all NULL when separable
    bool separable() const { return ax != nullptr; }
};
inline Queries queries_of(const ptv_grid *g) {
    if (g->ax && g->ay && g->az) return Queries{g->ax, g->ay, g->az, nullptr, nullptr, nullptr};
    return Queries{nullptr, nullptr, nullptr, g->px, g->py, g->pz};
}
// voxels from plane z0 of the grid as queries of the large-k path
inline BigQueries big_queries(const ptv_grid *g, int z0, const uint8_t *mask) {
    const Queries q = queries_of(g);
    BigQueries b;
    b.nx = (int)g->nx;
    b.ny = (int)g->ny;
    b.z0 = z0;
    b.ax = q.ax;
    b.ay = q.ay;
    b.az = q.az;
    b.px = q.qx;
    b.py = q.qy;
    b.pz = q.qz;
    b.mask = mask;
    return b;
}
inline int launch_knn(const KnnLaunch &a, const Binned &b, const Queries &q, const uint8_t *mask, double *U, double *V,
                      double *W, hipStream_t s) {
    return launch_knn(a, b, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, mask, U, V, W, s);
}

// ---- ptv_api.cpp: what the host-buffer calls of every file share ----

// The timings of the last call from its events, into c->last.
int finish_timing(ptv_ctx *c);
// finish_timing, and a host-buffer call's own legs: ev = call start, H2D end, D2H start, call end
int finish_host_timing(ptv_ctx *c, const Event ev[4]);
// The six particle columns -> the context's buffers; dp = the particles on the device.
int upload_particles(ptv_ctx *c, const ptv_particles *p, hipStream_t s, ptv_particles &dp);
// The grid's axes (separable) or point lists -> the context's buffers; dg = the grid on the device.
int upload_grid(ptv_ctx *c, const ptv_grid *g, hipStream_t s, ptv_grid &dg);

// ---- ptv_search.cpp ----

// Search settings shared by the k-NN consumers (IDW/Sibson epilogue, local RBF).
struct SearchParams {
    int method;  // PTV_METHOD_* (k-NN interpolation), ignored by the RBF path
    int k;
    double power, eps;
    uint32_t flags;
    double cell_occupancy, r0_scale;
    int lattice_bounds;
};

// What prepare()'s steps hand to each other and to the caller.
struct Prepared {
    double lo[3], hi[3];  // bounding box of the binned particles and the slab's queries
    CellGrid cg;
    Binned b;
    double r0;            // first gather radius
    CoarseBound cb;       // the finest lattice level (dk == NULL: no lattice was built)
};

// Bounding box, binning, coarse-lattice k-th distance bounds; fills `kl` with a launch template for
// planes [z_begin, z_end) of the grid.  box6 != NULL: the box is known (lo ++ hi, from the slab cull).
int prepare(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const SearchParams *prm, hipStream_t s,
            KnnLaunch &kl, Prepared &pr, const double *box6 = nullptr, bool exact_finest = false);
// Whether prepare() builds the coarse lattice for planes [z_begin, z_end) of a separable grid.
bool lattice_built(const ptv_grid *g, int lattice_bounds);

// The particles a slab cull kept (in the context's cull buffers) and their bounding box with the
// slab's query planes.  ok = false: fewer than k were kept (never provable), bin every particle.
struct Culled {
    bool ok = false;
    ptv_particles p{};
    double box[6];
};
int cull_slab(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, int k, double halo, const CullMap *map,
              const CullCache *spec, size_t nkey, hipStream_t s, Culled &out);

// ---- ptv_run_knn.cpp, ptv_run_chunked.cpp: the per-method runners, all pointers device memory ----
int run_knn(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, const uint8_t *mask,
            double *U, double *V, double *W, hipStream_t s, ptv_stats *st);
int run_filter(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep, double *kth,
               hipStream_t s);
std::vector<int> monomial_powers(int degree);
int run_rbf(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_rbf_params *prm, int m,
            const double *smooth, const uint8_t *mask, double *U, double *V, double *W, hipStream_t s,
            int64_t *n_singular);
int run_linear(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_linear_params *prm,
               const int32_t *simp, const int32_t *nbr, const double *tr, const int32_t *v2s, const uint8_t *mask,
               double *U, double *V, double *W, hipStream_t s);

}  // namespace ptv
