// ptv_mask_api.cpp — the C ABI of the mask and particle-set operations: pore-mask sampling and
// boundary particles (ptv_mask.hip), the k-NN outlier filter (ptv_filter.hip), the distance transform
// and the alignment score (ptv_edt.hip).  Argument validation, the host-buffer calls and the entry
// points on device pointers; the distance field and the points of the alignment score stay resident
// in the context between calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

// raw axes -> device (ascending; a descending axis is reversed and flagged, as scipy's
// RegularGridInterpolator flips descending grids, _rgi.py _check_dimensionality/flip)
int mask_source(ptv_ctx *c, const ptv_mask_grid *src, MaskSampleLaunch &m, hipStream_t s) {
    if (!src || !src->raw || !src->ax || !src->ay || !src->az) {
        set_error("sample_mask: NULL raw mask or axis");
        return PTV_E_ARG;
    }
    const int64_t rn[3] = {src->nx, src->ny, src->nz};
    for (int d = 0; d < 3; ++d)
        if (rn[d] <= 0 || rn[d] > (1 << 30)) {
            set_error("sample_mask: raw mask extents must be positive");
            return PTV_E_ARG;
        }
    std::vector<double> h;
    h.reserve(rn[0] + rn[1] + rn[2]);
    const double *ax[3] = {src->ax, src->ay, src->az};
    size_t off[3];
    for (int d = 0; d < 3; ++d) {
        const double *a = ax[d];
        const int64_t n = rn[d];
        const bool desc = n > 1 && a[0] > a[n - 1];
        off[d] = h.size();
        for (int64_t i = 0; i < n; ++i) h.push_back(desc ? a[n - 1 - i] : a[i]);
        for (int64_t i = 1; i < n; ++i)
            if (!(h[off[d] + i] > h[off[d] + i - 1])) {
                set_error("The points in dimension " + std::to_string(2 - d) +
                          " must be strictly ascending or descending");
                return PTV_E_ARG;
            }
        m.rn[d] = (int)n;
        m.flip[d] = desc ? 1 : 0;
    }
    PTV_TRY(c->mask_axes.ensure(h.size()));
    PTV_HIP(hipMemcpyAsync(c->mask_axes.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
    for (int d = 0; d < 3; ++d) m.ra[d] = c->mask_axes.p + off[d];
    // the host vector must outlive the async copy
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int mask_grid_check(ptv_ctx *c, const ptv_grid *g, uint8_t *out) {
    if (!c) {
        set_error("NULL context");
        return PTV_E_ARG;
    }
    if (!g || !out) {
        set_error("sample_mask: NULL grid or output");
        return PTV_E_ARG;
    }
    if (g->nx <= 0 || g->ny <= 0 || g->nz <= 0 || g->nx > (1 << 30) || g->ny > (1 << 30) || g->nz > (1 << 30)) {
        set_error("grid: dimensions must be positive");
        return PTV_E_ARG;
    }
    const bool sep = g->ax && g->ay && g->az, pts = g->px && g->py && g->pz;
    if (!sep && !pts) {
        set_error("grid: give either the three axes or the three point arrays");
        return PTV_E_ARG;
    }
    if (g->z_begin < 0 || g->z_end > g->nz || g->z_begin > g->z_end) {
        set_error("grid: bad z slab");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int run_mask_sample(ptv_ctx *c, MaskSampleLaunch &m, const ptv_grid *g, const uint8_t *raw, uint8_t *out,
                    hipStream_t s) {
    const Queries q = queries_of(g);
    m.raw = raw;
    m.nx = (int)g->nx;
    m.ny = (int)g->ny;
    m.nz = (int)g->nz;
    m.z0 = (int)g->z_begin;
    m.z1 = (int)g->z_end;
    PTV_TRY(c->mask_tabs.ensure(g->nx + g->ny + g->nz));
    return launch_mask_sample(m, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, c->mask_tabs.p, out, s);
}

int boundary_check(ptv_ctx *c, const ptv_boundary_params *prm, int64_t *count, BoundaryLaunch &m) {
    if (!c || !prm || !prm->mask || !count) {
        set_error("boundary: NULL context, params, mask or count");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30)) {
        set_error("boundary: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->thickness < 1 || prm->sampling_step < 1 ||
        (prm->encoding != PTV_MASK_BOOL && prm->encoding != PTV_MASK_BITS)) {
        set_error("boundary: need thickness >= 1, sampling_step >= 1 and a known encoding");
        return PTV_E_ARG;
    }
    m.nx = (int)prm->nx;
    m.ny = (int)prm->ny;
    m.nz = (int)prm->nz;
    m.mask = prm->mask;
    m.is_bool = prm->encoding == PTV_MASK_BOOL;
    m.thickness = prm->thickness;
    m.step = prm->sampling_step;
    for (int d = 0; d < 3; ++d) {
        m.lo[d] = prm->lo[d];
        m.span[d] = prm->span[d];
        m.den[d] = prm->den[d];
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

// count pass (dilations + block counts + scan), then the emit pass into x, y, z if they fit
int run_boundary(ptv_ctx *c, const BoundaryLaunch &m, double *x, double *y, double *z, int64_t cap, int64_t *count,
                 hipStream_t s) {
    const int64_t nvox = (int64_t)m.nx * m.ny * m.nz;
    const size_t nb = boundary_blocks(nvox);
    PTV_TRY(c->bnd_counts.ensure(nb + 1));
    if (m.thickness > 1) {
        PTV_TRY(c->bnd_ping.ensure(nvox));
        if (m.thickness > 2) PTV_TRY(c->bnd_pong.ensure(nvox));
    }
    const uint8_t *grown = nullptr;
    PTV_TRY(c->ev_div0.record(s));
    PTV_TRY(launch_boundary_count(m, c->bnd_ping.p, c->bnd_pong.p, c->bnd_counts.p, &grown, s));
    unsigned long long total = 0;
    PTV_HIP(hipMemcpyAsync(&total, c->bnd_counts.p + nb, sizeof(total), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    const int64_t nsel = (int64_t)((total + (unsigned long long)m.step - 1) / (unsigned long long)m.step);
    *count = nsel;
    if (x && y && z && cap >= nsel && nsel > 0)
        PTV_TRY(launch_boundary_emit(m, grown, c->bnd_counts.p, x, y, z, s));
    PTV_TRY(c->ev_div1.record(s));
    c->div_pending = true;
    return PTV_OK;
}

int filter_check(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep) {
    if (!c || !p || !prm || !keep) {
        set_error("filter: NULL context, particles, params or keep");
        return PTV_E_ARG;
    }
    if (p->n <= 0 || !p->x || !p->y || !p->z || !p->u || !p->v || !p->w) {
        set_error("particles: need n > 0 and six non-NULL arrays");
        return PTV_E_ARG;
    }
    if (p->n >= (int64_t)1 << 31) {
        set_error("particles: n must be < 2^31");
        return PTV_E_ARG;
    }
    if (prm->k < 1) {
        set_error("filter: k must be >= 1");
        return PTV_E_ARG;
    }
    if (p->n <= prm->k) {
        set_error("filter: need more particles than k (the reference skips the filter)");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

// ---- distance transform and alignment score (ptv_edt.hip) ----
// the dimensions a uint32 squared distance can hold; decided before any allocation or copy
int edt_dims(int64_t nx, int64_t ny, int64_t nz, const char *what) {
    if (nx < 1 || ny < 1 || nz < 1) {
        set_error(std::string(what) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    const int64_t most = 46340;  // floor(sqrt(2^31 - 1)): keeps the squares below from overflowing
    if (nx > most || ny > most || nz > most || nx * nx + ny * ny + nz * nz >= ((int64_t)1 << 31)) {
        set_error(std::string(what) + ": nz^2 + ny^2 + nx^2 must be below 2^31 (squared distances are 32-bit)");
        return PTV_E_UNSUPPORTED;
    }
    return PTV_OK;
}

int edt_args(ptv_ctx *c, const ptv_edt_params *prm, const uint8_t *mask) {
    if (!c || !prm || !mask) {
        set_error("distance transform: NULL context, params or mask");
        return PTV_E_ARG;
    }
    PTV_TRY(edt_dims(prm->nx, prm->ny, prm->nz, "distance transform"));
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int align_check(ptv_ctx *c, const ptv_align_params *prm, const double *offsets, ptv_align_record *records) {
    if (!c || !prm || !offsets || !records) {
        set_error("alignment score: NULL context, params, offsets or records");
        return PTV_E_ARG;
    }
    PTV_TRY(edt_dims(prm->nx, prm->ny, prm->nz, "alignment score"));
    if (prm->n_points < 0 || prm->n_points >= ((int64_t)1 << 31)) {
        set_error("alignment score: 0 <= n_points < 2^31");
        return PTV_E_ARG;
    }
    if (prm->n_offsets < 1) {
        set_error("alignment score: at least one offset");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_sample_mask_dev(ptv_ctx *c, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out, void *stream) {
    PTV_TRY(mask_grid_check(c, g, out));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    MaskSampleLaunch m{};
    PTV_TRY(mask_source(c, src, m, s));
    return run_mask_sample(c, m, g, src->raw, out, s);
}

int ptv_sample_mask(ptv_ctx *c, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out) {
    PTV_TRY(mask_grid_check(c, g, out));
    hipStream_t s = c->stream;
    MaskSampleLaunch m{};
    PTV_TRY(mask_source(c, src, m, s));
    const int64_t nraw = src->nx * src->ny * src->nz;
    PTV_TRY(c->mask_raw.ensure(nraw));
    PTV_HIP(hipMemcpyAsync(c->mask_raw.p, src->raw, nraw, hipMemcpyHostToDevice, s));
    ptv_grid dg;
    PTV_TRY(upload_grid(c, g, s, dg));
    const int64_t nout = (g->z_end - g->z_begin) * g->nx * g->ny;
    PTV_TRY(c->mask_out.ensure(nout));
    PTV_TRY(run_mask_sample(c, m, &dg, c->mask_raw.p, c->mask_out.p, s));
    PTV_HIP(hipMemcpyAsync(out, c->mask_out.p, nout, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_boundary_particles_dev(ptv_ctx *c, const ptv_boundary_params *prm, double *x, double *y, double *z,
                               int64_t cap, int64_t *count, void *stream) {
    BoundaryLaunch m{};
    PTV_TRY(boundary_check(c, prm, count, m));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_boundary(c, m, x, y, z, cap, count, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_boundary_particles(ptv_ctx *c, const ptv_boundary_params *prm, double *x, double *y, double *z, int64_t cap,
                           int64_t *count) {
    BoundaryLaunch m{};
    PTV_TRY(boundary_check(c, prm, count, m));
    hipStream_t s = c->stream;
    const int64_t nvox = prm->nx * prm->ny * prm->nz;
    PTV_TRY(c->mask_raw.ensure(nvox));
    PTV_HIP(hipMemcpyAsync(c->mask_raw.p, prm->mask, nvox, hipMemcpyHostToDevice, s));
    m.mask = c->mask_raw.p;
    // size the device output from the count pass when the caller's buffers are large enough
    int64_t nsel = 0;
    PTV_TRY(run_boundary(c, m, nullptr, nullptr, nullptr, 0, &nsel, s));
    *count = nsel;
    if (x && y && z && cap >= nsel && nsel > 0) {
        PTV_TRY(c->bnd_xyz.ensure((size_t)3 * nsel));
        double *d = c->bnd_xyz.p;
        PTV_TRY(run_boundary(c, m, d, d + nsel, d + 2 * nsel, nsel, &nsel, s));
        PTV_HIP(hipMemcpyAsync(x, d, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipMemcpyAsync(y, d + nsel, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipMemcpyAsync(z, d + 2 * nsel, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_filter_outliers_knn_dev(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep,
                                double *kth_dist, void *stream, ptv_stats *st) {
    PTV_TRY(filter_check(c, p, prm, keep));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_filter(c, p, prm, keep, kth_dist, s));
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_filter_outliers_knn(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep,
                            double *kth_dist, ptv_stats *st) {
    PTV_TRY(filter_check(c, p, prm, keep));
    hipStream_t s = c->stream;
    const int64_t n = p->n;
    ptv_particles dp;
    PTV_TRY(upload_particles(c, p, s, dp));
    PTV_TRY(c->flt_keep.ensure(n));
    PTV_TRY(c->flt_kth.ensure(n));
    PTV_TRY(run_filter(c, &dp, prm, c->flt_keep.p, c->flt_kth.p, s));
    PTV_HIP(hipMemcpyAsync(keep, c->flt_keep.p, n, hipMemcpyDeviceToHost, s));
    if (kth_dist) PTV_HIP(hipMemcpyAsync(kth_dist, c->flt_kth.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    PTV_TRY(finish_timing(c));
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_edt_dev(ptv_ctx *c, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist, void *stream,
                ptv_edt_stats *st) {
    PTV_TRY(edt_args(c, prm, mask));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_TRY(c->edt_a.ensure(n));
    PTV_TRY(c->edt_b.ensure(n));
    PTV_TRY(c->edt_max.ensure(1));
    double *kept = nullptr;
    if (prm->keep_distance) {
        c->align_dt_dims[0] = 0;  // nothing valid until this call has succeeded
        PTV_TRY(c->align_dt.ensure(n));
        kept = c->align_dt.p;
    }
    PTV_TRY(c->ev_edt0.record(s));
    // with both a caller's field and a kept one, the kernel writes the kept one and a copy follows
    PTV_TRY(launch_edt((int)prm->nx, (int)prm->ny, (int)prm->nz, mask, c->edt_a.p, c->edt_b.p, d2, kept ? kept : dist,
                       c->edt_max.p, s));
    if (kept && dist) PTV_HIP(hipMemcpyAsync(dist, kept, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    PTV_TRY(c->ev_edt1.record(s));
    unsigned top = 0;
    PTV_HIP(hipMemcpyAsync(&top, c->edt_max.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (top >= 0x80000000u) {
        set_error("distance transform: the mask has no zero voxel");
        return PTV_E_ARG;
    }
    if (kept) {
        c->align_dt_dims[0] = prm->nx;
        c->align_dt_dims[1] = prm->ny;
        c->align_dt_dims[2] = prm->nz;
    }
    if (st) {
        float t = 0.f;
        PTV_HIP(hipEventElapsedTime(&t, c->ev_edt0, c->ev_edt1));
        st->max_d2 = (int64_t)top;
        st->ms = t;
    }
    return PTV_OK;
}

int ptv_edt(ptv_ctx *c, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist, ptv_edt_stats *st) {
    PTV_TRY(edt_args(c, prm, mask));
    Stage sg(c);
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    const uint8_t *dM = sg.in<uint8_t>(0, mask, n);
    int32_t *dd2 = d2 ? sg.room<int32_t>(1, n * sizeof(int32_t)) : nullptr;
    PTV_TRY(sg.rc);
    // the float64 field of a host call lives in the context's resident buffer, kept or not
    ptv_edt_params q = *prm;
    const bool kept = prm->keep_distance != 0;
    if (dist) q.keep_distance = 1;
    const int rc = ptv_edt_dev(c, &q, dM, dd2, nullptr, sg.s, st);
    if (!kept) c->align_dt_dims[0] = 0;
    PTV_TRY(rc);
    if (d2) sg.back(d2, 1, n * sizeof(int32_t));
    if (dist) PTV_HIP(hipMemcpyAsync(dist, c->align_dt.p, n * sizeof(double), hipMemcpyDeviceToHost, sg.s));
    return sg.sync();
}

int ptv_align_score_dev(ptv_ctx *c, const ptv_align_params *prm, const double *points, const double *dt,
                        const double *offsets, void *stream, ptv_align_record *records, double *ms) {
    PTV_TRY(align_check(c, prm, offsets, records));
    if (!dt || (!points && prm->n_points > 0)) {
        set_error("alignment score: NULL points or distance field");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    AlignArgs a{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.n = prm->n_points;
    align_tile(a);
    const int chunk = 4096;  // offsets per launch (a grid's y extent is 16-bit)
    const int m = prm->n_offsets, mc = std::min(m, chunk);
    PTV_TRY(c->align_off.ensure((size_t)m * 3));
    PTV_TRY(c->align_rec.ensure((size_t)m));
    PTV_TRY(c->align_psum.ensure((size_t)mc * a.nblocks));
    PTV_TRY(c->align_pcnt.ensure((size_t)mc * a.nblocks));
    PTV_HIP(hipMemcpyAsync(c->align_off.p, offsets, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    PTV_TRY(c->ev_edt0.record(s));
    for (int o0 = 0; o0 < m; o0 += chunk)
        PTV_TRY(launch_align_score(a, points, dt, c->align_off.p + (size_t)o0 * 3, std::min(chunk, m - o0),
                                   c->align_psum.p, c->align_pcnt.p, c->align_rec.p + o0, s));
    PTV_TRY(c->ev_edt1.record(s));
    PTV_HIP(hipMemcpyAsync(records, c->align_rec.p, (size_t)m * sizeof(ptv_align_record), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (ms) {
        float t = 0.f;
        PTV_HIP(hipEventElapsedTime(&t, c->ev_edt0, c->ev_edt1));
        *ms = t;
    }
    return PTV_OK;
}

int ptv_align_score(ptv_ctx *c, const ptv_align_params *prm, const double *points, const double *dt,
                    const double *offsets, ptv_align_record *records, double *ms) {
    PTV_TRY(align_check(c, prm, offsets, records));
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (dt) {
        const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
        c->align_dt_dims[0] = 0;
        PTV_TRY(c->align_dt.ensure(n));
        PTV_HIP(hipMemcpyAsync(c->align_dt.p, dt, n * sizeof(double), hipMemcpyHostToDevice, s));
        c->align_dt_dims[0] = prm->nx;
        c->align_dt_dims[1] = prm->ny;
        c->align_dt_dims[2] = prm->nz;
    } else if (c->align_dt_dims[0] != prm->nx || c->align_dt_dims[1] != prm->ny || c->align_dt_dims[2] != prm->nz) {
        set_error("alignment score: dt is NULL and the context holds no distance field of these dimensions");
        return PTV_E_ARG;
    }
    if (points) {
        c->align_pts_n = -1;
        PTV_TRY(c->align_pts.ensure((size_t)prm->n_points * 3));
        PTV_HIP(hipMemcpyAsync(c->align_pts.p, points, (size_t)prm->n_points * 3 * sizeof(double),
                               hipMemcpyHostToDevice, s));
        c->align_pts_n = prm->n_points;
    } else if (c->align_pts_n != prm->n_points) {
        set_error("alignment score: points is NULL and the context holds no point set of this size");
        return PTV_E_ARG;
    }
    PTV_TRY(c->align_pts.ensure(1));  // zero points: still a pointer
    return ptv_align_score_dev(c, prm, c->align_pts.p, c->align_dt.p, offsets, s, records, ms);
}

}  // extern "C"
