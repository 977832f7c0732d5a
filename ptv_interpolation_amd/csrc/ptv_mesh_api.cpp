// ptv_mesh_api.cpp — the C ABI of the spline sampling and the mesh interface drag (ptv_mesh.hip):
// argument validation, the host-buffer calls and the entry points on device pointers.  The context
// keeps the coefficient buffers: an order-3 ptv_map_coordinates with field == NULL and a
// ptv_mesh_drag with prm->reuse sample what the previous call filtered.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

int spline_dims(int64_t nx, int64_t ny, int64_t nz, const char *what, SplineDims &d) {
    const int64_t most = 1 << 30;
    if (nx < 1 || ny < 1 || nz < 1) {
        set_error(std::string(what) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    if (nx > most || ny > most || nz > most || (double)(nx + 24) * (double)(ny + 24) * (double)(nz + 24) >= 1099511627776.0) {
        set_error(std::string(what) + ": fewer than 2^40 padded voxels, at most 2^30 per axis");
        return PTV_E_ARG;
    }
    d = SplineDims{(int)nx, (int)ny, (int)nz};
    return PTV_OK;
}

int spline_args(ptv_ctx *c, const ptv_spline_params *prm, const char *what, SplineDims &d) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error(std::string(what) + ": field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    PTV_TRY(spline_dims(prm->nx, prm->ny, prm->nz, what, d));
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

bool same_dims(const int64_t have[3], const SplineDims &d) {
    return have[0] == d.nx && have[1] == d.ny && have[2] == d.nz;
}
void set_dims(int64_t have[3], const SplineDims &d) {
    have[0] = d.nx;
    have[1] = d.ny;
    have[2] = d.nz;
}

int elapsed(const Event &e0, const Event &e1, double *ms) {
    float t = 0.f;
    PTV_HIP(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t;
    return PTV_OK;
}

int prefilter_args(ptv_ctx *c, const ptv_spline_params *prm, const void *field, const double *coef, SplineDims &d) {
    PTV_TRY(spline_args(c, prm, "spline prefilter", d));
    if (!field || !coef) {
        set_error("spline prefilter: NULL field or coefficients");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// what the host and the device call of map_coordinates check alike, before anything is copied
int map_args(ptv_ctx *c, const ptv_spline_params *prm, const double *coords, const double *out, SplineDims &d,
             bool device) {
    PTV_TRY(spline_args(c, prm, "map_coordinates", d));
    if (device && prm->order != 0 && prm->order != 1 && prm->order != 3) {
        set_error("map_coordinates: order must be 0, 1 or 3");
        return PTV_E_UNSUPPORTED;
    }
    if (prm->n_points < 0 || (prm->n_points > 0 && (!coords || !out))) {
        set_error("map_coordinates: n_points >= 0 with their coordinates and output");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int mesh_args(ptv_ctx *c, const ptv_mesh_params *prm, MeshArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    for (int dt : {prm->field_dtype, prm->vert_dtype})
        if (dt != PTV_F64 && dt != PTV_F32) {
            set_error("mesh drag: field_dtype and vert_dtype must be PTV_F64 or PTV_F32");
            return PTV_E_ARG;
        }
    a = MeshArgs{};
    PTV_TRY(spline_dims(prm->nx, prm->ny, prm->nz, "mesh drag", a.d));
    for (double h : {prm->dx, prm->dy, prm->dz})
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("mesh drag: spacings must be positive and finite");
            return PTV_E_ARG;
        }
    if (!std::isfinite(prm->viscosity)) {
        set_error("mesh drag: viscosity must be finite");
        return PTV_E_ARG;
    }
    if (prm->n_labels < 1 || prm->n_labels > 65535 * 32 || !prm->tri_offsets) {
        set_error("mesh drag: at least one label (at most 2097120) and their triangle offsets");
        return PTV_E_ARG;
    }
    if (prm->n_tris < 1 || prm->n_verts < 1 || prm->n_verts >= ((int64_t)1 << 31) ||
        prm->n_tris >= ((int64_t)1 << 38)) {
        set_error("mesh drag: at least one triangle and vertex, fewer than 2^31 vertices and 2^38 triangles");
        return PTV_E_ARG;
    }
    if (prm->tri_offsets[0] != 0 || prm->tri_offsets[prm->n_labels] != prm->n_tris) {
        set_error("mesh drag: tri_offsets must run from 0 to n_tris");
        return PTV_E_ARG;
    }
    for (int l = 0; l < prm->n_labels; ++l)
        if (prm->tri_offsets[l + 1] < prm->tri_offsets[l]) {
            set_error("mesh drag: tri_offsets must ascend");
            return PTV_E_ARG;
        }
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.vert_f32 = prm->vert_dtype == PTV_F32;
    a.n_verts = prm->n_verts;
    a.n_tris = prm->n_tris;
    a.n_labels = prm->n_labels;
    a.h[0] = prm->dz;
    a.h[1] = prm->dy;
    a.h[2] = prm->dx;
    a.viscosity = prm->viscosity;
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

// prm->mesh_resident: the parameters with the mesh that the context's last marching cubes left on
// the device in place of the caller's
int resident_mesh(ptv_ctx *c, const ptv_mesh_params *prm, ptv_mesh_params &out) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    out = *prm;
    if (!prm->mesh_resident) return PTV_OK;
    const SurfWork &w = c->surf;
    if (w.n_labels < 1 || w.tstart[w.n_labels] < 1) {
        set_error("mesh drag: mesh_resident, but the context holds no mesh with a triangle");
        return PTV_E_ARG;
    }
    if (prm->n_labels != w.n_labels) {  // the caller's records have room for n_labels
        set_error("mesh drag: mesh_resident, but n_labels is not the label count of the context's mesh");
        return PTV_E_ARG;
    }
    out.vert_dtype = PTV_F32;
    out.n_verts = w.vstart[w.n_labels];
    out.n_tris = w.tstart[w.n_labels];
    out.n_labels = w.n_labels;
    out.tri_offsets = w.tstart.data();
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_spline_prefilter_dev(ptv_ctx *c, const ptv_spline_params *prm, const void *field, double *coef, void *stream,
                             double *ms) {
    SplineDims d{};
    PTV_TRY(prefilter_args(c, prm, field, coef, d));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(c->ev_mesh[0].record(s));
    PTV_TRY(launch_spline_prefilter(d, field, prm->field_dtype == PTV_F32, coef, s));
    PTV_TRY(c->ev_mesh[1].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    return elapsed(c->ev_mesh[0], c->ev_mesh[1], ms);
}

int ptv_spline_prefilter(ptv_ctx *c, const ptv_spline_params *prm, const void *field, double *coef, double *ms) {
    SplineDims d{};
    PTV_TRY(prefilter_args(c, prm, field, coef, d));
    Stage sg(c);
    const size_t bytes = (size_t)d.nx * d.ny * d.nz * (prm->field_dtype == PTV_F32 ? 4 : 8);
    const void *dF = sg.in(0, field, bytes);
    double *dC = sg.room<double>(1, d.padded() * sizeof(double));
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_spline_prefilter_dev(c, prm, dF, dC, sg.s, ms));
    PTV_HIP(hipMemcpy(coef, dC, d.padded() * sizeof(double), hipMemcpyDeviceToHost));  // synchronised by the device call
    return PTV_OK;
}

int ptv_map_coordinates_dev(ptv_ctx *c, const ptv_spline_params *prm, const void *field, const double *coords,
                            double *out, void *stream, double *ms) {
    SplineDims d{};
    PTV_TRY(map_args(c, prm, coords, out, d, true));
    if (!field && prm->order != 3) {
        set_error("map_coordinates: orders 0 and 1 read the field (NULL)");
        return PTV_E_ARG;
    }
    if (!field && !same_dims(c->spl_dims, d)) {
        set_error("map_coordinates: the context holds no coefficients of these dimensions");
        return PTV_E_ARG;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const bool f32 = prm->field_dtype == PTV_F32;
    const void *src = field;
    if (prm->order == 3 && field) {
        set_dims(c->spl_dims, SplineDims{0, 0, 0});  // nothing valid until the filter is enqueued
        PTV_TRY(c->spl_coef.ensure(d.padded()));
    }
    PTV_TRY(c->ev_mesh[0].record(s));
    if (prm->order == 3) {
        if (field) {
            PTV_TRY(launch_spline_prefilter(d, field, f32, c->spl_coef.p, s));
            set_dims(c->spl_dims, d);
        }
        src = c->spl_coef.p;
    }
    PTV_TRY(launch_map_coordinates(d, prm->order, src, f32, coords, prm->n_points, out, s));
    PTV_TRY(c->ev_mesh[1].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    return elapsed(c->ev_mesh[0], c->ev_mesh[1], ms);
}

int ptv_map_coordinates(ptv_ctx *c, const ptv_spline_params *prm, const void *field, const double *coords, double *out,
                        double *ms) {
    SplineDims d{};
    PTV_TRY(map_args(c, prm, coords, out, d, false));  // the order is checked after the upload
    Stage sg(c);
    const size_t n = (size_t)prm->n_points;
    const size_t bytes = (size_t)d.nx * d.ny * d.nz * (prm->field_dtype == PTV_F32 ? 4 : 8);
    const void *dF = field ? sg.in(0, field, bytes) : nullptr;
    const double *dX = n ? sg.in<double>(1, coords, 3 * n * sizeof(double)) : sg.room<double>(1, 0);
    double *dO = sg.room<double>(2, n * sizeof(double));
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_map_coordinates_dev(c, prm, dF, dX, dO, sg.s, ms));
    if (n) PTV_HIP(hipMemcpy(out, dO, n * sizeof(double), hipMemcpyDeviceToHost));  // synchronised by the device call
    return PTV_OK;
}

int ptv_mesh_drag_dev(ptv_ctx *c, const ptv_mesh_params *given, const void *U, const void *V, const void *W,
                      const void *P, const uint8_t *bg, const void *verts, const int32_t *faces, void *stream,
                      ptv_mesh_record *records, double ms2[2]) {
    ptv_mesh_params resolved;
    PTV_TRY(resident_mesh(c, given, resolved));
    const ptv_mesh_params *prm = &resolved;
    if (prm->mesh_resident) {
        verts = c->surf.verts.p;
        faces = c->surf.faces.p;
    }
    MeshArgs a{};
    PTV_TRY(mesh_args(c, prm, a));
    if (!U || !V || !W || !verts || !faces || !records) {
        set_error("mesh drag: NULL field, vertices, faces or records");
        return PTV_E_ARG;
    }
    if (prm->reuse && !same_dims(c->mesh_dims, a.d)) {
        set_error("mesh drag: reuse, but the context holds no coefficients of these dimensions");
        return PTV_E_ARG;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int nl = prm->n_labels;
    // the block -> (label, first triangle) table: a block never spans two labels
    const int64_t nblocks = mesh_blocks(prm->tri_offsets, nl);
    std::vector<int32_t> blk_label((size_t)nblocks);
    std::vector<int64_t> blk_first((size_t)nblocks), lab_blk0((size_t)nl + 1);
    int64_t b = 0;
    for (int l = 0; l < nl; ++l) {
        lab_blk0[l] = b;
        for (int64_t t = prm->tri_offsets[l]; t < prm->tri_offsets[l + 1]; t += kMeshThreads, ++b) {
            blk_label[b] = l;
            blk_first[b] = t;
        }
    }
    lab_blk0[nl] = b;
    PTV_TRY(c->mesh_blk_label.ensure((size_t)nblocks));
    PTV_TRY(c->mesh_blk_first.ensure((size_t)nblocks));
    PTV_TRY(c->mesh_lab_blk0.ensure((size_t)nl + 1));
    PTV_TRY(c->mesh_off.ensure((size_t)nl + 1));
    PTV_TRY(c->mesh_part.ensure((size_t)nblocks * kMeshSums));
    PTV_TRY(c->mesh_res.ensure((size_t)nl * kMeshSums));
    if (!prm->reuse) {
        set_dims(c->mesh_dims, SplineDims{0, 0, 0});
        for (int k = 0; k < 3; ++k) PTV_TRY(c->mesh_coef[k].ensure(a.d.padded()));
    }
    PTV_HIP(hipMemcpyAsync(c->mesh_blk_label.p, blk_label.data(), (size_t)nblocks * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
    PTV_HIP(hipMemcpyAsync(c->mesh_blk_first.p, blk_first.data(), (size_t)nblocks * sizeof(int64_t),
                           hipMemcpyHostToDevice, s));
    PTV_HIP(hipMemcpyAsync(c->mesh_lab_blk0.p, lab_blk0.data(), ((size_t)nl + 1) * sizeof(int64_t),
                           hipMemcpyHostToDevice, s));
    PTV_HIP(hipMemcpyAsync(c->mesh_off.p, prm->tri_offsets, ((size_t)nl + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                           s));
    PTV_TRY(c->ev_mesh[0].record(s));
    if (!prm->reuse) {
        const void *f[3] = {U, V, W};
        for (int k = 0; k < 3; ++k) PTV_TRY(launch_spline_prefilter(a.d, f[k], a.field_f32, c->mesh_coef[k].p, s));
        set_dims(c->mesh_dims, a.d);
    }
    PTV_TRY(c->ev_mesh[1].record(s));
    const double *coef[3] = {c->mesh_coef[0].p, c->mesh_coef[1].p, c->mesh_coef[2].p};
    PTV_TRY(launch_mesh_drag(a, U, V, W, P, bg, coef, verts, faces, c->mesh_off.p, c->mesh_blk_label.p,
                             c->mesh_blk_first.p, c->mesh_lab_blk0.p, nblocks, c->mesh_part.p, c->mesh_res.p, s));
    PTV_TRY(c->ev_mesh[2].record(s));
    std::vector<double> h((size_t)nl * kMeshSums);
    PTV_HIP(hipMemcpyAsync(h.data(), c->mesh_res.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));  // the pageable staging vectors above are read by now
    PTV_TRY(elapsed(c->ev_mesh[0], c->ev_mesh[1], ms2 ? ms2 + 0 : nullptr));
    if (ms2 && prm->reuse) ms2[0] = 0.0;  // nothing was filtered
    PTV_TRY(elapsed(c->ev_mesh[1], c->ev_mesh[2], ms2 ? ms2 + 1 : nullptr));
    for (int l = 0; l < nl; ++l) {
        records[l].n_tris = prm->tri_offsets[l + 1] - prm->tri_offsets[l];
        for (int k = 0; k < kMeshSums; ++k) records[l].sums[k] = h[(size_t)l * kMeshSums + k];
    }
    return PTV_OK;
}

int ptv_mesh_drag(ptv_ctx *c, const ptv_mesh_params *given, const void *U, const void *V, const void *W, const void *P,
                  const uint8_t *bg, const void *verts, const int32_t *faces, ptv_mesh_record *records,
                  double ms2[2]) {
    ptv_mesh_params resolved;
    PTV_TRY(resident_mesh(c, given, resolved));
    const ptv_mesh_params *prm = &resolved;
    const bool resident = prm->mesh_resident != 0;
    MeshArgs a{};
    PTV_TRY(mesh_args(c, prm, a));
    if ((!resident && (!verts || !faces)) || !records || (!prm->reuse && (!U || !V || !W))) {
        set_error("mesh drag: NULL field, vertices, faces or records");
        return PTV_E_ARG;
    }
    if (prm->reuse && (!same_dims(c->mesh_dims, a.d) || c->mesh_fld_dtype != prm->field_dtype)) {
        set_error("mesh drag: reuse, but the context holds no fields of these dimensions and dtype");
        return PTV_E_ARG;
    }
    for (int64_t i = 0; !resident && i < 3 * prm->n_tris; ++i)
        if (faces[i] < 0 || faces[i] >= prm->n_verts) {
            set_error("mesh drag: a face index lies outside [0, n_verts)");
            return PTV_E_ARG;
        }
    hipStream_t s = c->stream;
    const size_t n = (size_t)a.d.nx * a.d.ny * a.d.nz, ts = a.field_f32 ? 4 : 8;
    if (!prm->reuse) {
        c->mesh_fld_dtype = -1;
        const void *src[4] = {U, V, W, P};
        for (int i = 0; i < 4; ++i) {
            if (!src[i]) continue;
            PTV_TRY(c->mesh_fld[i].ensure(n * ts));
            PTV_HIP(hipMemcpyAsync(c->mesh_fld[i].p, src[i], n * ts, hipMemcpyHostToDevice, s));
        }
        if (bg) {
            PTV_TRY(c->mesh_bg.ensure(n));
            PTV_HIP(hipMemcpyAsync(c->mesh_bg.p, bg, n, hipMemcpyHostToDevice, s));
        }
        c->mesh_has_p = P != nullptr;
        c->mesh_has_bg = bg != nullptr;
    }
    if (!resident) {  // a resident mesh is integrated where the marching cubes left it
        const size_t vbytes = (size_t)prm->n_verts * 3 * (a.vert_f32 ? 4 : 8);
        PTV_TRY(c->mesh_verts.ensure(vbytes));
        PTV_TRY(c->mesh_faces.ensure((size_t)prm->n_tris * 3));
        PTV_HIP(hipMemcpyAsync(c->mesh_verts.p, verts, vbytes, hipMemcpyHostToDevice, s));
        PTV_HIP(hipMemcpyAsync(c->mesh_faces.p, faces, (size_t)prm->n_tris * 3 * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    }
    PTV_TRY(ptv_mesh_drag_dev(c, given, c->mesh_fld[0].p, c->mesh_fld[1].p, c->mesh_fld[2].p,
                              c->mesh_has_p ? c->mesh_fld[3].p : nullptr, c->mesh_has_bg ? c->mesh_bg.p : nullptr,
                              resident ? nullptr : c->mesh_verts.p, resident ? nullptr : c->mesh_faces.p, s, records,
                              ms2));
    c->mesh_fld_dtype = prm->field_dtype;
    return PTV_OK;
}

}  // extern "C"
