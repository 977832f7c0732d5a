// ptv_surface_api.cpp — the C ABI of the device marching cubes (ptv_surface.hip): argument
// validation, the host-mask call, the entry point on a device mask, and the copy-out of the mesh the
// context keeps (ptv_mesh_drag with prm->mesh_resident integrates it where it lies).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

int surface_args(ptv_ctx *c, const ptv_surface_params *prm, SurfDims &d) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    const int64_t most = 1 << 30;
    if (prm->nx < 1 || prm->ny < 1 || prm->nz < 1) {
        set_error("marching cubes: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->step_size < 1) {
        set_error("marching cubes: step_size must be at least 1");
        return PTV_E_ARG;
    }
    if (prm->n_labels < 1 || !prm->labels) {
        set_error("marching cubes: at least one label");
        return PTV_E_ARG;
    }
    for (int l = 0; l < prm->n_labels; ++l)
        if (prm->labels[l] <= 0 || (l > 0 && prm->labels[l] <= prm->labels[l - 1])) {
            set_error("marching cubes: labels must be positive, ascending and distinct");
            return PTV_E_ARG;
        }
    if (prm->nx > most || prm->ny > most || prm->nz > most) {
        set_error("marching cubes: at most 2^30 voxels per axis");
        return PTV_E_UNSUPPORTED;
    }
    if (prm->n_labels > 65535 * 32) {
        set_error("marching cubes: at most 2097120 labels");
        return PTV_E_UNSUPPORTED;
    }
    const int64_t st = prm->step_size;
    d = SurfDims{(int)prm->nx, (int)prm->ny, (int)prm->nz, (int)(st > most ? most : st), 0, 0, 0};
    d.lx = (int)((prm->nx - 1) / st + 1);
    d.ly = (int)((prm->ny - 1) / st + 1);
    d.lz = (int)((prm->nz - 1) / st + 1);
    if ((double)d.lx * (double)d.ly * (double)d.lz >= 2147483647.0) {
        set_error("marching cubes: 2^31 - 1 or more lattice points");
        return PTV_E_UNSUPPORTED;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_marching_cubes_dev(ptv_ctx *c, const ptv_surface_params *prm, const int32_t *mask, void *stream,
                           int64_t *vert_counts, int64_t *tri_counts, double ms2[2]) {
    SurfDims d{};
    PTV_TRY(surface_args(c, prm, d));
    if (!mask || !vert_counts || !tri_counts) {
        set_error("marching cubes: NULL mask or counts");
        return PTV_E_ARG;
    }
    const int nl = prm->n_labels;
    SurfWork &w = c->surf;
    if (ms2) ms2[0] = ms2[1] = 0.0;
    if (d.lx < 2 || d.ly < 2 || d.lz < 2) {  // an axis without a cube: no label has a surface
        w.vstart.assign((size_t)nl + 1, 0);
        w.tstart.assign((size_t)nl + 1, 0);
        w.n_labels = nl;
    } else {
        hipStream_t s = stream ? (hipStream_t)stream : c->stream;
        PTV_TRY(c->h_misc.ensure(kHostWords));
        PTV_TRY(run_marching_cubes(w, d, mask, prm->labels, nl, s, c->ev_surf, c->h_misc.p));
        if (ms2) {
            float t = 0.f;
            PTV_HIP(hipEventElapsedTime(&t, c->ev_surf[0], c->ev_surf[1]));
            ms2[0] = t;
            PTV_HIP(hipEventElapsedTime(&t, c->ev_surf[1], c->ev_surf[2]));
            ms2[1] = t;
        }
    }
    for (int l = 0; l < nl; ++l) {
        vert_counts[l] = w.vstart[l + 1] - w.vstart[l];
        tri_counts[l] = w.tstart[l + 1] - w.tstart[l];
    }
    return PTV_OK;
}

int ptv_marching_cubes(ptv_ctx *c, const ptv_surface_params *prm, const int32_t *mask, int64_t *vert_counts,
                       int64_t *tri_counts, double ms2[2]) {
    SurfDims d{};
    PTV_TRY(surface_args(c, prm, d));
    if (!mask) {
        set_error("marching cubes: NULL mask or counts");
        return PTV_E_ARG;
    }
    const size_t n = (size_t)prm->nx * (size_t)prm->ny * (size_t)prm->nz;
    Stage sg(c);
    const int32_t *dM = sg.in<int32_t>(0, mask, n * sizeof(int32_t));
    PTV_TRY(sg.rc);
    return ptv_marching_cubes_dev(c, prm, dM, sg.s, vert_counts, tri_counts, ms2);
}

int ptv_surface_fetch(ptv_ctx *c, float *verts, int32_t *faces) {
    if (!c) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    const SurfWork &w = c->surf;
    if (w.n_labels < 1) {
        set_error("surface fetch: the context holds no mesh");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    const int64_t nv = w.vstart[w.n_labels], nt = w.tstart[w.n_labels];
    if (verts && nv > 0)
        PTV_HIP(hipMemcpy(verts, w.verts.p, (size_t)nv * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (faces && nt > 0) {
        PTV_HIP(hipMemcpy(faces, w.faces.p, (size_t)nt * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
        // the device keeps indices into all labels' vertices together (what the traction kernel reads)
        for (int l = 0; l < w.n_labels; ++l) {
            const int32_t v0 = (int32_t)w.vstart[l];
            if (v0 == 0) continue;
            for (int64_t i = 3 * w.tstart[l]; i < 3 * w.tstart[l + 1]; ++i) faces[i] -= v0;
        }
    }
    return PTV_OK;
}

}  // extern "C"
