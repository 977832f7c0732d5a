// ptv_flow_api.cpp — the C ABI of the reductions over a velocity or pressure grid: flow analysis
// (ptv_flow.hip), interface drag and gradient sums (ptv_drag.hip).  Every operation has one set of
// checks and one body: its host-buffer call stages through ptv_stage.hpp and runs what its entry
// point on device pointers runs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

// ---- flow analysis (ptv_flow.hip) ----
// ptv_flow_params -> FlowArgs, with the same checks for the host and device calls; the elementwise
// mode (stencil = false) reads neither the slab nor the spacings.
int flow_args(ptv_ctx *c, const ptv_flow_params *prm, bool stencil, FlowArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("flow analysis: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    const int64_t least = stencil ? 2 : 1, most = 1 << 30;
    if (prm->nx < least || prm->ny < least || prm->nz < least) {
        set_error(stencil ? "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                            "elements are required."
                          : "flow derived: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->nx > most || prm->ny > most || prm->nz > most ||
        (double)prm->nx * (double)prm->ny * (double)prm->nz >= 1099511627776.0) {
        set_error("flow analysis: fewer than 2^40 voxels, at most 2^30 per axis");
        return PTV_E_ARG;
    }
    a = FlowArgs{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.strong = prm->spacing_strong ? 1 : 0;
    a.viscosity = prm->viscosity;
    if (stencil) {
        const int64_t lo = prm->edge_lo ? 0 : 1, hi = prm->nz - (prm->edge_hi ? 0 : 1);
        if (prm->z_begin < lo || prm->z_end > hi || prm->z_begin > prm->z_end) {
            set_error("flow analysis: planes [" + std::to_string(prm->z_begin) + ", " + std::to_string(prm->z_end) +
                      ") must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) +
                      ") (a non-edge buffer end is a halo plane)");
            return PTV_E_ARG;
        }
        for (double h : {prm->dx, prm->dy, prm->dz})
            if (!(h > 0.0) || !std::isfinite(h)) {
                set_error("flow analysis: spacings must be positive and finite");
                return PTV_E_ARG;
            }
        a.z_begin = (int)prm->z_begin;
        a.z_end = (int)prm->z_end;
        a.edge_lo = prm->edge_lo ? 1 : 0;
        a.edge_hi = prm->edge_hi ? 1 : 0;
        a.dx = prm->dx;
        a.dy = prm->dy;
        a.dz = prm->dz;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int flow_analysis_args(ptv_ctx *c, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                       FlowArgs &a) {
    PTV_TRY(flow_args(c, prm, true, a));
    if (!U || !V || !W) {
        set_error("flow analysis: NULL field");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int flow_derived_args(ptv_ctx *c, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                      const void *flow_type, FlowArgs &a) {
    PTV_TRY(flow_args(c, prm, false, a));
    if (!strain || (flow_type && !vorticity_mag)) {
        set_error("flow derived: NULL strain rate, or flow type without the vorticity magnitude");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// the reduced rows -> ptv_flow_stats (synchronises `s`)
int flow_finish(ptv_ctx *c, unsigned want, int64_t nvox, hipStream_t s, ptv_flow_stats *st) {
    double h[kFlowRows];
    PTV_HIP(hipMemcpyAsync(h, c->flow_res.p, sizeof(h), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_flow0, c->ev_flow1));
    if (!st) return PTV_OK;
    *st = ptv_flow_stats{};
    st->n_voxels = nvox;
    st->n_fluid = (int64_t)h[15];
    st->sum_u = h[0];
    st->sum_v = h[1];
    st->sum_w = h[2];
    for (int k = 0; k < 4; ++k) {
        if (!(want >> k & 1)) continue;
        st->sum[k] = st->sum_fluid[k] = h[3 + 3 * k];
        st->max[k] = h[4 + 3 * k];
        st->min[k] = h[5 + 3 * k];
    }
    st->ms_stencil = ms;
    return PTV_OK;
}

int run_flow(ptv_ctx *c, const FlowArgs &a, const void *U, const void *V, const void *W, const uint8_t *M,
             void *const out[4], hipStream_t s) {
    PTV_TRY(c->flow_part.ensure(flow_partials(a)));
    PTV_TRY(c->flow_res.ensure(kFlowRows));
    PTV_TRY(c->ev_flow0.record(s));
    PTV_TRY(launch_flow(a, U, V, W, M, out, c->flow_part.p, c->flow_res.p, s));
    PTV_TRY(c->ev_flow1.record(s));
    return PTV_OK;
}

unsigned flow_want(void *const out[4]) {
    return (out[0] ? 1u : 0u) | (out[1] ? 2u : 0u) | (out[2] ? 4u : 0u) | (out[3] ? 8u : 0u);
}

// ---- interface drag and gradient sums (ptv_drag.hip) ----
int drag_dims(int64_t nx, int64_t ny, int64_t nz, int64_t least, const char *what) {
    const int64_t most = 1 << 30;
    if (nx < least || ny < least || nz < least) {
        set_error(least == 2 ? "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                               "elements are required."
                             : std::string(what) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    if (nx > most || ny > most || nz > most || (double)nx * (double)ny * (double)nz >= 1099511627776.0) {
        set_error(std::string(what) + ": fewer than 2^40 voxels, at most 2^30 per axis");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// ptv_drag_params -> DragArgs, with the same checks for the host and device calls
int drag_args(ptv_ctx *c, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
              const void *W, const ptv_drag_stats *records, DragArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("interface drag: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    PTV_TRY(drag_dims(prm->nx, prm->ny, prm->nz, 1, "interface drag"));
    for (double h : {prm->dx, prm->dy, prm->dz})
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("interface drag: spacings must be positive and finite");
            return PTV_E_ARG;
        }
    if (!std::isfinite(prm->viscosity)) {
        set_error("interface drag: viscosity must be finite");
        return PTV_E_ARG;
    }
    if (prm->n_labels < 1 || !prm->labels) {
        set_error("interface drag: at least one label");
        return PTV_E_ARG;
    }
    for (int i = 0; i < prm->n_labels; ++i)
        if (prm->labels[i] <= 0 || (i > 0 && prm->labels[i] <= prm->labels[i - 1])) {
            set_error("interface drag: labels must be positive and strictly ascending");
            return PTV_E_ARG;
        }
    a = DragArgs{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.area[0] = prm->dy * prm->dx;
    a.area[1] = prm->dz * prm->dx;
    a.area[2] = prm->dz * prm->dy;
    a.step[0] = prm->dz;
    a.step[1] = prm->dy;
    a.step[2] = prm->dx;
    a.viscosity = prm->viscosity;
    PTV_HIP(hipSetDevice(c->device));
    if (!mask || !U || !V || !W || !records) {
        set_error("interface drag: NULL mask, field or records");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// what the host call of the gradient sums can check before it copies
int gradient_sums_args(ptv_ctx *c, const ptv_flow_params *prm, const void *P, const double *sums3) {
    if (!c || !prm || !P || !sums3) {
        set_error("gradient sums: NULL argument");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("gradient sums: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    return drag_dims(prm->nx, prm->ny, prm->nz, 2, "gradient sums");
}

}  // namespace

extern "C" {

int ptv_flow_analysis_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                          void *strain, void *dissipation, void *vorticity, void *flow_type, void *stream,
                          ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_analysis_args(c, prm, U, V, W, a));
    if (st) *st = ptv_flow_stats{};
    if (a.z_end <= a.z_begin) return PTV_OK;
    void *const out[4] = {strain, dissipation, vorticity, flow_type};
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_flow(c, a, U, V, W, prm->fluid_mask, out, s));
    return flow_finish(c, flow_want(out), (prm->z_end - prm->z_begin) * prm->nx * prm->ny, s, st);
}

int ptv_flow_analysis(ptv_ctx *c, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                      void *strain, void *dissipation, void *vorticity, void *flow_type, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_analysis_args(c, prm, U, V, W, a));
    if (st) *st = ptv_flow_stats{};
    if (a.z_end <= a.z_begin) return PTV_OK;  // an empty slab: before any copy
    Stage sg(c);
    const size_t ts = a.field_f32 ? 4 : 8;
    const int64_t nfull = prm->nz * prm->nx * prm->ny;
    const int64_t nout = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    const void *dU = sg.in(0, U, nfull * ts), *dV = sg.in(1, V, nfull * ts), *dW = sg.in(2, W, nfull * ts);
    const uint8_t *M = sg.mask(prm->fluid_mask, nfull);
    void *const host[4] = {strain, dissipation, vorticity, flow_type};
    void *out[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k)
        if (host[k]) out[k] = sg.room(3 + k, nout * ts);
    PTV_TRY(sg.rc);
    PTV_TRY(run_flow(c, a, dU, dV, dW, M, out, sg.s));
    for (int k = 0; k < 4; ++k)
        if (host[k]) sg.back(host[k], 3 + k, nout * ts);
    PTV_TRY(sg.rc);
    return flow_finish(c, flow_want(out), nout, sg.s, st);
}

int ptv_flow_derived_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                         void *dissipation, void *flow_type, void *stream, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_derived_args(c, prm, strain, vorticity_mag, flow_type, a));
    if (st) *st = ptv_flow_stats{};
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int64_t n = prm->nz * prm->nx * prm->ny;
    PTV_TRY(c->flow_part.ensure(flow_derived_partials(n)));
    PTV_TRY(c->flow_res.ensure(kFlowRows));
    PTV_TRY(c->ev_flow0.record(s));
    PTV_TRY(launch_flow_derived(a, n, strain, vorticity_mag, prm->fluid_mask, dissipation, flow_type, c->flow_part.p,
                                c->flow_res.p, s));
    PTV_TRY(c->ev_flow1.record(s));
    return flow_finish(c, (dissipation ? 2u : 0u) | (flow_type ? 8u : 0u), n, s, st);
}

int ptv_flow_derived(ptv_ctx *c, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                     void *dissipation, void *flow_type, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_derived_args(c, prm, strain, vorticity_mag, flow_type, a));
    Stage sg(c);
    const size_t ts = a.field_f32 ? 4 : 8;
    const int64_t n = prm->nz * prm->nx * prm->ny;
    const void *dS = sg.in(0, strain, n * ts);
    const void *dO = flow_type ? sg.in(1, vorticity_mag, n * ts) : nullptr;  // read for the flow type only
    ptv_flow_params dp = *prm;
    dp.fluid_mask = sg.mask(prm->fluid_mask, n);
    void *const host[2] = {dissipation, flow_type};
    void *out[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k)
        if (host[k]) out[k] = sg.room(2 + k, n * ts);
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_flow_derived_dev(c, &dp, dS, dO, out[0], out[1], sg.s, st));
    for (int k = 0; k < 2; ++k)  // the device call has synchronised: a blocking copy
        if (host[k]) PTV_HIP(hipMemcpy(host[k], out[k], n * ts, hipMemcpyDeviceToHost));
    return PTV_OK;
}

int ptv_interface_drag_dev(ptv_ctx *c, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
                           const void *W, const void *P, void *stream, ptv_drag_stats *records, double *ms) {
    DragArgs a{};
    PTV_TRY(drag_args(c, prm, mask, U, V, W, records, a));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int nl = prm->n_labels;
    const size_t nrows = (size_t)nl * kDragSlotRows;
    PTV_TRY(c->drag_part.ensure(drag_partials(a, nl)));
    PTV_TRY(c->drag_res.ensure(nrows));
    PTV_TRY(c->drag_labels.ensure((size_t)nl));
    PTV_HIP(hipMemcpyAsync(c->drag_labels.p, prm->labels, (size_t)nl * sizeof(int), hipMemcpyHostToDevice, s));
    PTV_TRY(c->ev_drag0.record(s));
    PTV_TRY(launch_drag(a, mask, U, V, W, P, c->drag_labels.p, nl, c->drag_part.p, c->drag_res.p, s));
    PTV_TRY(c->ev_drag1.record(s));
    std::vector<double> h(nrows);
    PTV_HIP(hipMemcpyAsync(h.data(), c->drag_res.p, nrows * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    float t = 0.f;
    PTV_HIP(hipEventElapsedTime(&t, c->ev_drag0, c->ev_drag1));
    if (ms) *ms = t;
    for (size_t r = 0; r < (size_t)nl * 6; ++r) {
        const double *v = h.data() + r * kDragVals;
        records[r] = ptv_drag_stats{(int64_t)v[0], v[1], v[2], v[3], v[4]};  // a count is an exact integer
    }
    return PTV_OK;
}

int ptv_interface_drag(ptv_ctx *c, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
                       const void *W, const void *P, ptv_drag_stats *records, double *ms) {
    DragArgs a{};
    PTV_TRY(drag_args(c, prm, mask, U, V, W, records, a));
    Stage sg(c);
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz), ts = a.field_f32 ? 4 : 8;
    const int32_t *dM = sg.in<int32_t>(0, mask, n * sizeof(int32_t));
    const void *dU = sg.in(1, U, n * ts), *dV = sg.in(2, V, n * ts), *dW = sg.in(3, W, n * ts);
    const void *dP = P ? sg.in(4, P, n * ts) : nullptr;
    PTV_TRY(sg.rc);
    return ptv_interface_drag_dev(c, prm, dM, dU, dV, dW, dP, sg.s, records, ms);
}

int ptv_gradient_sums_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *P, void *stream, double sums3[3]) {
    PTV_TRY(gradient_sums_args(c, prm, P, sums3));
    if (prm->z_begin != 0 || prm->z_end != prm->nz || !prm->edge_lo || !prm->edge_hi) {
        set_error("gradient sums: the plane range must be the whole buffer");
        return PTV_E_UNSUPPORTED;
    }
    for (double h : {prm->dx, prm->dy, prm->dz})
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("gradient sums: spacings must be positive and finite");
            return PTV_E_ARG;
        }
    DragArgs a{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.strong = prm->spacing_strong ? 1 : 0;
    a.step[0] = prm->dz;
    a.step[1] = prm->dy;
    a.step[2] = prm->dx;
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(c->drag_part.ensure(drag_partials(a, 0)));
    PTV_TRY(c->drag_res.ensure(3));
    PTV_TRY(c->ev_drag0.record(s));
    PTV_TRY(launch_gradient_sums(a, P, c->drag_part.p, c->drag_res.p, s));
    PTV_TRY(c->ev_drag1.record(s));
    PTV_HIP(hipMemcpyAsync(sums3, c->drag_res.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_gradient_sums(ptv_ctx *c, const ptv_flow_params *prm, const void *P, double sums3[3]) {
    PTV_TRY(gradient_sums_args(c, prm, P, sums3));
    PTV_HIP(hipSetDevice(c->device));
    Stage sg(c);
    const size_t bytes = (size_t)(prm->nx * prm->ny * prm->nz) * (prm->field_dtype == PTV_F32 ? 4 : 8);
    const void *dP = sg.in(0, P, bytes);
    PTV_TRY(sg.rc);
    return ptv_gradient_sums_dev(c, prm, dP, sg.s, sums3);  // the unsupported-slab check comes after the upload
}

}  // extern "C"
