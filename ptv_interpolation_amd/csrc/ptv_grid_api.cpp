// ptv_grid_api.cpp — the C ABI of the dense-grid stencils and solvers: divergence (ptv_div.hip),
// projection cleaning (ptv_clean.hip), variational cleaning (ptv_variational.hip) and pressure
// recovery (ptv_pressure.hip).  Every operation has one set of checks and one body: its host-buffer
// call stages through ptv_stage.hpp and runs what its entry point on device pointers runs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

// ptv_div_params -> DivArgs, with the same checks for the host and device calls.
int div_args(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W, const void *out,
             DivArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!U || !V || !W || !out || !prm->fluid_mask) {
        set_error("divergence: NULL field, output or fluid mask");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30)) {
        set_error("divergence: dimensions must be positive");
        return PTV_E_ARG;
    }
    const int64_t lo = prm->edge_lo ? 0 : 1, hi = prm->nz - (prm->edge_hi ? 0 : 1);
    if (prm->z_begin < lo || prm->z_end > hi || prm->z_begin > prm->z_end) {
        set_error("divergence: planes [" + std::to_string(prm->z_begin) + ", " + std::to_string(prm->z_end) +
                  ") must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) +
                  ") (a non-edge buffer end is a halo plane)");
        return PTV_E_ARG;
    }
    if ((prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) ||
        (prm->result_dtype != PTV_F64 && prm->result_dtype != PTV_F32)) {
        set_error("divergence: dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.z_begin = (int)prm->z_begin;
    a.z_end = (int)prm->z_end;
    a.edge_lo = prm->edge_lo ? 1 : 0;
    a.edge_hi = prm->edge_hi ? 1 : 0;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.result_f32 = prm->result_dtype == PTV_F32;
    a.dx = prm->dx;
    a.dy = prm->dy;
    a.dz = prm->dz;
    if (!a.field_f32 && a.result_f32) {
        set_error("divergence: float64 fields cannot give float32 results (numpy promotion)");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int run_div(ptv_ctx *c, const DivArgs &a, const void *U, const void *V, const void *W, const uint8_t *M, void *out,
            hipStream_t s) {
    PTV_TRY(c->ev_div0.record(s));
    PTV_TRY(launch_divergence(a, U, V, W, M, out, s));
    PTV_TRY(c->ev_div1.record(s));
    c->div_pending = true;
    return PTV_OK;
}

// What every call of a solver family checks first: context and parameters, the fluid mask, the
// dimensions; `what` is the family's name in its messages.
template <typename Params>
int grid_check(ptv_ctx *c, const Params *prm, const char *what, GridSpec &g) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!prm->fluid_mask) {
        set_error(std::string(what) + ": the fluid mask is required");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30) || prm->nx * prm->ny * prm->nz > 0x7fff0000LL) {
        set_error(std::string(what) + ": dimensions must be positive, with fewer than 2^31 voxels");
        return PTV_E_ARG;
    }
    g = GridSpec{(int)prm->nx, (int)prm->ny, (int)prm->nz, prm->dx, prm->dy, prm->dz};
    return PTV_OK;
}

// After a family's checks: the call's own pointer test, then the device.
int ptrs_check(ptv_ctx *c, bool all_given, const char *null_msg) {
    if (!all_given) {
        set_error(null_msg);
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

template <typename Params>
size_t voxels(const Params *prm) {
    return (size_t)(prm->nx * prm->ny * prm->nz);
}

// three host grids -> slots first .. first + 2
void in3(Stage &st, int first, const double *a, const double *b, const double *c3, size_t bytes, double *d[3]) {
    const double *src[3] = {a, b, c3};
    for (int i = 0; i < 3; ++i) d[i] = st.in<double>(first + i, src[i], bytes);
}
// slots first .. first + 2 -> three host grids
void back3(Stage &st, double *a, double *b, double *c3, int first, size_t bytes) {
    double *dst[3] = {a, b, c3};
    for (int i = 0; i < 3; ++i) st.back(dst[i], first + i, bytes);
}

// ---- divergence cleaning (ptv_clean.hip) ----
int clean_args(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V, const double *W,
               const double *Uo, const double *Vo, const double *Wo, GridSpec &g) {
    PTV_TRY(grid_check(c, prm, "clean", g));
    return ptrs_check(c, U && V && W && Uo && Vo && Wo, "clean: NULL field or output");
}
CleanSolve clean_solve(const ptv_clean_params *prm) {
    return CleanSolve{prm->iterations, prm->damp, prm->atol, prm->btol, prm->iter_lim};
}

// ---- variational divergence cleaning (ptv_variational.hip) ----
int var_args(ptv_ctx *c, const ptv_variational_params *prm, const double *U, const double *V, const double *W,
             const double *Uo, const double *Vo, const double *Wo, GridSpec &g) {
    PTV_TRY(grid_check(c, prm, "variational", g));
    return ptrs_check(c, U && V && W && Uo && Vo && Wo, "variational: NULL field or output");
}
VarSolve var_solve(const ptv_variational_params *prm) { return VarSolve{prm->lambda_reg, prm->rtol, prm->maxiter}; }

// ---- pressure recovery (ptv_pressure.hip; the LSQR solve is ptv_clean.hip's) ----
// every argument check of the family, before any copy or launch
int press_check(ptv_ctx *c, const ptv_pressure_params *prm, GridSpec &g) {
    PTV_TRY(grid_check(c, prm, "pressure", g));
    for (double h : {prm->dx, prm->dy, prm->dz}) {
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("pressure: spacings must be positive finite numbers");
            return PTV_E_ARG;
        }
    }
    if (!std::isfinite(prm->mu) || !std::isfinite(prm->rho)) {
        set_error("pressure: mu and rho must be finite");
        return PTV_E_ARG;
    }
    if (prm->wall_bc != PTV_WALL_ZERO_NEUMANN && prm->wall_bc != PTV_WALL_INHOMOGENEOUS) {
        set_error("pressure: wall_bc must be PTV_WALL_ZERO_NEUMANN or PTV_WALL_INHOMOGENEOUS");
        return PTV_E_ARG;
    }
    if (prm->anchor < PTV_ANCHOR_NONE || prm->anchor > PTV_ANCHOR_INLET || prm->flow_direction < -1 ||
        prm->flow_direction > 1) {
        set_error("pressure: anchor must be PTV_ANCHOR_* and flow_direction -1, 0 or 1");
        return PTV_E_ARG;
    }
    if (!std::isfinite(prm->rtol) || prm->maxiter < 0 || prm->lsqr_iter_lim < 0 || !(prm->lsqr_damp >= 0.0) ||
        !(prm->lsqr_atol >= 0.0) || !(prm->lsqr_btol >= 0.0)) {
        set_error("pressure: rtol must be finite; maxiter and the LSQR settings non-negative");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int press_rho_check(const ptv_pressure_params *prm) {
    if (prm->rho > 0.0 && (prm->nx < 2 || prm->ny < 2 || prm->nz < 2)) {
        set_error("pressure: rho > 0 needs at least 2 voxels along every axis (np.gradient)");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int force_field_args(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                     const double *Fx, const double *Fy, const double *Fz, GridSpec &g) {
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    return ptrs_check(c, U && V && W && Fx && Fy && Fz, "force_field: NULL field or output");
}

int force_divergence_args(ptv_ctx *c, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                          const double *Fz, const double *D, GridSpec &g) {
    PTV_TRY(press_check(c, prm, g));
    return ptrs_check(c, Fx && Fy && Fz && D, "force_divergence: NULL field or output");
}

int poisson_solve_args(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                       const double *Fy, const double *Fz, const double *X, GridSpec &g) {
    PTV_TRY(press_check(c, prm, g));
    return ptrs_check(c, X && (rhs || (Fx && Fy && Fz)),
                      "poisson_solve: NULL output, or neither a right-hand side nor a force field");
}

int pressure_recover_args(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                          const double *W, const double *P, GridSpec &g) {
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    return ptrs_check(c, U && V && W && P, "pressure_recover: NULL field or output");
}

// CG with a Dirichlet grid, LSQR without one; all pointers device memory
int press_solve(ptv_ctx *c, const ptv_pressure_params *prm, const GridSpec &g, const uint8_t *M, const double *rhs,
                const uint8_t *Dir, double *X, hipStream_t s, ptv_pressure_stats &out) {
    if (Dir) return press_cg(c->press, g, prm->rtol, prm->maxiter, M, Dir, rhs, X, s, &out);
    const CleanSolve sv{0, prm->lsqr_damp, prm->lsqr_atol, prm->lsqr_btol, prm->lsqr_iter_lim};
    CleanRhsResult r{};
    PTV_TRY(clean_solve_rhs(c->clean, g, sv, M, rhs, X, s, &r));
    out.solver = 1;
    out.n_fluid = r.n_fluid;
    out.n_dirichlet = 0;
    out.itn = r.itn;
    out.info = r.istop;
    out.bnorm = r.bnorm;
    out.rnorm = r.rnorm;
    out.ms_solve = r.ms_solve;
    out.ms_iter_median = r.ms_iter_median;
    return PTV_OK;
}

// ---- the preconditioned anchored solve (ptv_multigrid.hip, press_pcg) ----
// the family's checks, then the multigrid parameters and the level table (host arithmetic only)
int mg_check(ptv_ctx *c, const ptv_pressure_params *prm, const ptv_mg_params *mg, GridSpec &g, MgPlan &plan) {
    PTV_TRY(press_check(c, prm, g));
    return mg_plan(g, mg, plan);
}

int needs_dirichlet(bool given, const char *who) {
    if (given) return PTV_OK;
    set_error(std::string(who) + ": the multigrid preconditioner serves the anchored (CG) solve only; "
              "the solve without a Dirichlet set is LSQR and takes no preconditioner");
    return PTV_E_UNSUPPORTED;
}

// the parameters of a host call with its staged fluid mask in place of the caller's
ptv_pressure_params on_device(const ptv_pressure_params *prm, const uint8_t *M) {
    ptv_pressure_params dp = *prm;
    dp.fluid_mask = M;
    return dp;
}

}  // namespace

extern "C" {

int ptv_divergence_dev(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W,
                       void *out, void *stream, ptv_stats *st) {
    DivArgs a{};
    PTV_TRY(div_args(c, prm, U, V, W, out, a));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_div(c, a, U, V, W, prm->fluid_mask, out, s));
    c->last.n_voxels = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_divergence(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W, void *out,
                   ptv_stats *st) {
    DivArgs a{};
    PTV_TRY(div_args(c, prm, U, V, W, out, a));
    Stage sg(c);
    Event ev[4];
    const size_t ts = a.field_f32 ? 4 : 8, rs = a.result_f32 ? 4 : 8;
    const int64_t nfull = prm->nz * prm->nx * prm->ny;
    const int64_t nout = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    PTV_TRY(ev[0].record(sg.s));
    const void *dU = sg.in(0, U, nfull * ts), *dV = sg.in(1, V, nfull * ts), *dW = sg.in(2, W, nfull * ts);
    const uint8_t *M = sg.mask(prm->fluid_mask, nfull);
    void *dout = sg.room(3, nout * rs);
    PTV_TRY(sg.rc);
    PTV_TRY(ev[1].record(sg.s));
    PTV_TRY(run_div(c, a, dU, dV, dW, M, dout, sg.s));
    PTV_TRY(ev[2].record(sg.s));
    sg.back(out, 3, nout * rs);
    PTV_TRY(sg.rc);
    PTV_TRY(ev[3].record(sg.s));
    PTV_TRY(sg.sync());
    PTV_TRY(finish_host_timing(c, ev));
    c->last.n_voxels = nout;
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_clean_divergence_dev(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                             const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                             ptv_clean_stats *st) {
    GridSpec g{};
    PTV_TRY(clean_args(c, prm, U, V, W, Uo, Vo, Wo, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return clean_run(c->clean, g, clean_solve(prm), prm->fluid_mask, U, V, W, Uo, Vo, Wo, s, st);
}

int ptv_clean_divergence(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, double *Uo, double *Vo, double *Wo, ptv_clean_stats *st) {
    GridSpec g{};
    PTV_TRY(clean_args(c, prm, U, V, W, Uo, Vo, Wo, g));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3];
    in3(sg, 0, U, V, W, bytes, d);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    PTV_TRY(sg.rc);
    PTV_TRY(clean_run(c->clean, g, clean_solve(prm), M, d[0], d[1], d[2], d[0], d[1], d[2], sg.s, st));  // in place
    back3(sg, Uo, Vo, Wo, 0, bytes);
    return sg.sync();
}

int ptv_apply_correction(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, const double *phi_grid, double *Uo, double *Vo, double *Wo) {
    GridSpec g{};
    PTV_TRY(grid_check(c, prm, "clean", g));
    PTV_TRY(ptrs_check(c, U && V && W && phi_grid && Uo && Vo && Wo, "apply_correction: NULL field, phi or output"));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3];
    in3(sg, 0, U, V, W, bytes, d);
    const double *phi = sg.in<double>(3, phi_grid, bytes);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    PTV_TRY(sg.rc);
    PTV_TRY(launch_clean_correction(g, M, d[0], d[1], d[2], phi, d[0], d[1], d[2], sg.s));
    back3(sg, Uo, Vo, Wo, 0, bytes);
    return sg.sync();
}

int ptv_laplacian_apply(ptv_ctx *c, const ptv_clean_params *prm, const double *x_grid, double *y_grid) {
    GridSpec g{};
    PTV_TRY(grid_check(c, prm, "clean", g));
    PTV_TRY(ptrs_check(c, x_grid && y_grid, "laplacian_apply: NULL input or output"));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    const double *x = sg.in<double>(0, x_grid, bytes);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    double *y = sg.room<double>(1, bytes);
    PTV_TRY(sg.rc);
    PTV_TRY(launch_clean_laplacian(g, M, x, y, sg.s));
    sg.back(y_grid, 1, bytes);
    return sg.sync();
}

int ptv_clean_variational_dev(ptv_ctx *c, const ptv_variational_params *prm, const double *U, const double *V,
                              const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                              ptv_variational_stats *st) {
    GridSpec g{};
    PTV_TRY(var_args(c, prm, U, V, W, Uo, Vo, Wo, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return variational_run(c->var, g, var_solve(prm), prm->fluid_mask, U, V, W, Uo, Vo, Wo, s, st);
}

int ptv_clean_variational(ptv_ctx *c, const ptv_variational_params *prm, const double *U, const double *V,
                          const double *W, double *Uo, double *Vo, double *Wo, ptv_variational_stats *st) {
    GridSpec g{};
    PTV_TRY(var_args(c, prm, U, V, W, Uo, Vo, Wo, g));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3];
    in3(sg, 0, U, V, W, bytes, d);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    PTV_TRY(sg.rc);
    PTV_TRY(variational_run(c->var, g, var_solve(prm), M, d[0], d[1], d[2], d[0], d[1], d[2], sg.s, st));  // in place
    back3(sg, Uo, Vo, Wo, 0, bytes);
    return sg.sync();
}

int ptv_divergence_operator_apply(ptv_ctx *c, const ptv_variational_params *prm, const double *xu, const double *xv,
                                  const double *xw, double *d_grid) {
    GridSpec g{};
    PTV_TRY(grid_check(c, prm, "variational", g));
    PTV_TRY(ptrs_check(c, xu && xv && xw && d_grid, "divergence_operator_apply: NULL input or output"));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *x[3];
    in3(sg, 0, xu, xv, xw, bytes, x);
    double *d = sg.room<double>(3, bytes);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    PTV_TRY(sg.rc);
    PTV_TRY(launch_var_divergence(g, M, x[0], x[1], x[2], d, sg.s));
    sg.back(d_grid, 3, bytes);
    return sg.sync();
}

int ptv_variational_apply(ptv_ctx *c, const ptv_variational_params *prm, const double *xu, const double *xv,
                          const double *xw, double *yu, double *yv, double *yw) {
    GridSpec g{};
    PTV_TRY(grid_check(c, prm, "variational", g));
    PTV_TRY(ptrs_check(c, xu && xv && xw && yu && yv && yw, "variational_apply: NULL input or output"));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *x[3], *y[3];
    in3(sg, 0, xu, xv, xw, bytes, x);
    for (int i = 0; i < 3; ++i) y[i] = sg.room<double>(3 + i, bytes);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    PTV_TRY(sg.rc);
    PTV_TRY(c->var.d.ensure(voxels(prm)));
    PTV_TRY(launch_var_divergence(g, M, x[0], x[1], x[2], c->var.d.p, sg.s));
    PTV_TRY(launch_var_adjoint(g, prm->lambda_reg, M, c->var.d.p, x[0], x[1], x[2], y[0], y[1], y[2], c->var.part,
                               sg.s));
    back3(sg, yu, yv, yw, 3, bytes);
    return sg.sync();
}

int ptv_force_field_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                        double *Fx, double *Fy, double *Fz, void *stream, ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(force_field_args(c, prm, U, V, W, Fx, Fy, Fz, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(press_force(c->press, g, prm->mu, prm->rho, prm->fluid_mask, U, V, W, Fx, Fy, Fz, s, &out));
    out.ms_total = out.ms_force;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_force_field(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                    double *Fx, double *Fy, double *Fz, ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(force_field_args(c, prm, U, V, W, Fx, Fy, Fz, g));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3], *F[3];
    in3(sg, 0, U, V, W, bytes, d);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, voxels(prm)));
    for (int i = 0; i < 3; ++i) F[i] = sg.room<double>(3 + i, bytes);
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_force_field_dev(c, &dp, d[0], d[1], d[2], F[0], F[1], F[2], sg.s, st));
    back3(sg, Fx, Fy, Fz, 3, bytes);
    return sg.sync();
}

int ptv_force_divergence_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                             const double *Fz, double *D, void *stream) {
    GridSpec g{};
    PTV_TRY(force_divergence_args(c, prm, Fx, Fy, Fz, D, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, prm->fluid_mask, Fx, Fy, Fz, D, s);
}

int ptv_force_divergence(ptv_ctx *c, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                         const double *Fz, double *D) {
    GridSpec g{};
    PTV_TRY(force_divergence_args(c, prm, Fx, Fy, Fz, D, g));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *F[3];
    in3(sg, 0, Fx, Fy, Fz, bytes, F);
    const uint8_t *M = sg.mask(prm->fluid_mask, voxels(prm));
    double *d = sg.room<double>(3, bytes);
    PTV_TRY(sg.rc);
    PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, M, F[0], F[1], F[2], d, sg.s));
    sg.back(D, 3, bytes);
    return sg.sync();
}

int ptv_poisson_solve_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                          const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X, void *stream,
                          ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(poisson_solve_args(c, prm, rhs, Fx, Fy, Fz, X, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(c->ev_press[0].record(s));
    if (!rhs) {
        PTV_TRY(c->press.rhs.ensure(voxels(prm)));
        PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, prm->fluid_mask, Fx, Fy, Fz,
                                 c->press.rhs.p, s));
        rhs = c->press.rhs.p;
    }
    PTV_TRY(press_solve(c, prm, g, prm->fluid_mask, rhs, dirichlet, X, s, out));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_poisson_solve(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                      const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X,
                      ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(poisson_solve_args(c, prm, rhs, Fx, Fy, Fz, X, g));
    Stage sg(c);
    const size_t n = voxels(prm), bytes = n * sizeof(double);
    // slot 0: the right-hand side, solved in place, or room for the solution; 1 .. 3: the force field
    double *F[3] = {nullptr, nullptr, nullptr};
    double *x = rhs ? sg.in<double>(0, rhs, bytes) : sg.room<double>(0, bytes);
    if (!rhs) in3(sg, 1, Fx, Fy, Fz, bytes, F);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, n));
    const uint8_t *dir = dirichlet ? sg.in<uint8_t>(4, dirichlet, n) : nullptr;
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_poisson_solve_dev(c, &dp, rhs ? x : nullptr, F[0], F[1], F[2], dir, x, sg.s, st));
    sg.back(X, 0, bytes);
    return sg.sync();
}

int ptv_pressure_recover_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                             const double *W, double *P, void *stream, ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(pressure_recover_args(c, prm, U, V, W, P, g));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = voxels(prm);
    PTV_TRY(c->press.f.ensure(3 * n));
    PTV_TRY(c->press.rhs.ensure(n));
    PTV_TRY(c->press.dir.ensure(n));
    double *F = c->press.f.p;
    const uint8_t *M = prm->fluid_mask;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(c->ev_press[0].record(s));
    PTV_TRY(press_force(c->press, g, prm->mu, prm->rho, M, U, V, W, F, F + n, F + 2 * n, s, &out));
    if (out.n_fluid == 0) {  // physics.py:274-276
        PTV_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
        PTV_HIP(hipStreamSynchronize(s));
        if (st) *st = out;
        return PTV_OK;
    }
    PTV_TRY(c->ev_press[1].record(s));
    PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, M, F, F + n, F + 2 * n, c->press.rhs.p, s));
    PTV_TRY(c->ev_press[2].record(s));
    const uint8_t *Dir = nullptr;
    if (prm->anchor != PTV_ANCHOR_NONE) {
        // velocity_analysis.py:304-321: np.mean(w[mask]) >= 0 has the sign of the sum
        const bool positive = prm->flow_direction == 1 || (prm->flow_direction == 0 && out.sum_w >= 0.0);
        const bool last = (prm->anchor == PTV_ANCHOR_OUTLET) == positive;
        out.anchor_plane = last ? g.nz - 1 : 0;
        PTV_TRY(press_anchor_plane(g, out.anchor_plane, M, c->press.dir.p, s));
        Dir = c->press.dir.p;
    }
    PTV_TRY(press_solve(c, prm, g, M, c->press.rhs.p, Dir, P, s, out));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[1], c->ev_press[2]));
    out.ms_divergence = ms;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_pressure_recover(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                         const double *W, double *P, ptv_pressure_stats *st) {
    GridSpec g{};
    PTV_TRY(pressure_recover_args(c, prm, U, V, W, P, g));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3];
    in3(sg, 0, U, V, W, bytes, d);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, voxels(prm)));
    double *p = sg.room<double>(3, bytes);
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_pressure_recover_dev(c, &dp, d[0], d[1], d[2], p, sg.s, st));
    sg.back(P, 3, bytes);
    return sg.sync();
}

int ptv_poisson_mg_apply_dev(ptv_ctx *c, const ptv_pressure_params *prm, const ptv_mg_params *mg,
                             const uint8_t *dirichlet, const double *r, double *z, void *stream,
                             ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(mg_check(c, prm, mg, g, plan));
    PTV_TRY(ptrs_check(c, r && z && r != z, "poisson_mg_apply: NULL input or output, or z aliases r"));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(mg_setup(c->mg, plan, prm->fluid_mask, dirichlet, s));
    PTV_TRY(c->mg.ev[2].record(s));
    PTV_TRY(mg_vcycle(c->mg, plan, prm->fluid_mask, dirichlet, nullptr, r, z, nullptr, s));
    PTV_TRY(c->mg.ev[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    if (mst) {
        PTV_TRY(mg_fill_stats(c->mg, plan, mst));
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, c->mg.ev[2], c->mg.ev[3]));
        mst->ms_vcycle_median = ms;
    }
    return PTV_OK;
}

int ptv_poisson_mg_apply(ptv_ctx *c, const ptv_pressure_params *prm, const ptv_mg_params *mg,
                         const uint8_t *dirichlet, const double *r, double *z, ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(mg_check(c, prm, mg, g, plan));
    PTV_TRY(ptrs_check(c, r && z, "poisson_mg_apply: NULL input or output"));
    Stage sg(c);
    const size_t n = voxels(prm), bytes = n * sizeof(double);
    const double *dr = sg.in<double>(0, r, bytes);
    double *dz = sg.room<double>(1, bytes);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, n));
    const uint8_t *dir = dirichlet ? sg.in<uint8_t>(4, dirichlet, n) : nullptr;
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_poisson_mg_apply_dev(c, &dp, mg, dir, dr, dz, sg.s, mst));
    sg.back(z, 1, bytes);
    return sg.sync();
}

int ptv_poisson_solve_mg_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                             const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X, void *stream,
                             const ptv_mg_params *mg, ptv_pressure_stats *st, ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(poisson_solve_args(c, prm, rhs, Fx, Fy, Fz, X, g));
    PTV_TRY(mg_plan(g, mg, plan));
    PTV_TRY(needs_dirichlet(dirichlet != nullptr, "poisson_solve_mg"));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(c->ev_press[0].record(s));
    if (!rhs) {
        PTV_TRY(c->press.rhs.ensure(voxels(prm)));
        PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, prm->fluid_mask, Fx, Fy, Fz,
                                 c->press.rhs.p, s));
        rhs = c->press.rhs.p;
    }
    PTV_TRY(press_pcg(c->press, c->mg, plan, g, prm->rtol, prm->maxiter, prm->fluid_mask, dirichlet, rhs, X, s, &out,
                      mst));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_poisson_solve_mg(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                         const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X,
                         const ptv_mg_params *mg, ptv_pressure_stats *st, ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(poisson_solve_args(c, prm, rhs, Fx, Fy, Fz, X, g));
    PTV_TRY(mg_plan(g, mg, plan));
    PTV_TRY(needs_dirichlet(dirichlet != nullptr, "poisson_solve_mg"));
    Stage sg(c);
    const size_t n = voxels(prm), bytes = n * sizeof(double);
    double *F[3] = {nullptr, nullptr, nullptr};
    double *x = rhs ? sg.in<double>(0, rhs, bytes) : sg.room<double>(0, bytes);
    if (!rhs) in3(sg, 1, Fx, Fy, Fz, bytes, F);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, n));
    const uint8_t *dir = sg.in<uint8_t>(4, dirichlet, n);
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_poisson_solve_mg_dev(c, &dp, rhs ? x : nullptr, F[0], F[1], F[2], dir, x, sg.s, mg, st, mst));
    sg.back(X, 0, bytes);
    return sg.sync();
}

int ptv_pressure_recover_mg_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                                const double *W, double *P, void *stream, const ptv_mg_params *mg,
                                ptv_pressure_stats *st, ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(pressure_recover_args(c, prm, U, V, W, P, g));
    PTV_TRY(mg_plan(g, mg, plan));
    PTV_TRY(needs_dirichlet(prm->anchor != PTV_ANCHOR_NONE, "pressure_recover_mg"));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = voxels(prm);
    PTV_TRY(c->press.f.ensure(3 * n));
    PTV_TRY(c->press.rhs.ensure(n));
    PTV_TRY(c->press.dir.ensure(n));
    double *F = c->press.f.p;
    const uint8_t *M = prm->fluid_mask;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    if (mst) *mst = ptv_mg_stats{};
    PTV_TRY(c->ev_press[0].record(s));
    PTV_TRY(press_force(c->press, g, prm->mu, prm->rho, M, U, V, W, F, F + n, F + 2 * n, s, &out));
    if (out.n_fluid == 0) {  // physics.py:274-276
        PTV_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
        PTV_HIP(hipStreamSynchronize(s));
        if (st) *st = out;
        return PTV_OK;
    }
    PTV_TRY(c->ev_press[1].record(s));
    PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, M, F, F + n, F + 2 * n, c->press.rhs.p, s));
    PTV_TRY(c->ev_press[2].record(s));
    // velocity_analysis.py:304-321: np.mean(w[mask]) >= 0 has the sign of the sum
    const bool positive = prm->flow_direction == 1 || (prm->flow_direction == 0 && out.sum_w >= 0.0);
    const bool last = (prm->anchor == PTV_ANCHOR_OUTLET) == positive;
    out.anchor_plane = last ? g.nz - 1 : 0;
    PTV_TRY(press_anchor_plane(g, out.anchor_plane, M, c->press.dir.p, s));
    PTV_TRY(press_pcg(c->press, c->mg, plan, g, prm->rtol, prm->maxiter, M, c->press.dir.p, c->press.rhs.p, P, s, &out,
                      mst));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[1], c->ev_press[2]));
    out.ms_divergence = ms;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_pressure_recover_mg(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                            const double *W, double *P, const ptv_mg_params *mg, ptv_pressure_stats *st,
                            ptv_mg_stats *mst) {
    GridSpec g{};
    MgPlan plan;
    PTV_TRY(pressure_recover_args(c, prm, U, V, W, P, g));
    PTV_TRY(mg_plan(g, mg, plan));
    PTV_TRY(needs_dirichlet(prm->anchor != PTV_ANCHOR_NONE, "pressure_recover_mg"));
    Stage sg(c);
    const size_t bytes = voxels(prm) * sizeof(double);
    double *d[3];
    in3(sg, 0, U, V, W, bytes, d);
    const ptv_pressure_params dp = on_device(prm, sg.mask(prm->fluid_mask, voxels(prm)));
    double *p = sg.room<double>(3, bytes);
    PTV_TRY(sg.rc);
    PTV_TRY(ptv_pressure_recover_mg_dev(c, &dp, d[0], d[1], d[2], p, sg.s, mg, st, mst));
    sg.back(P, 3, bytes);
    return sg.sync();
}

}  // extern "C"
