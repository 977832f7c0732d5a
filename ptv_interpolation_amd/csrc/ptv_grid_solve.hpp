// ptv_grid_solve.hpp — what the iterative dense-grid solvers share above the element groups of
// ptv_grid_vec.hpp (ptv_clean.hip, ptv_variational.hip, ptv_pressure.hip): the scalar recurrence of
// scipy's cg, the host loop that enqueues iterations and polls the stop flag, and the small host
// pieces around them (grid check, vector triples, the one- / two-wide launch, events).
//
// Stopping and polling.  A solver keeps its scalars in a device-resident array of doubles whose
// slot 0 is the stop flag; every kernel of an iteration returns at once when it is set.  The host
// enqueues kPoll iterations, copies the state to one of two pinned slots and records an event, and
// reads the copy of the batch before: the device never waits for the host, and x and itn are those
// of the iteration whose test stopped the solve.  Events of a Work struct: 0 / 1 the start and end
// of a call, 2 / 3 the start of a solve and of its first batch, 4 + b the end of batch b (the
// event after the last batch closes the solve).
#pragma once

#include "ptv_grid_vec.hpp"
#include "ptv_kernels.hpp"
#include "ptv_own.hpp"

namespace ptv {

constexpr int kPoll = 8;      // solver iterations between two polls of the stop flag
constexpr int kStopSlot = 0;  // the stop flag's slot in every solver's state

// ---- the scalar recurrence of scipy.sparse.linalg.cg (_isolve/iterative.py) ----
namespace cg {

// the first slots of a CG solver's state; a solver's own slots follow from S_CG_COUNT
enum { S_STOP = kStopSlot, S_INFO, S_ITN, S_RHO, S_RHO_PREV, S_BETA, S_ALPHA, S_RR, S_BNORM, S_THR, S_NAN, S_CG_COUNT };
// the solver phases of a scalar kernel; a solver's own phases follow from PH_CG_COUNT
enum { PH_INIT = 0, PH_TOP0, PH_TOP, PH_ALPHA, PH_END, PH_CG_COUNT };

struct CgCfg {
    double rtol;
    int maxiter;
};

// a phase that a set stop flag turns into a no-op
__device__ __forceinline__ bool in_iteration(int phase) {
    return phase == PH_TOP0 || phase == PH_TOP || phase == PH_ALPHA || phase == PH_END;
}

// One scalar step on the state, by one thread; r0 is the sum of the last pass's partials (b^2 for
// PH_INIT, r^2 for PH_TOP and PH_END, p q for PH_ALPHA; PH_TOP0 reads no sum).  scipy tests only at
// the top of an iteration: after the last one nothing is tested, and info = maxiter is returned
// even when r is 0.
__device__ __forceinline__ void cg_step(int phase, const CgCfg &cfg, double *__restrict__ st, double r0) {
    switch (phase) {
    case PH_INIT: {  // bnrm2, the threshold max(atol, rtol * bnrm2) with atol = 0, the early returns
        const double bnorm = sqrt(r0);
        for (int k = 0; k < S_CG_COUNT; ++k) st[k] = 0.0;
        st[S_RR] = r0;
        st[S_BNORM] = bnorm;
        st[S_THR] = cfg.rtol * bnorm > 0.0 ? cfg.rtol * bnorm : 0.0;
        if (bnorm == 0.0 || cfg.maxiter <= 0) {
            st[S_STOP] = 1.0;  // zeros, info = 0
        } else if (r0 != r0) {  // a NaN in b: alpha is NaN in the first step and x is NaN from then on
            st[S_NAN] = 1.0;
            st[S_INFO] = (double)cfg.maxiter;
            st[S_ITN] = (double)cfg.maxiter;
            st[S_STOP] = 1.0;
        }
        break;
    }
    case PH_TOP0:
    case PH_TOP: {  // the top of an iteration: the only convergence test, then rho and beta
        const double rr = phase == PH_TOP0 ? st[S_RR] : r0;
        st[S_RR] = rr;
        if (sqrt(rr) < st[S_THR]) {
            st[S_STOP] = 1.0;  // info = 0
            break;
        }
        st[S_RHO] = rr;
        st[S_BETA] = phase == PH_TOP0 ? 0.0 : rr / st[S_RHO_PREV];
        break;
    }
    case PH_ALPHA:
        st[S_ALPHA] = st[S_RHO] / r0;
        st[S_RHO_PREV] = st[S_RHO];
        st[S_ITN] += 1.0;  // this iteration's updates follow unconditionally
        break;
    case PH_END:  // the loop ran out: no test after the last step
        st[S_RR] = r0;
        st[S_INFO] = (double)cfg.maxiter;
        st[S_STOP] = 1.0;
        break;
    default:
        break;
    }
}

// ---- the same recurrence with a preconditioner (scipy's cg with M=) ----
// The top of an iteration splits in two around z = M r: PH_PTOP0 / PH_PTOP hold the convergence test
// on r^2 (as PH_TOP0 / PH_TOP), PH_PRHO takes rho = r z and beta.  PH_INIT, PH_ALPHA and PH_END are
// cg_step's.  A solver names the slot of its state that keeps r z as last summed.
enum { PH_PTOP0 = 64, PH_PTOP, PH_PRHO };

__device__ __forceinline__ bool pcg_in_iteration(int phase) {
    return in_iteration(phase) || phase == PH_PTOP0 || phase == PH_PTOP || phase == PH_PRHO;
}

// r0: r^2 for PH_PTOP, r z for PH_PRHO (PH_PTOP0 reads no sum); the other phases as in cg_step
__device__ __forceinline__ void pcg_step(int phase, const CgCfg &cfg, double *__restrict__ st, int rz_slot,
                                         double r0) {
    switch (phase) {
    case PH_PTOP0:
    case PH_PTOP: {
        const double rr = phase == PH_PTOP0 ? st[S_RR] : r0;
        st[S_RR] = rr;
        if (sqrt(rr) < st[S_THR]) st[S_STOP] = 1.0;  // info = 0
        break;
    }
    case PH_PRHO:
        st[rz_slot] = r0;
        st[S_RHO] = r0;
        st[S_BETA] = st[S_ITN] == 0.0 ? 0.0 : r0 / st[S_RHO_PREV];
        break;
    default:
        cg_step(phase, cfg, st, r0);
        break;
    }
}

}  // namespace cg

// ---- host ----

// three dense grids (the u, v, w parts of a vector)
struct V3 {
    double *c[3];
};
struct CV3 {
    const double *c[3];
};
inline V3 parts(double *base, size_t n) { return V3{{base, base + n, base + 2 * n}}; }
inline CV3 cparts(const double *base, size_t n) { return CV3{{base, base + n, base + 2 * n}}; }

// a pass of kernel<2> or kernel<1> over nb blocks
#define GRID_LAUNCH(kernel, vec2, nb, s, ...)                                                             \
    do {                                                                                                  \
        if (vec2) hipLaunchKernelGGL(kernel<2>, dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);          \
        else hipLaunchKernelGGL(kernel<1>, dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);               \
        PTV_HIP(hipGetLastError());                                                                       \
    } while (0)

// the dimensions of a solver's grid, checked; `who` is the solver's name in its error messages
inline int grid_dims(const char *who, int nx, int ny, int nz, GridDims &a) {
    if (nx <= 0 || ny <= 0 || nz <= 0) {
        set_error(std::string(who) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    const long long n = (long long)nx * ny * nz;
    if (n > 0x7fff0000LL) {
        set_error(std::string(who) + ": grids of 2^31 voxels or more are not supported");
        return PTV_E_ARG;
    }
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.n = (unsigned)n;
    a.plane = (unsigned)nx * (unsigned)ny;
    return PTV_OK;
}

// launch_divergence's arguments for the whole grid: both z ends are domain edges, float64
inline DivArgs full_grid_div(const GridDims &a, double dx, double dy, double dz) {
    DivArgs d{};
    d.nx = a.nx;
    d.ny = a.ny;
    d.nz = a.nz;
    d.z_begin = 0;
    d.z_end = a.nz;
    d.edge_lo = d.edge_hi = 1;
    d.dx = dx;
    d.dy = dy;
    d.dz = dz;
    return d;
}

inline int record_event(std::vector<Event> &ev, size_t k, hipStream_t s) {
    if (ev.size() <= k) ev.resize(k + 1);
    return ev[k].record(s);
}

// The iterations of a solve: `iteration(i)` enqueues iteration i (0 .. limit - 1) on s.  After
// every kPoll of them the state goes to the pinned slot `batch & 1` of h_state and event 4 + batch
// is recorded; the copy of the batch before is then awaited and its stop flag ends the loop.
// batch_iters takes the iteration count of every batch enqueued (its size is the batch count).
template <typename Iteration>
int poll_batches(hipStream_t s, const double *state, double *h_state, int state_len, std::vector<Event> &ev,
                 int limit, Iteration &&iteration, std::vector<int> &batch_iters) {
    const size_t sbytes = (size_t)state_len * sizeof(double);
    batch_iters.clear();
    bool stopped = false;
    for (int done = 0, batches = 0; done < limit && !stopped; done += kPoll, ++batches) {
        const int cnt = std::min(kPoll, limit - done);
        for (int k = 0; k < cnt; ++k) PTV_TRY(iteration(done + k));
        batch_iters.push_back(cnt);
        PTV_HIP(hipMemcpyAsync(h_state + (batches & 1) * state_len, state, sbytes, hipMemcpyDeviceToHost, s));
        PTV_TRY(record_event(ev, 4 + batches, s));
        if (batches >= 1) {  // poll one batch behind the enqueue: the device never waits for the host
            PTV_HIP(hipEventSynchronize(ev[4 + batches - 1]));
            stopped = h_state[((batches - 1) & 1) * state_len + kStopSlot] != 0.0;
        }
    }
    return PTV_OK;
}

}  // namespace ptv
