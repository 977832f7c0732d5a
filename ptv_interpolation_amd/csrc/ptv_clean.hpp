// ptv_clean.hpp — host interface of the divergence-cleaning solver (ptv_clean.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ptv_api.h"
#include "ptv_own.hpp"

namespace ptv {

// grow-only device scratch of the solver, owned by the context
struct CleanWork {
    DevBuf<double> u, v, w, x, div;  // LSQR vectors (dense grids, solid entries 0) and the divergence
    DevBuf<double> part;             // per-block partial sums (3 rows)
    DevBuf<double> state, rep;       // LSQR scalar state; report values (flux, mean |div|)
    PinnedBuf<double> h_state;       // pinned: 2 polling slots + 1 final copy of the state, then rep
    std::vector<Event> ev;           // one per polling batch (+ call start / end)
};

// LSQR settings of one call (scipy.sparse.linalg.lsqr arguments; conlim is scipy's default 1e8)
struct CleanSolve {
    int iterations;
    double damp, atol, btol;
    int iter_lim;
};

// all pointers device memory; Uo, Vo, Wo may alias U, V, W.  Synchronises `s`.
int clean_run(CleanWork &wk, const GridSpec &g, const CleanSolve &sv, const uint8_t *M, const double *U,
              const double *V, const double *W, double *Uo, double *Vo, double *Wo, hipStream_t s,
              ptv_clean_stats *st);
// One LSQR solve of A x = rhs - mean(rhs over fluid) for a caller's device right-hand side
// (solve_poisson without a Dirichlet set, physics.py:331-340): the solver of clean_run, untouched.
// sv.iterations is not read.  X (solid voxels 0) may alias rhs.  Synchronises `s`.
struct CleanRhsResult {
    int64_t n_fluid;
    int istop, itn;
    double bnorm, rnorm, ms_solve, ms_iter_median;
};
int clean_solve_rhs(CleanWork &wk, const GridSpec &g, const CleanSolve &sv, const uint8_t *M, const double *rhs,
                    double *X, hipStream_t s, CleanRhsResult *res);
int launch_clean_correction(const GridSpec &g, const uint8_t *M, const double *U, const double *V, const double *W,
                            const double *phi, double *Uo, double *Vo, double *Wo, hipStream_t s);
int launch_clean_laplacian(const GridSpec &g, const uint8_t *M, const double *x, double *y, hipStream_t s);

}  // namespace ptv
