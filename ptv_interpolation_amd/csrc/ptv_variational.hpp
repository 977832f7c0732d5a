// ptv_variational.hpp — host interface of the variational divergence cleaning (ptv_variational.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ptv_api.h"
#include "ptv_own.hpp"

namespace ptv {

// grow-only device scratch of the CG solve, owned by the context
struct VarWork {
    DevBuf<double> x, r, p[2], q;  // CG vectors: three dense grids each (u, v, w parts); p ping-pongs
    DevBuf<double> d, div;         // d = D p; the divergence of the report
    DevBuf<double> part;           // per-block partial sums (3 rows)
    DevBuf<double> state;          // CG scalar state
    PinnedBuf<double> h_state;     // pinned: 2 polling slots + 1 final copy of the state
    std::vector<Event> ev;         // call start / end, solve start, one per polling batch
};

// scipy.sparse.linalg.cg(A, b, rtol=rtol, atol=0, maxiter=maxiter) on A = I + lambda D^T D
struct VarSolve {
    double lambda_reg, rtol;
    int maxiter;
};

// all pointers device memory; Uo, Vo, Wo may alias U, V, W.  Synchronises `s`.
int variational_run(VarWork &wk, const GridSpec &g, const VarSolve &sv, const uint8_t *M, const double *U,
                    const double *V, const double *W, double *Uo, double *Vo, double *Wo, hipStream_t s,
                    ptv_variational_stats *st);
// d = Dx xu + Dy xv + Dz xw (solid voxels written as 0)
int launch_var_divergence(const GridSpec &g, const uint8_t *M, const double *xu, const double *xv, const double *xw,
                          double *d, hipStream_t s);
// y = x + lambda D^T d on the three parts (solid voxels written as 0); `part` holds one double per block
int launch_var_adjoint(const GridSpec &g, double lambda_reg, const uint8_t *M, const double *d, const double *xu,
                       const double *xv, const double *xw, double *yu, double *yv, double *yw, DevBuf<double> &part,
                       hipStream_t s);

}  // namespace ptv
