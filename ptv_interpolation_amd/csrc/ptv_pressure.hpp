// ptv_pressure.hpp — host interface of the pressure recovery (ptv_pressure.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ptv_api.h"
#include "ptv_multigrid.hpp"
#include "ptv_own.hpp"

namespace ptv {

// grow-only device scratch of the pressure recovery, owned by the context
struct PressWork {
    DevBuf<double> lap;            // the three Laplacians (raw, then filled in place)
    DevBuf<uint8_t> code;          // per voxel: 0 solid, 1 bulk, 2 / 3 filled in round 1 / 2, 4 fluid not filled
    DevBuf<double> f, rhs;         // the chain's force field (three grids) and its divergence
    DevBuf<uint8_t> dir;           // the chain's anchor plane as a Dirichlet grid
    DevBuf<double> x, r, p[2], q;  // CG vectors, one dense grid each; p ping-pongs
    DevBuf<double> z;              // the preconditioned residual (press_pcg only)
    DevBuf<double> part;           // per-block partial sums (5 rows)
    DevBuf<double> state;          // CG scalar state and the force pass's sums
    PinnedBuf<double> h_state;     // pinned: 2 polling slots + 1 final copy of the state
    std::vector<Event> ev;         // call start / end, solve start, one per polling batch
};

// All pointers device memory.  The force field's sums over the fluid voxels land in st (sum_abs_f*,
// sum_w, n_fluid); F must not alias U, V, W.  Synchronises `s`.
int press_force(PressWork &wk, const GridSpec &g, double mu, double rho, const uint8_t *M, const double *U,
                const double *V, const double *W, double *Fx, double *Fy, double *Fz, hipStream_t s,
                ptv_pressure_stats *st);
// D = the force divergence at every voxel; D must not alias F.
int press_divergence(const GridSpec &g, bool inhomogeneous, const uint8_t *M, const double *Fx, const double *Fy,
                     const double *Fz, double *D, hipStream_t s);
// scipy's cg(A, b, rtol, atol=0, maxiter) on the Laplacian with the Dirichlet rows and columns
// eliminated; Dir may be NULL (no Dirichlet voxel), X may alias B.  Synchronises `s`.
int press_cg(PressWork &wk, const GridSpec &g, double rtol, int maxiter, const uint8_t *M, const uint8_t *Dir,
             const double *B, double *X, hipStream_t s, ptv_pressure_stats *st);
// scipy's cg(A, b, M=, rtol, atol=0, maxiter) on the same system with the V-cycle of ptv_multigrid.hip
// as M; Dir is required.  Stopping, outputs and st as press_cg; mst (may be NULL) receives the
// hierarchy and the V-cycle's median time.  Synchronises `s`.
int press_pcg(PressWork &wk, MgWork &mg, const MgPlan &plan, const GridSpec &g, double rtol, int maxiter,
              const uint8_t *M, const uint8_t *Dir, const double *B, double *X, hipStream_t s,
              ptv_pressure_stats *st, ptv_mg_stats *mst);
// Dir[i] = M[i] != 0 on plane z, 0 elsewhere
int press_anchor_plane(const GridSpec &g, int z, const uint8_t *M, uint8_t *Dir, hipStream_t s);

}  // namespace ptv
