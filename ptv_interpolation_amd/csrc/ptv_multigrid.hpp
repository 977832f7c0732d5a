// ptv_multigrid.hpp — host interface of the multigrid preconditioner of the anchored pressure
// solve (ptv_multigrid.hip): the level table, the device workspace, setup and one V-cycle.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ptv_api.h"
#include "ptv_own.hpp"

namespace ptv {

constexpr int kMgMaxLevels = PTV_MG_MAX_LEVELS;
constexpr unsigned kMgTailCells = 4096;          // a level of at most this many cells runs in the fused tail
constexpr size_t kMgTailLdsBytes = 152 * 1024;   // what the tail's vectors may take of the CU's 160 KiB

// one level: the grid, and where its arrays start (in doubles) in MgWork::w and MgWork::vec
struct MgLevel {
    int nx, ny, nz;
    unsigned n, plane;
    size_t w;        // 4 doubles per cell (+x, +y, +z face weights, extra diagonal); unused on level 0
    size_t z, r, t;  // the level's iterate, right-hand side and sweep scratch; unused on level 0
};

// the hierarchy of a grid under a parameter set; host only, no device call
struct MgPlan {
    int levels = 0;
    int tail = 0;  // the first level of the fused tail (levels - 1 when only the coarsest is in it)
    int nu = 2, coarse_sweeps = 16;
    double omega = 2.0 / 3.0;
    double ih2[3] = {0, 0, 0};
    MgLevel lv[kMgMaxLevels];
    size_t w_len = 0, vec_len = 0;  // doubles of the two workspaces
    size_t tail_lds = 0;            // bytes of the tail launch's LDS
};

struct MgWork {
    DevBuf<double> w;         // the coarse operators
    DevBuf<double> vec;       // the coarse vectors
    DevBuf<double> t0;        // level 0's sweep scratch when the caller brings none
    DevBuf<unsigned> counts;  // per level: cells with a non-zero diagonal
    PinnedBuf<unsigned> h_counts;
    std::vector<Event> ev;    // 0 / 1 around the setup, 2 / 3 around a timed V-cycle, 4 + 2k / 5 + 2k in a solve
};

// ptv_mg_params with the defaults filled in, checked; then the level table of the grid
int mg_plan(const GridSpec &g, const ptv_mg_params *prm, MgPlan &plan);
// the coarse operators and the per-level counts, all on the device; does not synchronise
int mg_setup(MgWork &wk, const MgPlan &plan, const uint8_t *M, const uint8_t *Dir, hipStream_t s);
// Z = M R on the grid (Z is 0 at every voxel that is not active).  T0: a grid of scratch, or NULL
// (the workspace's own).  st: a solver's state whose slot 0 is the stop flag, or NULL.  Z, R and T0
// must not alias.  Does not synchronise.
int mg_vcycle(MgWork &wk, const MgPlan &plan, const uint8_t *M, const uint8_t *Dir, const double *st,
              const double *R, double *Z, double *T0, hipStream_t s);
// levels, cells, counts and ms_setup into `out` (after the stream was synchronised)
int mg_fill_stats(MgWork &wk, const MgPlan &plan, ptv_mg_stats *out);

}  // namespace ptv
