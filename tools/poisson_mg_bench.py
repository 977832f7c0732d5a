"""Time the anchored pressure Poisson solve with and without the multigrid preconditioner.

The system is tools/pressure_bench.py's: the mask is ``synth.fluid_mask(G)`` (default G = 256), the
right-hand side the force divergence of the project's own IDW interpolation of a seeded sphere-pack
particle set (N(0, 1) velocities plus a unit mean flow along z), the Dirichlet set the fluid voxels
of the last z plane.  Everything stays resident on the device and both solvers run through their
``_dev`` entry points in the same process, plain CG first: the baseline is measured next to the
preconditioned solve, not remembered.

Per solver: one warm-up call (16 iterations), then ``--repeats`` whole solves with the reference's
``rtol = 1e-10, maxiter = 3000``.  One JSON line each (stdout, and appended to ``--out``) with

* ``itn``, ``info`` (identical in every repeat: the sums are in a fixed order);
* ``ms_per_iter``: the median over the polling batches of (batch time / iterations), of the median
  repeat; ``ms_solve``: the median over the repeats of the solve's device time (the multigrid setup
  is inside it), with ``ms_solve_all`` the single values;
* multigrid only: ``ms_vcycle`` (median of the timed V-cycles), ``ms_setup``, the hierarchy;
* ``true_rel_residual``: ``|b - A x| / |b|`` over the active voxels, recomputed on the device by
  torch in a separate pass after the solve.

Times are hipEvent times of the solver's own stream.  Clocks are whatever the device runs at (not
pinned, not assumed); the two solvers alternate in one process so that they see the same state.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def true_residual(torch, x, b, fluid, act, h):
    """|b - A x| / |b| on the active voxels; x is 0 at every other voxel."""
    acc = torch.zeros_like(x)
    for axis, hh in ((2, h[0]), (1, h[1]), (0, h[2])):
        ih2 = 1.0 / (hh * hh)
        n = x.shape[axis]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis] = slice(0, n - 1)
        hi[axis] = slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        both = (fluid[lo] & fluid[hi]).to(x.dtype)
        diff = (x[hi] - x[lo]) * ih2 * both
        acc[lo] += diff
        acc[hi] -= diff
    res = torch.where(act, b - acc, torch.zeros_like(b))
    bb = torch.where(act, b, torch.zeros_like(b))
    return float(torch.linalg.vector_norm(res) / torch.linalg.vector_norm(bb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, default=500_000)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nu", type=int, default=0)
    ap.add_argument("--coarse-sweeps", type=int, default=0)
    ap.add_argument("--omega", type=float, default=0.0)
    ap.add_argument("--max-levels", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from ptv_interpolation_amd import _lib, synth

    G = args.grid
    h = (1.0, 1.0, 1.0)
    ctx = _lib.Context.get(0)
    mask = synth.fluid_mask(G)
    P, Q = synth.sphere_pack(args.particles, G, values="normal")
    ax = np.arange(G, dtype=np.float64)
    U, V, W = ctx.interp_knn(P, Q, axes=(ax, ax, ax), method=_lib.METHOD_IDW, k=8, fluid_mask=mask)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.nan_to_num(a)).to(dev) for a in (U, V, W)]
    t[2] += 1.0
    m = torch.from_numpy(mask.view(np.uint8)).to(dev)
    f = [torch.empty_like(t[0]) for _ in range(3)]
    b = torch.empty_like(t[0])
    dirichlet = torch.zeros_like(m)
    dirichlet[G - 1] = m[G - 1]
    torch.cuda.synchronize()
    ctx.force_field_dev(G, G, G, [a.data_ptr() for a in t], m.data_ptr(), [a.data_ptr() for a in f], *h, 1e-3)
    ctx.force_divergence_dev(G, G, G, [a.data_ptr() for a in f], m.data_ptr(), b.data_ptr(), *h)
    torch.cuda.synchronize()
    del t, f
    fluid = m != 0
    act = fluid & (dirichlet == 0)
    x = torch.empty_like(b)
    mg = {k: v for k, v in (("nu", args.nu), ("coarse_sweeps", args.coarse_sweeps), ("omega", args.omega),
                            ("max_levels", args.max_levels)) if v}

    def plain(maxiter):
        return ctx.poisson_solve_dev(G, G, G, m.data_ptr(), x.data_ptr(), *h, rhs_ptr=b.data_ptr(),
                                     dirichlet_ptr=dirichlet.data_ptr(), rtol=1e-10, maxiter=maxiter)

    def precond(maxiter):
        return ctx.poisson_solve_mg_dev(G, G, G, m.data_ptr(), x.data_ptr(), *h, rhs_ptr=b.data_ptr(),
                                        dirichlet_ptr=dirichlet.data_ptr(), multigrid=mg, rtol=1e-10, maxiter=maxiter)

    runs = {"cg": [], "mg_pcg": []}
    resid = {}
    plain(16)
    precond(16)
    for _ in range(args.repeats):  # alternate, so that neither solver owns the warmer half of the run
        for name, call in (("cg", plain), ("mg_pcg", precond)):
            st = call(args.maxiter)
            torch.cuda.synchronize()
            runs[name].append(st)
            resid[name] = true_residual(torch, x, b, fluid, act, h)
    for name in ("cg", "mg_pcg"):
        sts = sorted(runs[name], key=lambda s: s["ms_solve"])
        st = sts[len(sts) // 2]
        assert len({(s["itn"], s["info"]) for s in sts}) == 1
        line = {"tool": "poisson_mg_bench", "solver": name, "grid": G, "n_fluid": st["n_fluid"],
                "n_dirichlet": st["n_dirichlet"], "rtol": 1e-10, "maxiter": args.maxiter, "repeats": args.repeats,
                "itn": st["itn"], "info": st["info"], "ms_per_iter": st["ms_iter_median"], "ms_solve": st["ms_solve"],
                "ms_solve_all": [s["ms_solve"] for s in runs[name]],
                "rnorm_over_bnorm": st["rnorm"] / st["bnorm"] if st["bnorm"] else 0.0,
                "true_rel_residual": resid[name]}
        if name == "mg_pcg":
            g = st["multigrid"]
            line.update({"ms_vcycle": g["ms_vcycle_median"], "ms_setup": g["ms_setup"], "levels": g["levels"],
                         "tail_level": g["tail_level"], "cells": g["cells"], "active": g["active"],
                         "nu": args.nu or 2, "coarse_sweeps": args.coarse_sweeps or 16, "omega": args.omega or 2.0 / 3.0})
        text = json.dumps(line)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(text + "\n")


if __name__ == "__main__":
    main()
