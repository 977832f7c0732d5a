"""Time the GPU variational divergence cleaning on a sphere-pack grid.

The mask is ``synth.fluid_mask(G)`` (default G = 256) and the fields are the project's own IDW
interpolation of a seeded sphere-pack particle set with N(0, 1) velocities, left resident on the
device.  After one warm-up call, one solve per lambda (200, the dataset runner's, and 1e3, the
default) runs with the reference's ``rtol = 1e-8, maxiter = 2000`` and device events around every
polling batch of the CG solve; per lambda the line reports

* ``ms_per_iter``: the median over the solve's batches of (batch time / iterations in the batch);
* ``ms_solve``, ``itn``, ``info``: the whole solve;
* ``bytes_per_s`` and ``frac_of_8TBps``: the DESIGN.md §17 byte model (283 bytes per voxel and CG
  iteration over the dense grid) divided by that time, against 8 TB/s;

and once ``host_ms_per_iter_64``: scipy's ``cg`` on the assembled CSR system of the 64^3 sphere-pack
mask on this machine's CPU, per iteration (assembly not included), with
``host_ms_per_iter_extrapolated``: that figure scaled by the ratio of fluid voxels.  The scaled
figure is an extrapolation, not a measurement.

Clocks are whatever the device runs at (not pinned, not assumed); the line records the
event-timed figures only.  One JSON line goes to stdout and, with --out, is appended to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_VOXEL_ITER = 283


def host_ms_per_iter(G, iters, lam):
    from scipy.sparse.linalg import cg

    import _variational_ref as vref
    from ptv_interpolation_amd import synth

    mask = synth.fluid_mask(G)
    A = vref.csr_system(mask, 1.0, 1.0, 1.0, lam)
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    cg(A, b, rtol=0.0, atol=0.0, maxiter=3)  # warm-up
    t0 = time.perf_counter()
    cg(A, b, rtol=0.0, atol=0.0, maxiter=iters)
    dt = time.perf_counter() - t0
    return 1e3 * dt / iters, int(mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, default=500_000)
    ap.add_argument("--lambdas", type=float, nargs="*", default=[200.0, 1e3])
    ap.add_argument("--maxiter", type=int, default=2000)
    ap.add_argument("--host-grid", type=int, default=64)
    ap.add_argument("--host-iters", type=int, default=50)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from ptv_interpolation_amd import _lib, synth

    G = args.grid
    ctx = _lib.Context.get(0)
    mask = synth.fluid_mask(G)
    P, Q = synth.sphere_pack(args.particles, G, values="normal")
    ax = np.arange(G, dtype=np.float64)
    U, V, W = ctx.interp_knn(P, Q, axes=(ax, ax, ax), method=_lib.METHOD_IDW, k=8, fluid_mask=mask)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.nan_to_num(a)).to(dev) for a in (U, V, W)]
    o = [torch.empty_like(a) for a in t]
    m = torch.from_numpy(mask.view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    ptrs, optrs = [a.data_ptr() for a in t], [a.data_ptr() for a in o]
    ctx.clean_variational_dev(G, G, G, ptrs, m.data_ptr(), optrs, 1.0, 1.0, 1.0, lambda_reg=200.0, maxiter=16)  # warm-up
    solves = []
    for lam in args.lambdas:
        st = ctx.clean_variational_dev(G, G, G, ptrs, m.data_ptr(), optrs, 1.0, 1.0, 1.0, lambda_reg=lam,
                                       rtol=1e-8, maxiter=args.maxiter)
        ms_it = st["ms_iter_median"]
        bps = BYTES_PER_VOXEL_ITER * float(G) ** 3 / (ms_it * 1e-3) if ms_it > 0 else 0.0
        solves.append({"lambda_reg": lam, "itn": st["itn"], "info": st["info"], "ms_per_iter": ms_it,
                       "ms_solve": st["ms_solve"], "ms_total": st["ms_total"], "bytes_per_s": bps,
                       "frac_of_8TBps": bps / 8e12, "mean_abs_div_before": st["mean_abs_div_initial"],
                       "mean_abs_div_after": st["mean_abs_div_final"], "n_fluid": st["n_fluid"]})
    host_ms, host_fluid = host_ms_per_iter(args.host_grid, args.host_iters, 200.0)
    n_fluid = solves[0]["n_fluid"] if solves else int(mask.sum())
    line = {
        "tool": "variational_bench", "grid": G, "n_fluid": n_fluid, "rtol": 1e-8, "maxiter": args.maxiter,
        "bytes_per_voxel_iter": BYTES_PER_VOXEL_ITER, "solves": solves,
        "host_grid": args.host_grid, "host_n_fluid": host_fluid, "host_ms_per_iter_64": host_ms,
        "host_ms_per_iter_extrapolated": host_ms * n_fluid / host_fluid,
        "host_note": "extrapolation: scipy cg per-iteration time at host_grid scaled by fluid voxel count",
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
