"""Time the GPU pressure recovery on a sphere-pack grid.

The mask is ``synth.fluid_mask(G)`` (default G = 256) and the fields are the project's own IDW
interpolation of a seeded sphere-pack particle set with N(0, 1) velocities plus a unit mean flow
along z, left resident on the device.  After one warm-up call (16 iterations), one whole chain runs
with the reference's ``rtol = 1e-10, maxiter = 3000`` (outlet anchor, zero-neumann walls) and device
events around every polling batch of the CG solve.  The line reports

* ``ms_per_iter``: the median over the solve's batches of (batch time / iterations in the batch);
* ``itn``, ``info``: the solve (``info`` = maxiter: the iterations ran out);
* ``bytes_per_s`` and ``frac_of_8TBps``: the DESIGN.md §21 byte model (82 bytes per voxel and CG
  iteration over the dense grid, + 2 for the Dirichlet grid) divided by that time, against 8 TB/s;
* ``ms_force``, ``ms_divergence``: the force-field passes and the divergence pass;
* ``ms_total``: the whole call on the device;

and once ``host_ms_per_iter_64``: scipy's ``cg`` on the assembled CSR system of the 64^3 sphere-pack
mask on this machine's CPU, per iteration (assembly not included), with
``host_ms_per_iter_extrapolated``: that figure scaled by the ratio of fluid voxels.  The scaled
figure is an extrapolation, not a measurement.

Clocks are whatever the device runs at (not pinned, not assumed).  One JSON line goes to stdout
and, with --out, is appended to a file.
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

BYTES_PER_VOXEL_ITER = 84  # 82 + one Dirichlet byte in each of the two passes


def host_ms_per_iter(G, iters):
    from scipy.sparse.linalg import cg

    import _pressure_ref as pref
    from ptv_interpolation_amd import synth

    mask = synth.fluid_mask(G)
    d = pref.dirichlet_grid(mask, G - 1)
    A = pref.laplacian_matrix(mask, 1.0, 1.0, 1.0, d, symmetric=True)
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    b[d[mask]] = 0.0
    cg(A, b, rtol=0.0, atol=0.0, maxiter=3)  # warm-up
    t0 = time.perf_counter()
    cg(A, b, rtol=0.0, atol=0.0, maxiter=iters)
    dt = time.perf_counter() - t0
    return 1e3 * dt / iters, int(mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, default=500_000)
    ap.add_argument("--maxiter", type=int, default=3000)
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
    t[2] += 1.0
    p = torch.empty_like(t[0])
    m = torch.from_numpy(mask.view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    ptrs = [a.data_ptr() for a in t]
    call = lambda maxiter: ctx.pressure_recover_dev(G, G, G, ptrs, m.data_ptr(), p.data_ptr(), 1.0, 1.0, 1.0, 1e-3,  # noqa: E731
                                                    rtol=1e-10, maxiter=maxiter)
    call(16)  # warm-up
    st = call(args.maxiter)
    ms_it = st["ms_iter_median"]
    bps = BYTES_PER_VOXEL_ITER * float(G) ** 3 / (ms_it * 1e-3) if ms_it > 0 else 0.0
    host_ms, host_fluid = host_ms_per_iter(args.host_grid, args.host_iters)
    line = {
        "tool": "pressure_bench", "grid": G, "n_fluid": st["n_fluid"], "n_dirichlet": st["n_dirichlet"],
        "rtol": 1e-10, "maxiter": args.maxiter, "itn": st["itn"], "info": st["info"],
        "ended_on_maxiter": st["info"] != 0, "rnorm_over_bnorm": st["rnorm"] / st["bnorm"] if st["bnorm"] else 0.0,
        "bytes_per_voxel_iter": BYTES_PER_VOXEL_ITER, "ms_per_iter": ms_it, "bytes_per_s": bps,
        "frac_of_8TBps": bps / 8e12, "ms_force": st["ms_force"], "ms_divergence": st["ms_divergence"],
        "ms_solve": st["ms_solve"], "ms_total": st["ms_total"],
        "host_grid": args.host_grid, "host_n_fluid": host_fluid, "host_ms_per_iter_64": host_ms,
        "host_ms_per_iter_extrapolated": host_ms * st["n_fluid"] / host_fluid,
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
