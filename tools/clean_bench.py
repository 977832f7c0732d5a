"""Time the GPU divergence cleaning (one outer iteration) on a sphere-pack grid.

The mask is ``synth.fluid_mask(G)`` (default G = 256) and the fields are the project's own IDW
interpolation of a seeded sphere-pack particle set with N(0, 1) velocities, left resident on the
device.  After a short warm-up call, one ``iterations=1`` cleaning runs with device events around
every polling batch of the LSQR solve; the line reports

* ``ms_per_iter``: the median over the solve's batches of (batch time / iterations in the batch);
* ``bytes_per_s`` and ``frac_of_8TBps``: the DESIGN.md §14 byte model (91 bytes per voxel and
  LSQR iteration over the dense grid) divided by that time, against 8 TB/s;
* ``host_ms_per_iter_64``: scipy's ``lsqr`` on a CSR Laplacian of the 64^3 sphere-pack mask on this
  machine's CPU, per iteration, and ``host_ms_per_iter_extrapolated``: that figure scaled by the
  ratio of fluid voxels.  The scaled figure is an extrapolation, not a measurement.

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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_PER_VOXEL_ITER = 91


def csr_laplacian(mask, dx, dy, dz):
    """The masked 7-point Laplacian as CSR (duplicates summed), for the host timing only."""
    from scipy import sparse

    n = int(mask.sum())
    idx = np.full(mask.shape, -1, dtype=np.int64)
    idx[mask] = np.arange(n)
    rows, cols, vals = [], [], []
    for axis, h in ((2, dx), (1, dy), (0, dz)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        a, b = idx[tuple(lo)], idx[tuple(hi)]
        both = (a >= 0) & (b >= 0)
        a, b = a[both], b[both]
        c = np.full(a.size, 1.0 / (h * h))
        rows += [a, b, a, b]
        cols += [b, a, a, b]
        vals += [c, c, -c, -c]
    return sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                             shape=(n, n)).tocsr()


def host_ms_per_iter(G, iters):
    from scipy.sparse.linalg import lsqr

    from ptv_interpolation_amd import synth

    mask = synth.fluid_mask(G)
    A = csr_laplacian(mask, 1.0, 1.0, 1.0)
    b = np.random.default_rng(5).standard_normal(A.shape[0])
    b -= b.mean()
    lsqr(A, b, damp=1e-8, atol=1e-10, btol=1e-10, iter_lim=3)  # warm-up
    t0 = time.perf_counter()
    res = lsqr(A, b, damp=1e-8, atol=1e-10, btol=1e-10, iter_lim=iters)
    dt = time.perf_counter() - t0
    return 1e3 * dt / max(res[2], 1), int(mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--particles", type=int, default=500_000)
    ap.add_argument("--iter-lim", type=int, default=600)
    ap.add_argument("--host-grid", type=int, default=64)
    ap.add_argument("--host-iters", type=int, default=100)
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
    ctx.clean_divergence_dev(G, G, G, ptrs, m.data_ptr(), optrs, 1.0, 1.0, 1.0, iterations=1, iter_lim=16)  # warm-up
    st = ctx.clean_divergence_dev(G, G, G, ptrs, m.data_ptr(), optrs, 1.0, 1.0, 1.0, iterations=1,
                                  iter_lim=args.iter_lim)
    ms_it = st["ms_iter_median"][0]
    bps = BYTES_PER_VOXEL_ITER * float(G) ** 3 / (ms_it * 1e-3)
    host_ms, host_fluid = host_ms_per_iter(args.host_grid, args.host_iters)
    line = {
        "tool": "clean_bench", "grid": G, "n_fluid": st["n_fluid"], "iterations": 1, "iter_lim": args.iter_lim,
        "istop": st["istop"][0], "itn": st["itn"][0], "ms_per_iter": ms_it, "ms_solve": st["ms_solve"],
        "ms_total": st["ms_total"], "bytes_per_voxel_iter": BYTES_PER_VOXEL_ITER, "bytes_per_s": bps,
        "frac_of_8TBps": bps / 8e12, "mean_abs_div_before": st["mean_abs_div"][0],
        "mean_abs_div_after": st["mean_abs_div_final"],
        "host_grid": args.host_grid, "host_n_fluid": host_fluid, "host_ms_per_iter_64": host_ms,
        "host_ms_per_iter_extrapolated": host_ms * st["n_fluid"] / host_fluid,
        "host_note": "extrapolation: scipy lsqr per-iteration time at host_grid scaled by fluid voxel count",
    }
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
