"""Time the GPU distance transform and the alignment score (csrc/ptv_edt.hip) on inputs resident on
the device, through the ``_dev`` entry points.

Masks (nonzero = foreground, the voxels that get a distance), at 256^3 and 512^3:

* ``blob``: cubic blobs of 16 voxels on a coarse grid, each foreground with probability 1/2, as
  tools/drag_bench.py builds its mask;
* ``fill0.999``: independent voxels, foreground with probability 0.999 (long distances for a
  random mask: the nearest zero is some 6 voxels away);
* ``corner`` (``--corner-grid``, default 256): a single zero voxel in a corner, the worst case of
  the envelope passes' outward scan (every scan runs to the end of its axis).

A call writes both outputs (int32 d2, float64 distance).  After warm-up calls the time is the
median over the repeats of the hipEvent time around the call's kernels (x pass, y pass, z pass).
Per run the line reports

* ``ms``, ``min_ms`` / ``max_ms``;
* ``model_bytes``: what the three passes must move at least, N (1 + 4) + N (4 + 4) + N (4 + 4 + 8)
  = 29 N bytes (mask in, uint32 between passes, d2 and distance out);
* ``frac_of_8TBps``: model bytes / time against the 8 TB/s HBM peak;
* ``max_d2``.

Score runs: ``--points`` (5M) float64 points uniform over the 512^3 volume and a margin, m = 1 and
m = 64 offsets, the same timing; model bytes per offset: 24 B of coordinates and one 8 B gather per
point.

A CPU leg runs ``scipy.ndimage.distance_transform_edt`` once on the 256^3 blob mask on this
machine's host.  Clocks are whatever the device runs at.  One JSON line per case goes to stdout
and, with --out, is appended to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12
CELL = 16


def make_mask(torch, kind, G, dev, seed=11):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if kind == "blob":
        c = (G + CELL - 1) // CELL
        m = torch.rand((c, c, c), device=dev, generator=gen) < 0.5
        for ax in range(3):
            m = m.repeat_interleave(CELL, dim=ax)
        m = m[:G, :G, :G]
    elif kind == "corner":
        m = torch.ones((G, G, G), dtype=torch.bool, device=dev)
        m[0, 0, 0] = False
    else:
        m = torch.rand((G, G, G), device=dev, generator=gen) < 0.999
    return m.to(torch.uint8).contiguous()


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--corner-grid", type=int, default=256, help="0: skip the worst case")
    ap.add_argument("--points", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-grid", type=int, default=256, help="0: skip the CPU leg")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    dev = torch.device("cuda", 0)
    cases = [(kind, G) for G in args.grids for kind in ("blob", "fill0.999")]
    if args.corner_grid:
        cases.append(("corner", args.corner_grid))
    for kind, G in cases:
        n = float(G)**3
        m = make_mask(torch, kind, G, dev)
        d2 = torch.empty((G, G, G), dtype=torch.int32, device=dev)
        dist = torch.empty((G, G, G), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ms = []
        for i in range(args.warmup + args.repeats):
            st = ctx.edt_dev(G, G, G, m.data_ptr(), d2.data_ptr(), dist.data_ptr())
            if i >= args.warmup:
                ms.append(st["ms"])
        med = statistics.median(ms)
        model = 29.0 * n
        emit({"tool": "edt_bench", "pass": "edt", "mask": kind, "grid": G, "ms": med, "min_ms": min(ms),
              "max_ms": max(ms), "repeats": len(ms), "model_bytes": model, "bytes_per_s": model / (med * 1e-3),
              "frac_of_8TBps": model / (med * 1e-3) / HBM_PEAK, "max_d2": st["max_d2"],
              "foreground": float(m.to(torch.float32).mean().item())}, args.out)
        if kind == "blob" and G == args.host_grid:
            from scipy import ndimage

            host = m.cpu().numpy()
            t0 = time.perf_counter()
            ref = ndimage.distance_transform_edt(host)
            host_ms = 1e3 * (time.perf_counter() - t0)
            emit({"tool": "edt_bench", "pass": "edt_host_scipy", "mask": kind, "grid": G, "ms": host_ms, "repeats": 1,
                  "equal_to_gpu": bool(np.array_equal(ref, dist.cpu().numpy())),
                  "note": "scipy.ndimage.distance_transform_edt on this machine's CPU, one run"}, args.out)
        del m, d2, dist
    if args.points:
        G = max(args.grids)
        m = make_mask(torch, "blob", G, dev)
        dist = torch.empty((G, G, G), dtype=torch.float64, device=dev)
        ctx.edt_dev(G, G, G, m.data_ptr(), 0, dist.data_ptr())
        gen = torch.Generator(device=dev).manual_seed(5)
        pts = (torch.rand((args.points, 3), dtype=torch.float64, device=dev, generator=gen) * (G + 8.0) - 4.0).contiguous()
        rng = np.random.default_rng(9)
        for mo in (1, 64):
            off = rng.uniform(-3.0, 3.0, (mo, 3))
            torch.cuda.synchronize()
            ms = []
            for i in range(args.warmup + args.repeats):
                rec, t = ctx.align_score_dev((G, G, G), args.points, pts.data_ptr(), dist.data_ptr(), off)
                if i >= args.warmup:
                    ms.append(t)
            med = statistics.median(ms)
            model = 32.0 * args.points * mo
            emit({"tool": "edt_bench", "pass": "align_score", "grid": G, "points": args.points, "offsets": mo, "ms": med,
                  "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms), "model_bytes": model,
                  "bytes_per_s": model / (med * 1e-3), "frac_of_8TBps": model / (med * 1e-3) / HBM_PEAK,
                  "inside_first": int(rec["n_inside"][0])}, args.out)


if __name__ == "__main__":
    main()
