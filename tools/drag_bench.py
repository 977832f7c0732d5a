"""Time the GPU interface drag and the gradient sums (csrc/ptv_drag.hip) on inputs resident on the
device, through the ``_dev`` entry points.

The label mask is made of cubic blobs on a coarse grid: each coarse cell of ``cell`` voxels is
fluid with probability 1/2, else one of ``n_labels`` labels, seeded; the fields are seeded N(0, 1)
values made on the device.  Sizes 256^3 and 512^3, float64 and float32, 1, 64 and 1024 labels.
After warm-up calls the time is the median over the repeats of the hipEvent time around the call's
kernels (every pass over the mask and its closing reduction).  Per run the line reports

* ``ms``: that median, ``min_ms`` / ``max_ms`` its spread, ``passes`` = ceil(labels / 32);
* ``model_bytes``: one read of the int32 mask plus the four fields, N (4 + 4 sizeof(T)), the
  DESIGN.md §19 model of one pass (the fields are in fact only read at interface faces);
* ``frac_of_8TBps``: model bytes / time against the 8 TB/s HBM peak;
* ``faces``: the faces counted over all labels.

``gradient_sums`` runs report the same for the one-field pass, model N sizeof(T).

A CPU leg runs the numpy restatement of the reference's loop (tests/_drag_ref.py ``records``, not the
reference itself) at ``--host-grid`` with 1 and 8 labels on this machine's host, one run each.
Clocks are whatever the device runs at.  One JSON line goes to stdout and, with --out, is appended
to a file.
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
H = (1.0e-5, 1.3e-5, 0.9e-5)
VISC = 1.0e-3
CELL = 16  # blob edge in voxels


def blob_mask(torch, G, n_labels, dev, seed=11):
    gen = torch.Generator(device=dev).manual_seed(seed)
    c = (G + CELL - 1) // CELL
    lab = torch.randint(1, n_labels + 1, (c, c, c), device=dev, generator=gen, dtype=torch.int32)
    lab = lab * (torch.rand((c, c, c), device=dev, generator=gen) < 0.5)
    for ax in range(3):
        lab = lab.repeat_interleave(CELL, dim=ax)
    return lab[:G, :G, :G].to(torch.int32).contiguous()


def host_ms(G, n_labels):
    """The restatement's per-label loop on the host (float64): one timed run."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _drag_ref as dref

    rng = np.random.default_rng(7)
    u, v, w, p = (rng.standard_normal((G, G, G)) for _ in range(4))
    c = (G + CELL - 1) // CELL
    lab = rng.integers(1, n_labels + 1, size=(c, c, c)) * (rng.random((c, c, c)) < 0.5)
    for ax in range(3):
        lab = np.repeat(lab, CELL, axis=ax)
    mask = np.ascontiguousarray(lab[:G, :G, :G])
    t0 = time.perf_counter()
    rec = dref.records(u, v, w, p, VISC, *H, mask, list(range(1, n_labels + 1)))
    return 1e3 * (time.perf_counter() - t0), int(rec["count"].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--labels", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-grid", type=int, default=96, help="0: skip the CPU leg")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    dev = torch.device("cuda", 0)
    runs = []
    for G in args.grids:
        n = float(G)**3
        gen = torch.Generator(device=dev).manual_seed(3)
        base = [torch.randn((G, G, G), dtype=torch.float64, device=dev, generator=gen) for _ in range(4)]
        for tdt, code, size in ((torch.float64, _lib.F64, 8), (torch.float32, _lib.F32, 4)):
            f = [b.to(tdt).contiguous() for b in base]
            name = "float64" if size == 8 else "float32"
            for nl in args.labels:
                m = blob_mask(torch, G, nl, dev)
                labels = np.arange(1, nl + 1)
                torch.cuda.synchronize()
                ms = []
                for i in range(args.warmup + args.repeats):
                    rec, t = ctx.interface_drag_dev(G, G, G, m.data_ptr(), [a.data_ptr() for a in f[:3]],
                                                    f[3].data_ptr(), VISC, *H, labels, field_dtype=code)
                    if i >= args.warmup:
                        ms.append(t)
                med = statistics.median(ms)
                model = n * (4 + 4 * size)
                runs.append({"pass": "interface_drag", "grid": G, "dtype": name, "labels": nl,
                             "passes": -(-nl // 32), "ms": med, "min_ms": min(ms), "max_ms": max(ms),
                             "repeats": len(ms), "model_bytes": model, "bytes_per_s": model / (med * 1e-3),
                             "frac_of_8TBps": model / (med * 1e-3) / HBM_PEAK, "faces": int(rec["count"].sum())})
                del m
            ms = []
            for i in range(args.warmup + args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sums = ctx.gradient_sums_dev(G, G, G, f[3].data_ptr(), *H, field_dtype=code)  # synchronises
                if i >= args.warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
            med = statistics.median(ms)
            runs.append({"pass": "gradient_sums", "grid": G, "dtype": name, "ms": med, "min_ms": min(ms),
                         "max_ms": max(ms), "repeats": len(ms), "timer": "host clock around the synchronising call",
                         "model_bytes": n * size, "bytes_per_s": n * size / (med * 1e-3),
                         "frac_of_8TBps": n * size / (med * 1e-3) / HBM_PEAK, "sums": sums})
            del f
        del base
    line = {"tool": "drag_bench", "runs": runs, "hbm_peak_bytes_per_s": HBM_PEAK, "blob_cell": CELL}
    if args.host_grid:
        line["host_grid"] = args.host_grid
        line["host_ms"] = {str(nl): host_ms(args.host_grid, nl)[0] for nl in (1, 8)}
        line["host_note"] = ("tests/_drag_ref.py records() (the numpy restatement of the reference's loop, not the "
                             "reference), float64, one run on this machine's CPU")
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
