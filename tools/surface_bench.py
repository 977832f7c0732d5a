"""Times of the device marching cubes (csrc/ptv_surface.hip) on sphere packs.

Appends JSON lines to profiles/surface_bench.jsonl (or --out):
  - the triangulation of a sphere pack with 1, 64 and 1024 labels at 256^3 and 512^3 on a mask
    resident in HBM: hipEvent times of the counting passes (classify, reductions, scans) and of the
    emitting passes (emit, sorts, gathers), median and minimum of --repeats calls after one warm-up
    call (which also grows the context's buffers).  Beside them the bytes the passes must move, the
    int32 mask read in classify and again in emit plus the float32 vertices and int32 faces written,
    and the fraction of 8 TB/s that those bytes over the median time are.  The passes move more than
    that (one byte pair per lattice point written, scanned into two uint32 offsets, and the sort's
    keys and values); the figure says how far the whole stage is from one read-twice-write-once pass.
  - the wall time of ``compute_interface_drag_mesh(triangulation='device')`` at 256^3 with 64 labels
    from host arrays (uploads, three prefilters, triangulation, traction, assembly), with the device
    times the call reports.

There is no baseline: the parent commit cannot run this path without scikit-image, and
scikit-image is not available.  No threshold is set.

Usage:  python tools/surface_bench.py [--repeats 5] [--sizes 256 512] [--out profiles/surface_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def sphere_pack(torch, n, labels):
    """int32 (n, n, n) on the device: `labels` spheres on a cubic grid of cells, radius 0.4 cells."""
    per = int(np.ceil(labels ** (1.0 / 3.0) - 1e-9))
    cell = n / per
    ax = torch.arange(n, dtype=torch.float32, device="cuda")
    idx = torch.clamp((ax / cell).floor(), max=per - 1)
    off = ax - (idx + 0.5) * cell
    d2 = off[:, None, None] ** 2 + off[None, :, None] ** 2 + off[None, None, :] ** 2
    lab = (idx[:, None, None] * per + idx[None, :, None]) * per + idx[None, None, :] + 1
    mask = torch.where((d2 <= (0.4 * cell) ** 2) & (lab <= labels), lab, torch.zeros_like(lab))
    return mask.to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.jsonl"))
    args = ap.parse_args()
    import torch  # torch brings up its HIP runtime before the library does, as bench.py does

    from ptv_interpolation_amd import _lib, velocity_analysis as va

    ctx = _lib.Context.get(0)
    lines = []
    for n in args.sizes:
        for labels in (1, 64, 1024):
            mask = sphere_pack(torch, n, labels)
            torch.cuda.synchronize()
            table = np.arange(1, labels + 1, dtype=np.int32)
            runs = [ctx.marching_cubes_dev(n, n, n, mask.data_ptr(), table) for _ in range(args.repeats + 1)][1:]
            nv, nt = int(runs[0][0].sum()), int(runs[0][1].sum())
            total = [r[2]["ms_count"] + r[2]["ms_emit"] for r in runs]
            must = 2 * 4 * n ** 3 + 12 * nv + 12 * nt
            lines.append({"what": "marching cubes, sphere pack", "n": n, "labels": labels, "vertices": nv,
                          "triangles": nt, "ms_count_median": float(np.median([r[2]["ms_count"] for r in runs])),
                          "ms_emit_median": float(np.median([r[2]["ms_emit"] for r in runs])),
                          "ms_median": float(np.median(total)), "ms_min": float(min(total)), "repeats": args.repeats,
                          "bytes_must_move": must,
                          "fraction_of_8TBps": must / (float(np.median(total)) * 1e-3) / HBM_BYTES_PER_S})
            del mask
    n, labels = 256, 64
    mask = sphere_pack(torch, n, labels).cpu().numpy()
    rng = np.random.default_rng(0)
    u, v, w, p = (rng.standard_normal((n, n, n)) for _ in range(4))
    va.compute_interface_drag_mesh(u, v, w, p, 1e-3, 1.0, 1.0, 1.0, mask, triangulation='device')  # warm up
    wall = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = va.compute_interface_drag_mesh(u, v, w, p, 1e-3, 1.0, 1.0, 1.0, mask, triangulation='device')
        wall.append((time.perf_counter() - t0) * 1e3)
    lines.append({"what": "compute_interface_drag_mesh(triangulation='device'), host arrays", "n": n,
                  "labels": len(res), "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(min(wall)),
                  "repeats": args.repeats, "device_ms": va.integrate_mesh_drag.last_times})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for line in lines:
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
