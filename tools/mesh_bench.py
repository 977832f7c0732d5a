"""Times of the spline prefilter and of the mesh drag's traction pass, against scipy on the host.

Appends JSON lines to profiles/mesh_bench.jsonl (or --out):
  - the device prefilter at 256^3 and 512^3 (hipEvent time of the three passes, median of --repeats);
  - the traction pass over 1M and 10M synthetic triangles on resident 128^3 fields (hipEvent time of
    the two kernels; the triangles are a jittered lattice of small float32 triangles in one label);
  - scipy's wall time for the same three ``map_coordinates(order=3)`` calls on the host at 256^3 on
    200k points (each call filters the whole volume again, as the reference does per label).

Usage:  python tools/mesh_bench.py [--repeats 5] [--skip-host] [--out profiles/mesh_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def triangles(n, shape, rng):
    """n small float32 triangles inside the volume, (3n, 3) vertices and (n, 3) faces."""
    hi = np.array(shape, dtype=np.float64) - 2.0
    c = rng.uniform(1.0, hi, (n, 3))
    v = (c[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.jsonl"))
    args = ap.parse_args()
    import torch  # torch brings up its HIP runtime before the library does, as bench.py does

    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    rng = np.random.default_rng(0)
    lines = []
    for n in (256, 512):
        f = torch.rand((n, n, n), dtype=torch.float64, device="cuda")
        coef = torch.empty((n + 24,) * 3, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ms = [ctx.spline_prefilter_dev(n, n, n, f.data_ptr(), coef.data_ptr()) for _ in range(args.repeats + 1)][1:]
        lines.append({"what": "prefilter", "n": n, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)),
                      "repeats": args.repeats, "padded_gb": coef.numel() * 8 / 1e9})
        del f, coef
    shape = (128, 128, 128)
    fields = [rng.standard_normal(shape) for _ in range(4)]
    for n in (1_000_000, 10_000_000):
        v, fc = triangles(n, shape, rng)
        ctx.mesh_drag(fields[:3], fields[3], None, v, fc, [0, n], 1e-3, 1.0, 1.0, 1.0)  # upload, filter, warm up
        ms = [ctx.mesh_drag(None, None, None, v, fc, [0, n], 1e-3, 1.0, 1.0, 1.0, shape=shape)[1]["ms_traction"]
              for _ in range(args.repeats)]
        lines.append({"what": "traction", "triangles": n, "fields": list(shape), "ms_median": float(np.median(ms)),
                      "ms_min": float(min(ms)), "repeats": args.repeats})
    if not args.skip_host:
        from scipy import ndimage

        n = 256
        f = [rng.standard_normal((n, n, n)) for _ in range(3)]
        pts = rng.uniform(0, n - 1, (3, 200_000))
        t0 = time.perf_counter()
        for a in f:
            ndimage.map_coordinates(a, pts, order=3, mode="nearest")
        host = (time.perf_counter() - t0) * 1e3
        t = [ctx.map_coordinates(a, pts, order=3)[1] for a in f]
        lines.append({"what": "three map_coordinates(order=3), 256^3, 200k points", "host_scipy_ms": host,
                      "device_kernels_ms": float(sum(t)), "cpus": os.cpu_count()})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for line in lines:
            print(json.dumps(line))
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
