"""Times of the device component labelling (csrc/ptv_label.hip) against scipy.ndimage.label.

Appends JSON lines to profiles/label_bench.jsonl (or --out): per volume (256^3, 512^3), mask (the sphere
pack of tools/surface_bench.py with 1024 spheres; a random half-filled mask) and structure (6 and 26
neighbours) the hipEvent times of the two halves of ``ptv_label_dev`` on a uint8 mask resident in HBM,
tile-local labelling plus border merge and flatten plus scan plus numbering, as the median and the
minimum of --repeats calls after one warm-up call (which also grows the context's buffers), with
``num_features``.  Beside them scipy's host time on the same mask (one call; the labels are compared),
the bytes a labelling must move at least (the uint8 mask read, the int32 labels written: 5 per voxel),
the bytes the four passes move by their own count (about 35 per voxel without the unions' walks, DESIGN.md
section 24) and the fraction of 8 TB/s that each is over the median time.  No threshold is set.

Usage:  python tools/label_bench.py [--repeats 5] [--sizes 256 512] [--out profiles/label_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8e12
MUST_BYTES_PER_VOXEL = 5     # mask read, labels written
PASSES_BYTES_PER_VOXEL = 35  # tile 1 + 4, borders 4, flatten 4 + 4 + 1, scan 1 + 4, numbering 4 + 4 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_bench.jsonl"))
    args = ap.parse_args()
    import torch  # torch brings up its HIP runtime before the library does, as bench.py does
    from scipy import ndimage

    from surface_bench import sphere_pack

    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    lines = []
    for n in args.sizes:
        gen = torch.Generator(device="cuda").manual_seed(n)
        masks = {"sphere pack, 1024 spheres": (sphere_pack(torch, n, 1024) != 0).to(torch.uint8).contiguous(),
                 "random, half filled": (torch.rand((n, n, n), device="cuda", generator=gen) < 0.5).to(torch.uint8)}
        labels = torch.empty((n, n, n), dtype=torch.int32, device="cuda")
        for name, mask in masks.items():
            host = mask.cpu().numpy()
            for conn, rank in ((6, 1), (26, 3)):
                torch.cuda.synchronize()
                runs = [ctx.label_dev(n, n, n, mask.data_ptr(), labels.data_ptr(), conn)
                        for _ in range(args.repeats + 1)][1:]
                total = [r["ms_merge"] + r["ms_number"] for r in runs]
                t0 = time.perf_counter()
                want, num = ndimage.label(host, ndimage.generate_binary_structure(3, rank))
                scipy_ms = (time.perf_counter() - t0) * 1e3
                med = float(np.median(total))
                lines.append({"what": "label, " + name, "n": n, "neighbours": conn,
                              "num_features": runs[0]["n_components"], "n_foreground": runs[0]["n_foreground"],
                              "equals_scipy": bool(num == runs[0]["n_components"] and
                                                   np.array_equal(labels.cpu().numpy(), want)),
                              "ms_merge_median": float(np.median([r["ms_merge"] for r in runs])),
                              "ms_number_median": float(np.median([r["ms_number"] for r in runs])),
                              "ms_median": med, "ms_min": float(min(total)), "repeats": args.repeats,
                              "scipy_host_ms": scipy_ms, "speedup_over_scipy": scipy_ms / med,
                              "bytes_must_move": MUST_BYTES_PER_VOXEL * n ** 3,
                              "fraction_of_8TBps": MUST_BYTES_PER_VOXEL * n ** 3 / (med * 1e-3) / HBM_BYTES_PER_S,
                              "bytes_passes": PASSES_BYTES_PER_VOXEL * n ** 3,
                              "passes_fraction_of_8TBps": PASSES_BYTES_PER_VOXEL * n ** 3 / (med * 1e-3) / HBM_BYTES_PER_S})
                del want
        del masks, labels
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for line in lines:
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
