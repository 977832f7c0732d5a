"""Time the GPU flow analysis (csrc/ptv_flow.hip) on fields resident on the device.

The mask is ``synth.fluid_mask_device(G)`` (the sphere pack) and the fields are seeded N(0, 1) values
made on the device, zeroed in the solid; sizes 256^3 and 512^3, float64 and float32.  Per size and
dtype the fused call runs with all four outputs and with the strain rate only; after warm-up calls
the step time is the median over the repeats of the hipEvent time around the call's kernels
(``ms_stencil``: the stencil and the closing reduction).  Per run the line reports

* ``ms``: that median, ``min_ms`` / ``max_ms`` its spread;
* ``bytes_per_voxel``: the DESIGN.md §18 model, 3 sizeof(T) + 1 + sizeof(T) x outputs;
* ``frac_of_8TBps``: model bytes / time against the 8 TB/s HBM peak (the divergence stencil's
  figure at 512^3, DESIGN.md §5, is 0.64 float64 / 0.60 float32).

A CPU leg computes the same four fields at 256^3 float64 by np.gradient on this machine's host,
written out below (``host_ms_256``, one run).  Clocks are whatever the device runs at (not pinned,
not assumed).  One JSON line goes to stdout and, with --out, is appended to a file.
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
H = (1.0e-5, 1.0e-5, 1.0e-5)
VISC = 1.0e-3


def host_ms(G):
    """The four fields by np.gradient on the host, float64, no fused pass: one timed run."""
    rng = np.random.default_rng(7)
    u, v, w = (rng.standard_normal((G, G, G)) for _ in range(3))
    dx, dy, dz = H
    t0 = time.perf_counter()
    uz, uy, ux = np.gradient(u, dz, dy, dx)
    vz, vy, vx = np.gradient(v, dz, dy, dx)
    wz, wy, wx = np.gradient(w, dz, dy, dx)
    s = np.sqrt(0.5 * ((2 * ux)**2 + (2 * vy)**2 + (2 * wz)**2) + (uy + vx)**2 + (uz + wx)**2 + (vz + wy)**2)
    o = np.sqrt((wy - vz)**2 + (uz - wx)**2 + (vx - uy)**2)
    d = VISC * s**2
    den = s + o
    f = np.zeros_like(s)
    np.divide(s - o, den, out=f, where=den > 1e-15)
    dt = time.perf_counter() - t0
    return 1e3 * dt, float(d.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-grid", type=int, default=256, help="0: skip the CPU leg")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from ptv_interpolation_amd import _lib, synth

    ctx = _lib.Context.get(0)
    dev = torch.device("cuda", 0)
    runs = []
    for G in args.grids:
        m = synth.fluid_mask_device(G, 0, G, dev)
        gen = torch.Generator(device=dev).manual_seed(synth.PARTICLE_SEED)
        base = [torch.randn((G, G, G), dtype=torch.float64, device=dev, generator=gen) * m for _ in range(3)]
        for tdt, code, size in ((torch.float64, _lib.F64, 8), (torch.float32, _lib.F32, 4)):
            f = [b.to(tdt).contiguous() for b in base]
            outs = [torch.empty((G, G, G), dtype=tdt, device=dev) for _ in range(4)]
            torch.cuda.synchronize()
            for label, ptrs in (("all_four", [o.data_ptr() for o in outs]), ("strain_only", [outs[0].data_ptr(), 0, 0, 0])):
                ms = []
                for i in range(args.warmup + args.repeats):
                    st = ctx.flow_analysis_dev(G, G, G, [t.data_ptr() for t in f], ptrs, *H, viscosity=VISC,
                                               mask_ptr=m.data_ptr(), field_dtype=code)
                    if i >= args.warmup:
                        ms.append(st["ms_stencil"])
                nout = sum(1 for p in ptrs if p)
                bpv = 3 * size + 1 + size * nout
                med = statistics.median(ms)
                runs.append({"grid": G, "dtype": "float64" if size == 8 else "float32", "outputs": label,
                             "ms": med, "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms),
                             "bytes_per_voxel": bpv, "bytes_per_s": bpv * float(G)**3 / (med * 1e-3),
                             "frac_of_8TBps": bpv * float(G)**3 / (med * 1e-3) / HBM_PEAK,
                             "n_fluid": st["n_fluid"], "mean_strain_fluid": st["sum_fluid"]["strain_rate"] / st["n_fluid"]})
            del f, outs
        del base, m
    line = {"tool": "flow_bench", "runs": runs, "hbm_peak_bytes_per_s": HBM_PEAK,
            "divergence_frac_512": {"float64": 0.64, "float32": 0.60}}
    if args.host_grid:
        line["host_grid"] = args.host_grid
        line["host_ms_256" if args.host_grid == 256 else "host_ms"], _ = host_ms(args.host_grid)
        line["host_note"] = "np.gradient on u, v, w once (9 arrays), float64, one run on this machine's CPU"
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
