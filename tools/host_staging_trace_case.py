"""Dev tool: a fixed sequence of calls through the grid-field host layer, for comparing two library
builds operation by operation (PTV_LIB selects the build), in the manner of tools/api_trace_case.py.

Default: on one context, at 64^3, a warm-up pass and then one host call and one ``_dev`` call of each
family of tests/_host_staging.py.  Run it under
    rocprofv3 --kernel-trace --hip-trace --stats -- python tools/host_staging_trace_case.py
once per library: the kernel names with their call counts, and the call counts of hipLaunchKernel,
hipMemcpyAsync, hipMemcpy, hipMemsetAsync, hipEventRecord and hipStreamSynchronize, must not differ
(hipMalloc and hipFree may).

--held G: instead, the device memory the context holds after the host sequence clean, variational,
pressure, flow at G^3 float64 (two iterations each), from torch.cuda.mem_get_info around it.

--time G: instead, the wall time of one host call per family at G^3: median, min and max of
--repeat calls after a warm-up, the solvers at two iterations so that the copies are not drowned."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

torch.cuda.init()  # before the library opens the device
import _host_staging as hs

from ptv_interpolation_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=64)
ap.add_argument("--held", type=int, default=0, metavar="G")
ap.add_argument("--time", type=int, default=0, metavar="G")
ap.add_argument("--repeat", type=int, default=5)
a = ap.parse_args()
lib = os.environ.get("PTV_LIB", "in-tree")
ctx = _lib.Context(0)

if a.held or a.time:
    G = a.held or a.time
    d = hs.Inputs((G, G, G))
    u, v, w, p = d.f
    calls = {
        "clean": lambda: ctx.clean_divergence(u, v, w, d.mask, *hs.H, iterations=1, iter_lim=2),
        "variational": lambda: ctx.clean_variational(u, v, w, d.mask, *hs.H, lambda_reg=200.0, maxiter=2),
        "pressure": lambda: ctx.pressure_recover(u, v, w, d.mask, *hs.H, 1e-3, maxiter=2),
        "flow": lambda: ctx.flow_analysis(u, v, w, *hs.H, viscosity=1e-3, fluid_mask=d.mask),
    }
    if a.held:
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        print(f"{lib} held after clean, variational, pressure, flow at {G}^3: {(free0 - free1) / 2**20:.1f} MiB "
              f"({(free0 - free1) / (8 * G**3):.2f} float64 grids)", flush=True)
    else:
        # grains in blocks of 32 voxels: random labels would make the marching cubes' mesh the whole grid
        z, y, x = np.indices((G, G, G), sparse=True)
        d.labels = ((z // 32 + y // 32 + x // 32) % 3).astype(np.int32)
        calls.update({
            "divergence": lambda: ctx.divergence(u, v, w, d.mask, *hs.H),
            "drag": lambda: ctx.interface_drag(d.labels, u, v, w, p, 1e-3, *hs.H, hs.TABLE),
            "gradient sums": lambda: ctx.gradient_sums(p, *hs.H),
            "edt": lambda: ctx.edt(d.solid),
            "label": lambda: ctx.label(d.solid),
            "marching cubes": lambda: ctx.marching_cubes(d.labels, hs.TABLE),
            "spline prefilter": lambda: ctx.spline_prefilter(u),
        })
        for name, fn in calls.items():
            fn()
            ms = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            print(f"{lib} | {name} {G}^3 | wall ms median {np.median(ms):.2f} min {min(ms):.2f} max {max(ms):.2f}",
                  flush=True)
else:
    G = a.grid
    inputs = {dt: hs.Inputs((G, G, G), dt) for dt in (np.float32, np.float64)}
    for rounds in range(2):  # the warm-up pass, then the pass that is compared
        for name, (dtypes, fn) in hs.CASES.items():
            for on_dev in (False, True):
                fn(ctx, inputs[dtypes[-1]], on_dev)
    print(f"{lib} trace case done: {len(hs.CASES)} families, host and _dev, {G}^3", flush=True)
ctx.close()
