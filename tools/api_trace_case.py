"""Dev tool: a fixed sequence of calls through the host layer, for comparing two library builds
operation by operation (PTV_LIB selects the build).

Default: on one context and device-resident inputs, a 64^3 grid with 40k sphere-pack particles:
a warm-up (whole grid k = 8, slab_halo slab, RBF k = 20, filter k = 25), then each call once:
whole grid, the slab with slab_halo, the slab under FLAG_SLAB_CULL_AUTO three times (cold, warm,
speculative), RBF k = 20, the filter at k = 25.  Run it under
    rocprofv3 --kernel-trace --hip-trace --stats -- python tools/api_trace_case.py
once per library; the kernel names with their call counts, and the call counts of
hipStreamSynchronize, hipMemcpyAsync, hipMemsetAsync and hipEventRecord, must not differ.

--time-auto N: instead, N speculative FLAG_SLAB_CULL_AUTO calls of one slab (--grid 512
--particles 5000000: the call where the host path is the larger share of the wall time); prints
the median and spread of the wall time per call and of the device time (cull + bin + lattice +
k-NN) from the call's own events."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ptv_interpolation_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=64)
ap.add_argument("--particles", type=int, default=40_000)
ap.add_argument("--time-auto", type=int, default=0, metavar="N")
a = ap.parse_args()

G, N = a.grid, a.particles
P, Q = synth.sphere_pack(N, G, values="normal")
cols = [torch.from_numpy(np.ascontiguousarray(P[:, i])).cuda() for i in range(3)] + \
       [torch.from_numpy(np.ascontiguousarray(Q[:, i])).cuda() for i in range(3)]
ptrs = [c.data_ptr() for c in cols]
axes = [torch.linspace(0, G - 1, G, dtype=torch.float64, device="cuda") for _ in range(3)]
aptrs = [x.data_ptr() for x in axes]
slab = (G // 4, G // 4 + G // 2)
out = [torch.empty((G, G, G), dtype=torch.float64, device="cuda") for _ in range(3)]
optrs = [o.data_ptr() for o in out]
keep = torch.empty(N, dtype=torch.uint8, device="cuda")
kth = torch.empty(N, dtype=torch.float64, device="cuda")
ctx = _lib.Context(0)
lib = os.environ.get("PTV_LIB", "in-tree")


def knn(**kw):
    st = ctx.interp_knn_dev(N, ptrs, G, G, G, axes_ptrs=aptrs, out_ptrs=optrs, k=8, **kw)
    torch.cuda.synchronize()
    return st


def others():
    ctx.interp_rbf_dev(N, ptrs, G, G, G, axes_ptrs=aptrs, out_ptrs=optrs, k=20)
    ctx.filter_outliers_knn_dev(N, ptrs, keep.data_ptr(), kth.data_ptr(), k=25)
    torch.cuda.synchronize()


if a.time_auto:
    for _ in range(3):  # cold (builds the map), warm (proves it), speculative
        knn(z_range=slab, flags=_lib.FLAG_SLAB_CULL_AUTO)
    wall, dev = [], []
    for _ in range(a.time_auto):
        t0 = time.perf_counter()
        knn(z_range=slab, flags=_lib.FLAG_SLAB_CULL_AUTO)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.last_stats()
        assert st["halo_required"] == 0.0 and st["n_binned"] < N  # the culled, proven path
        dev.append(st["ms_cull"] + st["ms_bin"] + st["ms_lattice"] + st["ms_knn"])
    w, d = np.sort(wall), np.sort(dev)
    print(f"{lib} auto warm {G}^3 / {N}: wall ms median {np.median(w):.3f} min {w[0]:.3f} max {w[-1]:.3f} | "
          f"device ms median {np.median(d):.3f} min {d[0]:.3f} max {d[-1]:.3f} | binned {st['n_binned']}", flush=True)
else:
    knn()
    knn(z_range=slab, slab_halo=float(G))
    others()
    knn()
    knn(z_range=slab, slab_halo=float(G))
    binned = [knn(z_range=slab, flags=_lib.FLAG_SLAB_CULL_AUTO)["n_binned"] for _ in range(3)]
    others()
    print(f"{lib} trace case done: binned by the three auto calls {binned}", flush=True)
ctx.close()
