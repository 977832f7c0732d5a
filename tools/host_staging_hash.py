"""Dev tool: SHA-256 of every output array and the untimed stats of the grid-field families that
tools/grid_solver_hash.py does not cover, through the host and the ``_dev`` entry points, for
bit-identity A/B of library builds (PTV_LIB selects the build).

    PTV_LIB=ab/libptv_base.so python tools/host_staging_hash.py > base.txt
    python tools/host_staging_hash.py > new.txt
    python tools/grid_solver_hash.py --join base.txt new.txt

One line per call, in grid_solver_hash.py's format: ``case | entry point | sha256 | stats``.  The
cases are those of tests/_host_staging.py: divergence, the solvers, flow analysis and flow derived,
interface drag, gradient sums, edt, align score, label, marching cubes, spline prefilter and
map_coordinates at (5, 4, 2) and (7, 9, 13), float32 and float64 where the entry point takes both.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from grid_solver_hash import fmt  # noqa: E402


def flat(st):
    return " ".join(f"{k}={fmt(v) if not isinstance(v, dict) else '{' + flat(v) + '}'}" for k, v in st.items())


def main():
    import torch

    torch.cuda.init()  # before the library opens the device, as in tools/*_bench.py
    import _host_staging as hs
    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    for shape in hs.SHAPES:
        for name, (dtypes, fn) in hs.CASES.items():
            for dt in dtypes:
                d = hs.Inputs(shape, dt)
                for on_dev in (False, True):
                    case, entry = f"{shape} {np.dtype(dt).name}", name + ("_dev" if on_dev else "")
                    try:
                        arrays, st = fn(ctx, d, on_dev)
                    except (_lib.PtvError, ValueError) as e:
                        print(f"{case} | {entry} | error | {e}", flush=True)
                        continue
                    h = hashlib.sha256()
                    for a in arrays:
                        h.update(np.ascontiguousarray(a).tobytes())
                    print(f"{case} | {entry} | {h.hexdigest()} | {flat(hs.untimed(st))}", flush=True)


if __name__ == "__main__":
    main()
