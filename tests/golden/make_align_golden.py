"""Golden fixtures of the reference's mask alignment (auto_align.find_best_offset, auto_align.py:10-62).

Imports the reference ``auto_align.py`` from the directory named by ``PTV_REFERENCE_DIR`` and runs
``find_best_offset`` on the seeded cases of tests/_align_ref.py.  The reference imports ``tifffile``
at the top and uses it only to load mask files, so an empty stand-in module of that name is
registered first.  The objective is a closure inside ``find_best_offset``; it is recorded at the
probe offsets by running the function with ``scipy.optimize.minimize`` replaced, for that call, by
a stand-in that evaluates the closure at the probes.

Each ``align_<case>.npz`` holds the inputs (mask, points, initial offset), ``res_x`` and ``res_fun``
of the real search, the number of objective evaluations it took, the probe offsets and the
objective there.

Usage:  PTV_REFERENCE_DIR=<directory of the reference> python tests/golden/make_align_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _align_ref as aref  # noqa: E402


def load_reference(ref):
    sys.modules.setdefault("tifffile", types.ModuleType("tifffile"))
    sys.path.insert(0, ref)  # its own ``from interpolator import ...``
    spec = importlib.util.spec_from_file_location("_reference_auto_align", os.path.join(ref, "auto_align.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(os.environ["PTV_REFERENCE_DIR"])
    real_minimize = ref.minimize
    for name, make in aref.CASES.items():
        mask, pts, initial = make()
        df = pd.DataFrame(pts, columns=["x", "y", "z"])
        calls = []

        def counting(fun, x0, **kw):
            def counted(x):
                calls.append(1)
                return fun(x)
            return real_minimize(counted, x0, **kw)

        probes = []

        def probing(fun, x0, **kw):
            probes.extend(np.float64(fun(o)) for o in aref.PROBE_OFFSETS)
            return types.SimpleNamespace(x=np.asarray(x0, dtype=np.float64), fun=np.float64(0.0))

        with contextlib.redirect_stdout(io.StringIO()):
            ref.minimize = counting
            x, fun = ref.find_best_offset(df, mask, initial_offset=initial)
            ref.minimize = probing
            ref.find_best_offset(df, mask, initial_offset=initial)
            ref.minimize = real_minimize
        path = os.path.join(HERE, f"align_{name}.npz")
        np.savez_compressed(path, mask=mask, points=pts, initial=np.asarray(initial, dtype=np.float64),
                            res_x=np.asarray(x, dtype=np.float64), res_fun=np.float64(fun), nfev=np.int64(len(calls)),
                            probe_offsets=aref.PROBE_OFFSETS, probe_values=np.asarray(probes, dtype=np.float64))
        print(f"{path}: {os.path.getsize(path)} bytes, nfev {len(calls)}, x {x}, fun {fun}")


if __name__ == "__main__":
    main()
