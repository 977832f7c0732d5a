"""Golden fixtures of the reference's staircase interface drag (velocity_analysis.py:332-511) and of
compute_permeability_from_pressure (:659-697).

Imports the reference ``velocity_analysis.py`` from the directory named by ``PTV_REFERENCE_DIR`` and
runs ``compute_interface_drag(method='staircase')`` on the seeded cases of tests/_drag_ref.py.  Each
``drag_<case>.npz`` holds the case's name, a checksum of its seeded inputs (the tests rebuild them
from the seed and compare), the label mask, the labels the result is keyed by, and the reference's
13 keys per label as float64 (``values``: (labels, 13) in _drag_ref.KEYS order; float32 results
widen exactly).  ``drag_perm_<dtype>.npz`` holds the permeability of _drag_ref.make_perm_case.

Usage:  PTV_REFERENCE_DIR=<directory of the reference> python tests/golden/make_drag_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _drag_ref as dref  # noqa: E402


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("_reference_velocity_analysis",
                                                  os.path.join(ref, "velocity_analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(name, **data):
    path = os.path.join(HERE, f"drag_{name}.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {os.path.getsize(path)} bytes")


def main():
    ref = load_reference(os.environ["PTV_REFERENCE_DIR"])
    for name in dref.CASES:
        c = dref.make_case(name)
        dx, dy, dz = c["spacing"]
        res = ref.compute_interface_drag(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], dx, dy, dz,
                                         c["mask"], labels=c["labels"], method="staircase")
        keys = list(res)
        values = np.array([[np.float64(res[k][q]) for q in dref.KEYS] for k in keys], dtype=np.float64)
        values = values.reshape(len(keys), len(dref.KEYS))
        small = np.int8 if c["mask"].dtype != np.bool_ and np.abs(c["mask"]).max() < 127 else c["mask"].dtype
        save(name, case=np.array(name), checksum=np.float64(dref.checksum(c)), mask=c["mask"].astype(small),
             keys=np.array(keys), values=values)
    for dtype in (np.float64, np.float32):
        c = dref.make_perm_case(dtype)
        dx, dy, dz = c["spacing"]
        k = ref.compute_permeability_from_pressure(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], dx, dy, dz)
        save(f"perm_{np.dtype(dtype).name}", checksum=np.float64(dref.checksum(c)), permeability=np.float64(k))


if __name__ == "__main__":
    main()
