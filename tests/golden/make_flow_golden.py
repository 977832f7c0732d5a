"""Golden fixtures of the reference's flow analysis (velocity_analysis.py:10-188).

Imports the reference ``velocity_analysis.py`` from the directory given with --ref and runs
``compute_strain_rate``, ``compute_viscous_dissipation``, ``compute_vorticity``,
``compute_astarita_flow_type`` and ``compute_permeability`` the way analyze_flow.py chains them.
Each ``flow_<case>.npz`` holds the inputs (u, v, w, the mask when the case has one, the three
spacings, ``strong`` = 1 when they were passed as np.float64 scalars and 0 when as Python floats,
the Python-float viscosity), the four fields and the permeability.

Usage:  python tests/golden/make_flow_golden.py --ref <directory of the reference>
"""
import argparse
import importlib.util
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# dx, dy, dz: anisotropic, and none a float32 value: dividing a float32 by a double that float32
# holds exactly rounds the same in float32 and in float64-then-float32, so only such spacings tell
# numpy's two division rules apart
SPACING = (0.3, 1.1, 0.7)
VISCOSITY = 1.5e-3

# name: (shape, field dtype, spacings as np.float64, mask kind, what is special)
CASES = {
    "f64_py": ((9, 10, 12), np.float64, False, "random", None),
    "f64_np64": ((9, 10, 12), np.float64, True, None, None),
    "f32_py": ((9, 10, 12), np.float32, False, "random", None),
    "f32_np64": ((9, 10, 12), np.float32, True, "random", None),
    "f32_py_nomask": ((9, 10, 12), np.float32, False, None, None),
    "small_222": ((2, 2, 2), np.float64, False, None, None),
    "small_253": ((2, 5, 3), np.float32, False, "random", None),
    "small_253_np64": ((2, 5, 3), np.float32, True, "random", None),
    "all_solid": ((2, 5, 3), np.float64, False, "solid", None),
    "naninf": ((9, 10, 12), np.float64, False, "random", "naninf"),
    "int": ((9, 10, 12), np.int64, False, "random", "int"),
}


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("_reference_velocity_analysis",
                                                  os.path.join(ref, "velocity_analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(name, seed):
    shape, dtype, strong, mask_kind, special = CASES[name]
    rng = np.random.default_rng(seed)
    if special == "int":
        fields = [rng.integers(-50, 50, size=shape).astype(dtype) for _ in range(3)]
    else:
        fields = [rng.standard_normal(shape).astype(dtype) for _ in range(3)]
    if special == "naninf":
        fields[0][4, 5, 6] = np.nan
        fields[2][2, 3, 4] = np.inf
    mask = None
    if mask_kind == "random":
        mask = rng.random(shape) < 0.7
    elif mask_kind == "solid":
        mask = np.zeros(shape, dtype=bool)
    kind = np.float64 if strong else float
    return fields, mask, tuple(kind(h) for h in SPACING)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="directory that holds the reference's velocity_analysis.py")
    args = ap.parse_args()
    ref = load_reference(args.ref)
    for seed, name in enumerate(CASES):
        (u, v, w), mask, (dx, dy, dz) = make_case(name, 100 + seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the NaN / inf case
            s = ref.compute_strain_rate(u, v, w, dx, dy, dz, mask)
            d = ref.compute_viscous_dissipation(s, VISCOSITY, dx, dy, dz, mask)
            o = ref.compute_vorticity(u, v, w, dx, dy, dz, mask)
            f = ref.compute_astarita_flow_type(s, o, mask)
            k = ref.compute_permeability(u, v, w, d, VISCOSITY, dx, dy, dz, mask)
        data = dict(u=u, v=v, w=w, spacing=np.array(SPACING), strong=np.int64(CASES[name][2]),
                    viscosity=np.float64(VISCOSITY), strain_rate=s, dissipation=d, vorticity=o, flow_type=f,
                    permeability=np.asarray(k))
        if mask is not None:
            data["mask"] = mask
        path = os.path.join(HERE, f"flow_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
