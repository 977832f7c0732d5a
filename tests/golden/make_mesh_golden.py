"""Golden fixtures of the reference's mesh interface drag (velocity_analysis.py:513-657) and of
scipy's spline sampling under it.

Imports the reference ``velocity_analysis.py`` and runs ``compute_interface_drag_mesh`` per case.
scikit-image is not needed: a stub ``skimage.measure`` is put into ``sys.modules`` whose
``marching_cubes`` hands out the case's prepared ``(verts, faces, normals, values)`` call by call (and
raises ``RuntimeError`` for a label without a surface, which the reference skips).  Everything the
reference does from the mesh onward (:547-655) runs as it is.

Each ``mesh_<case>.npz`` holds the inputs (fields, spacings, viscosity, volume, background mask, the
label mask handed to the reference, per given label ``verts_<i>`` / ``faces_<i>``), the reference's
result (``out_labels``, ``keys``, ``values``) and, per label and each of the 21 sums, the long-double
value of tests/_mesh_ref.py (``exact_hi + exact_lo``), ``gap = |reference - exact|`` and
``scale = sum |term|``.  Each ``spline_<case>.npz`` holds a field, scipy's padded coefficients,
coordinates, scipy's order-0/1/3 samples and ``s1_diff`` / ``s3_diff`` = the long-double sample minus
scipy's (float32 holds a difference of 1e-15 to 1e-22; the gap is its magnitude);
``spline_<case>_coef.npz`` holds scipy's padded coefficients and ``coef_diff`` likewise, in a file of
its own to stay under the per-file size limit.

Usage:  python tests/golden/make_mesh_golden.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _mesh_ref as mref  # noqa: E402
from make_clean_golden import PART_BYTES  # noqa: E402

VISC = 1.5e-3
H = (0.7, 1.1, 0.3)  # dx, dy, dz


def _zero_area_sheet():
    v, f = mref.sheet_mesh((2.5, 2.0, 2.0), (0.0, 1.0, 0.0), (0.25, 0.0, 1.0), 3, 3)
    f = f.copy()
    f[4] = (f[4][0], f[4][1], f[4][1])  # a repeated vertex: area 0
    return v, f


def _cases():
    """name -> dict(shape, seed, meshes {label: (verts, faces)}, and what differs from the defaults)."""
    one = (np.array([[2.0, 2.5, 3.0], [2.5, 4.0, 3.5], [3.5, 3.0, 5.0]], dtype=np.float32),
           np.array([[0, 1, 2]], dtype=np.int32))
    none = (np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32))
    small = mref.sheet_mesh((4.5, 1.0, 1.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 4, 5)
    return {
        # two labels, distinct spacings, a background mask that splits the triangles
        "two": dict(shape=(16, 14, 18), seed=1, background="half",
                    meshes={1: mref.sphere_mesh((6.0, 6.5, 6.0), 4.25, 2), 2: mref.sphere_mesh((11.5, 8.0, 9.5), 2.5, 1)}),
        "odd": dict(shape=(7, 9, 33), seed=2, background="half",
                    meshes={3: mref.sheet_mesh((1.5, 0.5, 1.0), (0.5, 0.5, 0.0), (0.0, 0.125, 1.5), 7, 19),
                            5: mref.sphere_mesh((3.0, 4.0, 27.0), 2.25, 1)}),
        "nop": dict(shape=(9, 8, 10), seed=3, pressure=False, meshes={1: mref.sphere_mesh((4.0, 3.5, 4.5), 2.75, 1)}),
        "vol": dict(shape=(9, 8, 10), seed=4, volume=2.5e-3, meshes={1: mref.sphere_mesh((4.0, 3.5, 4.5), 2.75, 1)}),
        # vertices exactly on 0 and n - 1: the +-0.25 samples leave the volume
        "edge": dict(shape=(9, 11, 13), seed=5, background="half",
                     meshes={1: mref.sphere_mesh((4.0, 5.0, 6.0), (4.0, 5.0, 6.0), 2)}),
        "single": dict(shape=(9, 8, 10), seed=6, meshes={1: one, 2: none, 4: small}),
        # 1,300 triangles in one label: six blocks, the last one 20 triangles
        "big": dict(shape=(8, 28, 29), seed=7, background="half",
                    meshes={1: mref.sheet_mesh((3.25, 1.0, 1.0), (0.0, 1.0, 0.0), (0.125, 0.0, 1.0), 25, 26)}),
        "zero": dict(shape=(9, 8, 10), seed=8, background="corner", meshes={1: _zero_area_sheet()}),
        "f32": dict(shape=(9, 8, 10), seed=9, dtype=np.float32, background="half",
                    meshes={1: mref.sphere_mesh((4.0, 3.5, 4.5), 2.75, 1)}),
    }


def background_of(kind, shape):
    if kind is None:
        return None
    bg = np.zeros(shape, dtype=bool)
    if kind == "half":
        bg[:, :, : shape[2] // 2] = True
    else:  # "corner": [0, 0, 0] differs from the rest, where scipy reads for a NaN coordinate
        bg[:] = True
        bg[0, 0, 0] = False
    return bg


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("_ref_velocity_analysis_for_mesh_golden",
                                                  os.path.join(ref, "velocity_analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(va, case, fields, bg, mask, labels):
    queue = [case["meshes"][lab] for lab in labels]

    def marching_cubes(volume, level=None, step_size=1, **kw):
        verts, faces = queue.pop(0)
        if len(faces) == 0:
            raise RuntimeError("no surface found at the given iso value")
        return verts, faces, np.zeros_like(verts), np.zeros(len(verts), dtype=np.float32)

    sk, measure = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    measure.marching_cubes = marching_cubes
    sk.measure = measure
    saved = {k: sys.modules.get(k) for k in ("skimage", "skimage.measure")}
    sys.modules.update({"skimage": sk, "skimage.measure": measure})
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            res = va.compute_interface_drag_mesh(*fields[:3], fields[3], VISC, *H, mask, labels=labels,
                                                 volume=case.get("volume"), background_mask=bg)
    finally:
        for k, m in saved.items():
            if m is None:
                del sys.modules[k]
            else:
                sys.modules[k] = m
    assert not queue
    return res


def build_mesh_case(va, case):
    shape = case["shape"]
    fields = mref.make_fields(shape, case["seed"], case.get("dtype", np.float64), case.get("pressure", True))
    bg = background_of(case.get("background"), shape)
    labels = list(case["meshes"])
    mask = np.zeros(shape, dtype=np.int32)
    for i, lab in enumerate(labels):  # the reference only asks whether the label occurs
        mask.reshape(-1)[i] = lab
    res = run_reference(va, case, fields, bg, mask, labels)
    ex = mref.integrate(case["meshes"], *fields, VISC, *H, background=bg, ft=mref.LD)
    out_labels = list(res)
    assert out_labels == list(ex), (out_labels, list(ex))
    keys = list(res[out_labels[0]])
    assert tuple(keys[:21]) == mref.KEYS
    values = np.array([[res[lab][k] for k in keys] for lab in out_labels], dtype=np.float64)
    exact = np.array([ex[lab][0] for lab in out_labels], dtype=mref.LD)
    hi = exact.astype(np.float64)
    lo = (exact - hi.astype(mref.LD)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        gap = np.abs(values[:, :21].astype(mref.LD) - exact).astype(np.float64)
    d = {"u": fields[0], "v": fields[1], "w": fields[2], "mask": mask, "labels": np.array(labels),
         "spacing": np.array(H), "viscosity": np.float64(VISC), "volume": np.float64(case.get("volume") or 0.0),
         "out_labels": np.array(out_labels), "keys": np.array(keys), "values": values, "exact_hi": hi, "exact_lo": lo,
         "gap": gap, "scale": np.array([ex[lab][1] for lab in out_labels])}
    if fields[3] is not None:
        d["pressure"] = fields[3]
    if bg is not None:
        d["background"] = bg
    for i, lab in enumerate(labels):
        d[f"verts_{i}"], d[f"faces_{i}"] = case["meshes"][lab]
    return d


def spline_points(shape, seed, n=400, special=False):
    rng = np.random.default_rng(seed)
    hi = np.array(shape, dtype=np.float64)[:, None] - 1.0
    pts = rng.uniform(-0.25, hi + 0.25, (3, n))  # up to a quarter voxel outside: where the drag samples
    if special:  # on integers, at .5 ties, just outside both ends
        grid = np.stack(np.meshgrid(*(np.arange(0, s, max(1, s // 3), dtype=np.float64) for s in shape),
                                    indexing="ij")).reshape(3, -1)
        ties = np.minimum(grid + 0.5, hi)
        ends = np.array([[-0.25, shape[0] - 0.75, 2.0, 3.5], [1.0, -0.25, shape[1] - 0.75, 2.5],
                         [shape[2] - 0.75, 4.0, -0.25, -0.25]])
        pts = np.concatenate([pts, grid, ties, ends], axis=1)
    return pts


SPLINES = {"a": dict(shape=(20, 17, 23), seed=11), "line": dict(shape=(1, 2, 70), seed=12),
           "ties": dict(shape=(9, 7, 11), seed=13, special=True)}


def build_spline_case(case):
    field = mref.make_fields(case["shape"], case["seed"])[0]
    pts = spline_points(case["shape"], case["seed"], special=case.get("special", False))
    coef = ndimage.spline_filter(np.pad(field, 12, mode="edge"), 3, mode="nearest")
    s = {o: ndimage.map_coordinates(field, pts, order=o, mode="nearest") for o in (0, 1, 3)}
    coef_x = mref.prefilter(field)
    s3_x, s1_x = mref.sample3(coef_x, pts), mref.sample1(field, pts)
    assert np.array_equal(field[mref.index0(field.shape, pts)], s[0])

    # exact = scipy's value + diff: the difference is ~1e-15, so float32 holds it to ~1e-22
    d = {"field": field, "points": pts, "s0": s[0], "s1": s[1], "s3": s[3]}
    c = {"coef": coef, "coef_diff": (coef_x - coef.astype(mref.LD)).astype(np.float32)}
    for name, x, ref in (("s1", s1_x, s[1]), ("s3", s3_x, s[3])):
        d[name + "_diff"] = (x - ref.astype(mref.LD)).astype(np.float32)
    return d, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    va = load_reference(args.ref)
    todo = [("mesh", n, c) for n, c in _cases().items()] + [("spline", n, c) for n, c in SPLINES.items()]
    for kind, name, case in todo:
        if args.only and name not in args.only:
            continue
        parts = {}
        if kind == "mesh":
            d = build_mesh_case(va, case)
            parts[f"mesh_{name}.npz"] = d
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.nanmax(d["gap"] / np.maximum(mref.EPS * d["scale"], 1e-300))
            print(f"mesh {name}: shape {case['shape']} labels {d['out_labels'].tolist()} max gap / (eps scale) {rel:.2f}")
        else:
            d, c = build_spline_case(case)
            parts[f"spline_{name}.npz"], parts[f"spline_{name}_coef.npz"] = d, c
            print(f"spline {name}: shape {case['shape']} coef gap {np.abs(c['coef_diff']).max():.2e} (max |c| "
                  f"{np.abs(c['coef']).max():.3g}) s3 gap {np.abs(d['s3_diff']).max():.2e}")
        for fname, arrays in parts.items():
            path = os.path.join(HERE, fname)
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            print(f"  {fname}: {size} bytes")
            if size > PART_BYTES:
                raise SystemExit(f"{fname}: {size} bytes exceed the part size {PART_BYTES}")


if __name__ == "__main__":
    main()
