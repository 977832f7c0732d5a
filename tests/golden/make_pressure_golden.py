"""Golden fixtures of the reference's pressure recovery (velocity_analysis.py:190-330 with
physics.py:211-345).

Imports the reference ``velocity_analysis.py`` and ``physics.py`` and runs ``compute_pressure_field``
per case with its prints redirected.  ``solve_poisson`` is wrapped to capture what it is given (the
force field, the Dirichlet mask) and the right-hand side field it computes.  The reference spells
its solver call ``cg(A, b, tol=1e-10, maxiter=3000)``; scipy 1.14 removed ``tol=``, so the module's
``cg`` name is bound to an adapter that calls ``cg(A, b, rtol=tol, atol=0.0, maxiter=maxiter)`` (the
same test) and counts iterations, with BLAS held to one thread, as ``make_variational_golden.py``
does.

A Krylov solve cannot be reproduced bit for bit by an implementation that sums in another order, so
every fixture carries its own bar: the run is repeated with the CSR matrix replaced by the numpy
slice operator of ``tests/_pressure_ref.py`` (for ``anchor='none'``: by ``make_clean_golden``'s
matrix-free builder), and the normwise difference of the two pressures is stored as ``order_gap``.
``itn_free`` is the second run's iteration count.

Each fixture ``pressure_<case>.npz`` holds the inputs, ``fx, fy, fz`` as passed to ``solve_poisson``,
``rhs``, ``dirichlet``, ``p``, ``itn``, ``info`` (CG: scipy's; none: lsqr's istop), the report's three
means and ``order_gap``.

Usage:  python tests/golden/make_pressure_golden.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _pressure_ref as pref  # noqa: E402
from _variational_ref import single_threaded_blas  # noqa: E402
from make_clean_golden import PART_BYTES, SPACINGS, make_fields, make_mask, matrix_free_builder  # noqa: E402

MU = 1e-3
# name: shape (nz, ny, nx), seed, and the arguments that differ from the defaults
CASES = {
    "g12": dict(shape=(12, 10, 14), seed=1),
    "g20": dict(shape=(20, 18, 24), seed=2),
    "inhom": dict(shape=(12, 10, 14), seed=3, wall_bc="inhomogeneous"),
    "rho": dict(shape=(12, 10, 14), seed=4, rho=1000.0, anchor="inlet"),
    "neg": dict(shape=(12, 10, 14), seed=5, flow_direction="negative"),
    "autoneg": dict(shape=(12, 10, 14), seed=6, negate_w=True),
    "odd": dict(shape=(7, 9, 33), seed=7),
    "none": dict(shape=(12, 10, 14), seed=8, anchor="none"),
    "wrap": dict(shape=(12, 10, 14), seed=9, wrap=True),
}


def load_reference(ref):
    mods = {}
    for name in ("physics", "velocity_analysis"):
        spec = importlib.util.spec_from_file_location(f"_ref_{name}_for_pressure_golden", os.path.join(ref, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods["physics"], mods["velocity_analysis"]


def run_reference(phys, va, fields, mask, case, free):
    """One reference run; free = the matrix-free operator instead of the CSR matrix."""
    from scipy.sparse.linalg import cg as scipy_cg

    rec = {"itn": 0, "info": 0}
    dx, dy, dz = SPACINGS

    def adapter(A, b, tol=1e-5, maxiter=None):
        def callback(_x):
            rec["itn"] += 1

        op = pref.slice_operator(mask, rec["dirichlet"], dx, dy, dz) if free else A
        with single_threaded_blas():
            sol, info = scipy_cg(op, b, rtol=tol, atol=0.0, maxiter=maxiter, callback=callback)
        rec["info"] = int(info)
        return sol, info

    orig_lsqr, orig_cg, orig_solve, orig_build = phys.lsqr, phys.cg, phys.solve_poisson, phys.build_laplacian_matrix

    def lsqr(*a, **k):
        with single_threaded_blas():
            res = orig_lsqr(*a, **k)
        rec["info"], rec["itn"] = int(res[1]), int(res[2])
        return res

    def solve_poisson(source, m, hx, hy, hz, force_field=None, wall_bc="inhomogeneous", dirichlet_mask=None,
                      dirichlet_values=None):
        rec["f"] = [np.array(a) for a in force_field]
        rec["dirichlet"] = np.zeros(m.shape, bool) if dirichlet_mask is None else np.array(dirichlet_mask)
        rec["rhs"] = phys.compute_force_divergence(*force_field, m, hx, hy, hz, wall_bc=wall_bc)
        return orig_solve(source, m, hx, hy, hz, force_field=force_field, wall_bc=wall_bc,
                          dirichlet_mask=dirichlet_mask, dirichlet_values=dirichlet_values)

    phys.lsqr, phys.cg, phys.solve_poisson = lsqr, adapter, solve_poisson
    if free and case.get("anchor") == "none":
        phys.build_laplacian_matrix = matrix_free_builder(phys)
    saved = sys.modules.get("physics")
    sys.modules["physics"] = phys  # the reference imports solve_poisson by this name inside the call
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            p = va.compute_pressure_field(*fields, dx, dy, dz, MU, rho=case.get("rho", 0), mask=mask,
                                          wall_bc=case.get("wall_bc", "zero-neumann"),
                                          anchor=case.get("anchor", "outlet"),
                                          flow_direction=case.get("flow_direction", "auto"))
    finally:
        phys.lsqr, phys.cg, phys.solve_poisson, phys.build_laplacian_matrix = orig_lsqr, orig_cg, orig_solve, orig_build
        if saved is None:
            del sys.modules["physics"]
        else:
            sys.modules["physics"] = saved
    return p, rec


def build_case(phys, va, case, seed):
    shape = case["shape"]
    rng = np.random.default_rng(seed)
    mask = make_mask(shape, rng, "grains")
    if case.get("wrap"):
        # the last plane has no bulk neighbour of its own: round 2 fills it from plane 0 across the wrap
        mask[shape[0] - 2] = False
    fields = make_fields(shape, rng)
    if case.get("negate_w"):
        fields[2] = -fields[2]
    p, rec = run_reference(phys, va, fields, mask, case, free=False)
    p2, rec2 = run_reference(phys, va, fields, mask, case, free=True)
    if rec["info"] != rec2["info"]:
        raise SystemExit(f"the two CPU orderings disagree on info: {rec['info']} {rec2['info']}")
    d = {"u": fields[0], "v": fields[1], "w": fields[2], "mask": mask, "mu": np.float64(MU),
         "rho": np.float64(case.get("rho", 0)), "dx": np.float64(SPACINGS[0]), "dy": np.float64(SPACINGS[1]),
         "dz": np.float64(SPACINGS[2]), "wall_bc": np.str_(case.get("wall_bc", "zero-neumann")),
         "anchor": np.str_(case.get("anchor", "outlet")),
         "flow_direction": np.str_(case.get("flow_direction", "auto")),
         "fx": rec["f"][0], "fy": rec["f"][1], "fz": rec["f"][2], "rhs": rec["rhs"], "dirichlet": rec["dirichlet"],
         "p": p, "itn": np.int64(rec["itn"]), "itn_free": np.int64(rec2["itn"]), "info": np.int64(rec["info"]),
         "order_gap": np.float64(pref.normwise(p2, p)), "seed": np.int64(seed),
         "means": np.array([np.mean(np.abs(f[mask])) for f in rec["f"]])}
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    phys, va = load_reference(args.ref)
    for name, case in CASES.items():
        if args.only and name not in args.only:
            continue
        d = build_case(phys, va, case, case["seed"])
        path = os.path.join(HERE, f"pressure_{name}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"{name}: shape {case['shape']} fluid {int(d['mask'].sum())} dirichlet {int(d['dirichlet'].sum())} "
              f"itn {int(d['itn'])} / {int(d['itn_free'])} info {int(d['info'])} order_gap {float(d['order_gap']):.3e}: "
              f"{size} bytes")
        if size > PART_BYTES:
            raise SystemExit(f"{name}: {size} bytes exceed the part size {PART_BYTES}")


if __name__ == "__main__":
    main()
