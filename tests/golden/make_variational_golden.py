"""Golden fixtures of the reference's variational divergence cleaning (physics.py:356-514).

Imports the reference ``physics.py`` as ``make_clean_golden.py`` does and runs
``clean_divergence_variational`` per case with its prints redirected.  The reference spells its
solver call ``cg(A, rhs, tol=1e-8, maxiter=2000)``; scipy 1.14 removed ``tol=``, so the module's
``cg`` name is bound to an adapter that calls scipy's ``cg(A, b, rtol=tol, atol=0.0,
maxiter=maxiter)`` (the same test, ``||r|| < tol * ||b||``) and counts iterations through
``callback``, with BLAS held to one thread (a threaded ddot sums in an order that depends on the
thread count, and the fixtures must not).

CG cannot be reproduced bit for bit by an implementation that sums in another order, so every
fixture carries its own bar: the run is repeated with the explicit matrix replaced, in the adapter,
by the matrix-free numpy operator of ``tests/_variational_ref.py`` (only the matvec's rounding order
changes), and the normwise difference of the two runs' fields is stored as ``order_gap``.  A seed is
skipped when the two orderings disagree on ``itn`` or when ``||r||`` at the top of any iteration
lies within 1e-6 relative of the threshold (an implementation with other roundings could then stop
one iteration earlier or later).

Each fixture ``var_<case>.npz`` holds the inputs, the outputs, ``itn``, ``info``, ``order_gap``, the
report's two mean |div| values, and A x (``ax_y*``) for one random x (``ax_x*``) whose entries span
six decades.

Usage:  python tests/golden/make_variational_golden.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _variational_ref as vref  # noqa: E402
from make_clean_golden import PART_BYTES, SPACINGS, load_reference, make_fields, make_mask  # noqa: E402

# name: (shape (nz, ny, nx), lambda, first seed, kind)
CASES = {
    "g12": ((12, 10, 14), 1e3, 1, "grains"),
    "g12_l200": ((12, 10, 14), 200.0, 1, "grains"),
    "thin": ((2, 9, 33), 200.0, 1, "grains"),
    "iso": ((7, 9, 11), 1e3, 1, "isolated"),
    "g20": ((20, 18, 24), 1e5, 1, "grains"),
}
NEAR = 1e-6  # relative distance of ||r|| from the threshold under which a seed is skipped


def run_reference(ref, fields, mask, lam, free):
    """(fields, itn, info, near): one reference run; free = the matrix-free operator instead of A."""
    from scipy.sparse.linalg import cg as scipy_cg

    rec = {"itn": 0, "near": False}

    def adapter(A, b, tol=1e-5, maxiter=None):
        thr = tol * np.linalg.norm(b)
        if np.abs(np.linalg.norm(b) - thr) <= NEAR * thr:
            rec["near"] = True

        def callback(_x):
            rec["itn"] += 1
            r = sys._getframe(1).f_locals["r"]  # scipy's residual after this iteration's update
            if abs(np.linalg.norm(r) - thr) <= NEAR * thr:
                rec["near"] = True

        op = vref.Stencil(mask, *SPACINGS).operator(lam) if free else A
        with vref.single_threaded_blas():  # the dot products' order must not depend on the thread count
            sol, info = scipy_cg(op, b, rtol=tol, atol=0.0, maxiter=maxiter, callback=callback)
        rec["info"] = int(info)
        return sol, info

    orig = ref.cg
    ref.cg = adapter
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = ref.clean_divergence_variational(*fields, mask, *SPACINGS, lambda_reg=lam)
    finally:
        ref.cg = orig
    return out, rec["itn"], rec["info"], rec["near"]


def build_case(ref, shape, lam, seed, kind):
    rng = np.random.default_rng(seed)
    mask = make_mask(shape, rng, kind)
    fields = make_fields(shape, rng)
    out, itn, info, near = run_reference(ref, fields, mask, lam, free=False)
    out2, itn2, info2, near2 = run_reference(ref, fields, mask, lam, free=True)
    if itn != itn2 or info != info2 or near or near2:
        return None
    d = {"u": fields[0], "v": fields[1], "w": fields[2], "mask": mask, "seed": np.int64(seed),
         "dx": np.float64(SPACINGS[0]), "dy": np.float64(SPACINGS[1]), "dz": np.float64(SPACINGS[2]),
         "lambda_reg": np.float64(lam), "itn": np.int64(itn), "info": np.int64(info),
         "order_gap": np.float64(vref.order_gap(out, out2))}
    for name, arr in zip("uvw", out):
        d[f"{name}_c"] = arr
    for key, f in (("mean_abs_div_initial", fields), ("mean_abs_div_final", out)):
        d[key] = np.float64(np.mean(np.abs(ref.compute_consistent_divergence(*f, mask, *SPACINGS)[mask])))
    # A x for one x whose entries span six decades (float32-representable, so that it compresses)
    n = int(mask.sum())
    x = rng.standard_normal(3 * n) * 10.0 ** rng.uniform(-3, 3, 3 * n)
    x = x.astype(np.float32).astype(np.float64)
    Dx, Dy, Dz, _ = ref.build_divergence_operators(mask, *SPACINGS)
    y = vref_matrix(Dx, Dy, Dz, lam) @ x
    for k, name in enumerate("uvw"):
        for key, vec in (("ax_x", x), ("ax_y", y)):
            g = np.zeros(shape)
            g[mask] = vec[k * n:(k + 1) * n]
            d[f"{key}{name}"] = g
    return d


def vref_matrix(Dx, Dy, Dz, lam):
    """The reference's block matrix from its own operators (physics.py:465-480 builds it inline)."""
    from scipy.sparse import bmat, eye

    I = eye(Dx.shape[0])
    xx, xy, xz, yy, yz, zz = Dx.T @ Dx, Dx.T @ Dy, Dx.T @ Dz, Dy.T @ Dy, Dy.T @ Dz, Dz.T @ Dz
    return bmat([[I + lam * xx, lam * xy, lam * xz], [lam * xy.T, I + lam * yy, lam * yz],
                 [lam * xz.T, lam * yz.T, I + lam * zz]], format="csr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    ref = load_reference(args.ref)
    for name, (shape, lam, seed, kind) in CASES.items():
        if args.only and name not in args.only:
            continue
        for s in range(seed, seed + 20):
            d = build_case(ref, shape, lam, s, kind)
            if d is not None:
                break
            print(f"{name}: seed {s}: the orderings disagree on itn or ||r|| is near the threshold, next seed")
        else:
            raise SystemExit(f"{name}: no usable seed")
        path = os.path.join(HERE, f"var_{name}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"{name}: shape {shape} lambda {lam:g} seed {s} fluid {int(d['mask'].sum())} itn {int(d['itn'])} "
              f"info {int(d['info'])} order_gap {float(d['order_gap']):.3e}: {size} bytes")
        if size > PART_BYTES:
            raise SystemExit(f"{name}: {size} bytes exceed the part size {PART_BYTES}")


if __name__ == "__main__":
    main()
