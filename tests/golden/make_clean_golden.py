"""Golden fixtures of the reference's projection-method divergence cleaning (physics.py:55-209).

Imports the reference ``physics.py`` and runs, per case, ``clean_divergence_projection`` with
``iterations=1`` and ``iterations=3``, ``apply_consistent_correction`` on the first solve's phi and
``build_laplacian_matrix`` on a random vector.  The reference's prints (and scipy's ``show=True``
log) are redirected away.

LSQR cannot be reproduced bit for bit by any implementation that sums in another order, so every
fixture carries its own bar: the same reference run is repeated with ``build_laplacian_matrix``
replaced, inside the loaded module, by a matrix-free numpy operator (only the matvec's rounding
order changes), and the normwise difference of the cleaned fields (``order_gap_fields``, the 2-norm
over all three components relative to the reference's) and the relative difference of the final
mean |div| (``order_gap_div``) are stored, entry 0 for ``iterations=1`` and entry 1 for
``iterations=3``.  Both orderings must agree on ``istop`` for every solve; a case whose orderings
disagree is regenerated from the next seed.

Each case is written as ``clean_<case>.npz`` holding arrays only; a case whose arrays exceed what
one committed file may hold continues in ``clean_<case>.p1.npz``, ``.p2.npz``, ...
(``tests/test_gpu_clean.py`` merges the parts).  The input fields are float32-representable
float64 values, which compress.

Usage:  python tests/golden/make_clean_golden.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import contextlib
import glob
import importlib.util
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900_000  # per committed file

# name: (shape (nz, ny, nx), first seed, kind)
CASES = {
    "g12": ((12, 10, 14), 1, "grains"),
    "g20": ((20, 18, 24), 1, "grains"),
    "g32": ((32, 28, 36), 1, "grains"),
    "thin": ((2, 9, 33), 1, "grains"),
    "iso": ((7, 9, 11), 1, "isolated"),
}
SPACINGS = (1.0, 1.25, 0.8)  # dx, dy, dz


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("_ref_physics_for_golden", os.path.join(ref, "physics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_mask(shape, rng, kind):
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.ones(shape, bool)
    for _ in range(6):  # six random spherical grains
        c = rng.uniform(0, 1, 3) * np.array([nz, ny, nx])
        r = rng.uniform(0.12, 0.22) * max(min(ny, nx), 6)
        mask &= (Z - c[0]) ** 2 + (Y - c[1]) ** 2 + (X - c[2]) ** 2 > r * r
    if kind == "isolated":
        # a fluid voxel fully enclosed by solid (a zero row of A) and a solid voxel on a domain face
        cz, cy, cx = nz // 2, ny // 2, nx // 2
        mask[cz - 1:cz + 2, cy - 1:cy + 2, cx - 1:cx + 2] = False
        mask[cz, cy, cx] = True
        mask[0, 1, 2] = False
        mask[nz - 1, ny - 1, nx - 1] = False
    return mask


def make_fields(shape, rng):
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    u = np.sin(X / 5.0) + 0.3 * np.cos(Y / 3.0) + 0.1 * rng.standard_normal(shape)
    v = np.cos(Y / 4.0) * np.sin(Z / 3.0) + 0.1 * rng.standard_normal(shape)
    w = 1.0 + 0.2 * np.sin(Z / 2.0 + X / 7.0) + 0.1 * rng.standard_normal(shape)
    return [a.astype(np.float32).astype(np.float64) for a in (u, v, w)]


def matrix_free_builder(ref):
    """A stand-in for build_laplacian_matrix: the same operator, applied as a numpy stencil."""
    from scipy.sparse.linalg import LinearOperator

    def build(mask, dx, dy, dz):
        n = int(mask.sum())
        idx_map = np.full(mask.shape, -1, dtype=np.int32)
        idx_map[mask] = np.arange(n)
        h2 = {2: 1.0 / (dx ** 2), 1: 1.0 / (dy ** 2), 0: 1.0 / (dz ** 2)}

        def matvec(xc):
            X = np.zeros(mask.shape)
            X[mask] = np.asarray(xc).ravel()
            Y = np.zeros(mask.shape)
            for axis in (2, 1, 0):
                lo = [slice(None)] * 3
                hi = [slice(None)] * 3
                lo[axis] = slice(0, -1)
                hi[axis] = slice(1, None)
                lo, hi = tuple(lo), tuple(hi)
                both = mask[lo] & mask[hi]
                d = np.where(both, (X[hi] - X[lo]) * h2[axis], 0.0)
                Y[lo] += d
                Y[hi] -= d
            return Y[mask]

        return LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64), idx_map

    return build


def run_reference(ref, fields, mask, iterations, builder=None):
    """(cleaned fields, [(istop, itn)], [phi], final mean |div|) of one reference run."""
    solves, phis = [], []
    orig_lsqr, orig_build = ref.lsqr, ref.build_laplacian_matrix

    def lsqr(*a, **k):
        res = orig_lsqr(*a, **k)
        solves.append((int(res[1]), int(res[2])))
        phis.append(np.array(res[0]))
        return res

    ref.lsqr = lsqr
    if builder is not None:
        ref.build_laplacian_matrix = builder
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = ref.clean_divergence_projection(*fields, mask, *SPACINGS, iterations=iterations)
    finally:
        ref.lsqr, ref.build_laplacian_matrix = orig_lsqr, orig_build
    div = ref.compute_consistent_divergence(*out, mask, *SPACINGS)
    return out, solves, phis, float(np.mean(np.abs(div[mask])))


def build_case(ref, shape, seed, kind):
    rng = np.random.default_rng(seed)
    mask = make_mask(shape, rng, kind)
    fields = make_fields(shape, rng)
    free = matrix_free_builder(ref)
    d = {"u": fields[0], "v": fields[1], "w": fields[2], "mask": mask, "seed": np.int64(seed),
         "dx": np.float64(SPACINGS[0]), "dy": np.float64(SPACINGS[1]), "dz": np.float64(SPACINGS[2])}
    gap_f, gap_d = [], []
    for its in (1, 3):
        out, solves, phis, mdiv = run_reference(ref, fields, mask, its)
        out2, solves2, _, mdiv2 = run_reference(ref, fields, mask, its, builder=free)
        if [s[0] for s in solves] != [s[0] for s in solves2]:
            return None  # the two CPU orderings stop for different reasons: try another seed
        a, b = np.stack(out), np.stack(out2)
        gap_f.append(np.linalg.norm((a - b).ravel()) / np.linalg.norm(a.ravel()))
        gap_d.append(abs(mdiv - mdiv2) / mdiv)
        for name, arr in zip("uvw", out):
            d[f"{name}_it{its}"] = arr
        d[f"istop_it{its}"] = np.array([s[0] for s in solves], np.int64)
        d[f"itn_it{its}"] = np.array([s[1] for s in solves], np.int64)
        d[f"itn_free_it{its}"] = np.array([s[1] for s in solves2], np.int64)
        d[f"mean_abs_div_it{its}"] = np.float64(mdiv)
        if its == 1:
            d["phi"] = phis[0]
    d["order_gap_fields"] = np.array(gap_f)
    d["order_gap_div"] = np.array(gap_d)
    with contextlib.redirect_stdout(io.StringIO()):
        corr = ref.apply_consistent_correction(*fields, d["phi"], mask, *SPACINGS)
        A, _ = ref.build_laplacian_matrix(mask, *SPACINGS)
    for name, arr in zip("uvw", corr):
        d[f"corr_{name}"] = arr
    x = rng.standard_normal(int(mask.sum())).astype(np.float32).astype(np.float64)
    for key, vec in (("lap_x", x), ("lap_y", A @ x), ("lap_abs", abs(A) @ np.abs(x))):
        g = np.zeros(shape)
        g[mask] = vec
        d[key] = g
    return d


def write_parts(name, d):
    for old in glob.glob(os.path.join(HERE, f"clean_{name}.npz")) + glob.glob(os.path.join(HERE, f"clean_{name}.p*.npz")):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k, a in d.items():
        a = np.asarray(a)
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(HERE, f"clean_{name}.npz" if i == 0 else f"clean_{name}.p{i}.npz")
        np.savez_compressed(path, **part)
        print(f"  {os.path.basename(path)}: {os.path.getsize(path)} bytes, {sorted(part)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    ref = load_reference(args.ref)
    for name, (shape, seed, kind) in CASES.items():
        if args.only and name not in args.only:
            continue
        for s in range(seed, seed + 20):
            d = build_case(ref, shape, s, kind)
            if d is not None:
                break
            print(f"{name}: seed {s}: the two CPU orderings disagree on istop, trying the next seed")
        else:
            raise SystemExit(f"{name}: no seed on which both CPU orderings agree")
        print(f"{name}: shape {shape} seed {s} fluid {int(d['mask'].sum())} istop {d['istop_it3'].tolist()} "
              f"itn {d['itn_it3'].tolist()} / {d['itn_free_it3'].tolist()} gaps {d['order_gap_fields'].tolist()} "
              f"{d['order_gap_div'].tolist()}")
        write_parts(name, d)


if __name__ == "__main__":
    main()
