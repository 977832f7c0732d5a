"""Dev tool: SHA-256 of every output array, and the integer and float stats, of the dense-grid
solvers (projection cleaning, variational cleaning, pressure recovery) on seeded cases, for
bit-identity A/B of library builds (PTV_LIB selects the build, as in tools/out_hash.py).

    PTV_LIB=ab/libptv_base.so python tools/grid_solver_hash.py [--big] > base.txt
    python tools/grid_solver_hash.py [--big] > new.txt
    python tools/grid_solver_hash.py --join base.txt new.txt      # the table of pairs with a match column

One line per call: ``case | entry point | sha256 of the outputs | stats``.  Floats are printed as
hex, timings (``ms_*``) are left out, and an error is printed by its message.  The small cases
cover the one- and two-wide paths, groups whose x neighbours are both faces, extents of one, the
alignment fallback (arrays offset by one element, through the ``_dev`` entry points), more than
256 partial sums, iteration limits around the polling batch of 8, a zero right-hand side and a NaN
in a fluid voxel; ``--big`` adds one 256^3 sphere-pack case per solver (the benchmarks' inputs).
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = (0.7, 1.1, 1.3)  # dx, dy, dz


def fmt(v):
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(fmt(x) for x in v) + "]"
    return str(v)


def emit(case, entry, fn):
    """Run fn() -> (arrays, stats dict or None) and print its line."""
    from ptv_interpolation_amd import _lib

    try:
        arrays, st = fn()
    except (_lib.PtvError, ValueError) as e:
        print(f"{case} | {entry} | error | {e}", flush=True)
        return
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    stats = " ".join(f"{k}={fmt(v)}" for k, v in (st or {}).items() if not k.startswith("ms_"))
    print(f"{case} | {entry} | {h.hexdigest()} | {stats}", flush=True)


def inputs(shape, seed, fluid=0.8):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < fluid
    mask.flat[0] = True
    f = [rng.standard_normal(shape) for _ in range(4)]
    dirichlet = (rng.random(shape) < 0.1) & mask
    return mask, f, dirichlet


def host_calls(ctx, case, mask, f, dirichlet, iters, outer=(1,), tol=None):
    """Every entry point of the three solvers on host arrays."""
    u, v, w, phi = f
    lsqr = dict(iter_lim=iters) if tol is None else dict(iter_lim=iters, atol=tol, btol=tol)
    cg = dict(maxiter=iters) if tol is None else dict(maxiter=iters, rtol=tol)
    for it in outer:
        emit(case, f"clean outer={it}", lambda: ctx.clean_divergence(u, v, w, mask, *H, iterations=it, **lsqr))
    emit(case, "lsqr rhs", lambda: (lambda x, st: ([x], st))(*ctx.poisson_solve(mask, *H, rhs=phi, **lsqr)))
    emit(case, "laplacian", lambda: ([ctx.laplacian_apply(phi, mask, *H)], None))
    emit(case, "correction", lambda: (ctx.apply_correction(u, v, w, phi, mask, *H), None))
    emit(case, "variational", lambda: ctx.clean_variational(u, v, w, mask, *H, lambda_reg=200.0, **cg))
    emit(case, "var D", lambda: ([ctx.divergence_operator_apply(u, v, w, mask, *H)], None))
    emit(case, "var A", lambda: (ctx.variational_apply(u, v, w, mask, *H, 200.0), None))
    for rho in (0.0, 1.2):
        emit(case, f"force rho={rho}", lambda: ctx.force_field(u, v, w, mask, *H, 1e-3, rho))
    for bc in ("zero-neumann", "inhomogeneous"):
        emit(case, f"force div {bc}", lambda: ([ctx.force_divergence(u, v, w, mask, *H, wall_bc=bc)], None))
    emit(case, "cg dirichlet", lambda: (lambda x, st: ([x], st))(
        *ctx.poisson_solve(mask, *H, rhs=phi, dirichlet=dirichlet, **cg)))
    emit(case, "cg anchor", lambda: (lambda x, st: ([x], st))(*ctx.pressure_recover(u, v, w, mask, *H, 1e-3, **cg)))


def offset_calls(ctx, case, shape, seed, iters):
    """Even nx with every device array one element off a 16-byte (mask: 2-byte) boundary."""
    import torch

    dev = torch.device("cuda", 0)
    mask, f, dirichlet = inputs(shape, seed)
    nz, ny, nx = shape
    n = mask.size

    def off(a):  # a device copy that starts one element into its allocation
        t = torch.empty(n + 1, dtype=torch.float64 if a.dtype == np.float64 else torch.uint8, device=dev)
        t[1:] = torch.from_numpy(np.ascontiguousarray(a).ravel()).to(dev)
        return t, t.data_ptr() + t.element_size()

    keep = [off(a) for a in f] + [off(mask.view(np.uint8)), off(dirichlet.view(np.uint8))]
    (u, v, w, phi, m, d) = [p for _, p in keep]
    outs = [off(np.zeros(shape)) for _ in range(3)]
    optr = [p for _, p in outs]
    back = lambda k: [outs[i][0][1:].cpu().numpy() for i in range(k)]  # noqa: E731
    sync = torch.cuda.synchronize
    emit(case, "clean_dev", lambda: (lambda st: (back(3), st))(
        ctx.clean_divergence_dev(nx, ny, nz, [u, v, w], m, optr, *H, iterations=2, iter_lim=iters)))
    emit(case, "variational_dev", lambda: (lambda st: (back(3), st))(
        ctx.clean_variational_dev(nx, ny, nz, [u, v, w], m, optr, *H, lambda_reg=200.0, maxiter=iters)))
    emit(case, "lsqr rhs_dev", lambda: (lambda st: (back(1), st))(
        ctx.poisson_solve_dev(nx, ny, nz, m, optr[0], *H, rhs_ptr=phi, iter_lim=iters)))
    emit(case, "cg dirichlet_dev", lambda: (lambda st: (back(1), st))(
        ctx.poisson_solve_dev(nx, ny, nz, m, optr[0], *H, rhs_ptr=phi, dirichlet_ptr=d, maxiter=iters)))
    emit(case, "force_dev", lambda: (lambda st: (back(3), st))(
        ctx.force_field_dev(nx, ny, nz, [u, v, w], m, optr, *H, 1e-3, 1.2)))
    emit(case, "force div_dev", lambda: (ctx.force_divergence_dev(nx, ny, nz, [u, v, w], m, optr[0], *H,
                                                                   wall_bc="inhomogeneous"), sync(), (back(1), None))[2])
    emit(case, "cg anchor_dev", lambda: (lambda st: (back(1), st))(
        ctx.pressure_recover_dev(nx, ny, nz, [u, v, w], m, optr[0], *H, 1e-3, maxiter=iters)))


def big_calls(ctx, G=256):
    """One bench-sized sphere-pack case per solver (the inputs of tools/*_bench.py)."""
    from ptv_interpolation_amd import _lib, synth

    mask = synth.fluid_mask(G)
    P, Q = synth.sphere_pack(500_000, G, values="normal")
    ax = np.arange(G, dtype=np.float64)
    u, v, w = [np.nan_to_num(a) for a in
               ctx.interp_knn(P, Q, axes=(ax, ax, ax), method=_lib.METHOD_IDW, k=8, fluid_mask=mask)]
    case = f"sphere-pack {G}^3"
    emit(case, "clean outer=1", lambda: ctx.clean_divergence(u, v, w, mask, 1.0, 1.0, 1.0, iterations=1, iter_lim=100))
    emit(case, "variational", lambda: ctx.clean_variational(u, v, w, mask, 1.0, 1.0, 1.0, lambda_reg=200.0, maxiter=100))
    emit(case, "cg anchor", lambda: (lambda x, st: ([x], st))(
        *ctx.pressure_recover(u, v, w + 1.0, mask, 1.0, 1.0, 1.0, 1e-3, rtol=1e-10, maxiter=300)))


def run(big):
    import torch

    torch.cuda.init()  # before the library opens the device, as in tools/*_bench.py
    from ptv_interpolation_amd import _lib

    ctx = _lib.Context.get(0)
    first = (5, 4, 2)  # two-wide, both x neighbours of every group at faces
    mask, f, dirichlet = inputs(first, 1)
    host_calls(ctx, f"{first}", mask, f, dirichlet, 40, outer=(1, 3))
    for lim in (0, 1, 8, 9, 17):  # before the first poll, at a batch edge, one past it; tolerance 0: the limit ends it
        host_calls(ctx, f"{first} limit={lim}", mask, f, dirichlet, lim, tol=0.0)
    zero = [np.zeros(first) for _ in range(4)]
    host_calls(ctx, f"{first} zero rhs", mask, zero, dirichlet, 40)
    nan = [a.copy() for a in f]
    for a in nan:
        a[tuple(np.argwhere(mask & ~dirichlet)[3])] = np.nan
    host_calls(ctx, f"{first} nan", mask, nan, dirichlet, 40)
    for seed, shape in enumerate([(7, 9, 13), (1, 6, 8), (6, 1, 8), (6, 8, 1)], start=2):  # one-wide; extents of one
        host_calls(ctx, f"{shape}", *inputs(shape, seed), 40, outer=(1, 3))
    offset_calls(ctx, "(6, 8, 10) offset", (6, 8, 10), 6, 40)
    for seed, shape in enumerate([(66, 66, 66), (80, 80, 82)], start=7):  # more than 256 partials, one- and two-wide
        host_calls(ctx, f"{shape}", *inputs(shape, seed), 20)
    if big:
        big_calls(ctx)


def join(pa, pb):
    rows = [[ln.rstrip("\n").split(" | ") for ln in open(p) if " | " in ln] for p in (pa, pb)]
    keys = [[(r[0], r[1]) for r in rs] for rs in rows]
    if keys[0] != keys[1]:
        sys.exit("the two files list different cases")
    bad = 0
    print(f"# a = {pa}, b = {pb}; sha256 is shortened to 16 digits, match compares the whole lines")
    print("case | entry point | sha256 a | sha256 b | match")
    for ra, rb in zip(*rows):
        ok = ra == rb
        bad += not ok
        print(f"{ra[0]} | {ra[1]} | {ra[2][:16]} | {rb[2][:16]} | {'yes' if ok else 'NO'}")
        if not ok:
            print(f"    a: {' | '.join(ra[3:])}\n    b: {' | '.join(rb[3:])}")
    print(f"# {len(rows[0])} pairs, {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--join", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.join:
        join(*args.join)
    else:
        run(args.big)
