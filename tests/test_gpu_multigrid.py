"""The multigrid preconditioner and the preconditioned anchored solve on the GPU
(csrc/ptv_multigrid.hip, press_pcg) against the numpy restatement (tests/_mg_ref.py) and scipy's
``cg(A, b, M=...)``.

``z = M r`` is demanded bit for bit at every voxel.  The solve is compared normwise in units of the
fixture's PCG ``order_gap``: the difference between the oracle run with np.dot and with its inner
products summed in another fixed order; the device, a third ordering, is granted FACTOR = 10 units
(the bar of the plain solve's tests).
"""
import numpy as np
import pytest

import _mg_ref as mg
import _pressure_ref as pref

pytestmark = pytest.mark.gpu

FACTOR = 10.0


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


_h = {}


def hierarchy(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _h:
        mask, d, sp = mg.case(name)
        _h[key] = mg.Hierarchy(mask, d, *sp, **kw)
    return _h[key]


def residual_vector(name):
    return np.random.default_rng(17).standard_normal(mg.case(name)[0].shape)


def same_bits(z, ref):
    bad = z.view(np.uint64) != ref.view(np.uint64)
    if bad.any():
        print(f"{int(bad.sum())} of {bad.size} voxels differ, max |diff| {np.abs(z - ref).max():.3e}, first at "
              f"{np.argwhere(bad)[0]}")
    return not bad.any()


def check_stats(st, H):
    assert st["levels"] == len(H.levels) and st["cells"] == H.cells() and st["active"] == H.active()
    assert st["tail_level"] == H.tail_level()


def test_abi_sizes13(ctx):
    from ptv_interpolation_amd import _lib

    c, py = _lib.abi_sizes13()
    assert c == py


# the launch paths the cases are there for: (lane width of level 0, the tail's first level)
PATHS = {"odd": (1, 0), "g20": (2, 1), "half": (2, 2), "line5": (1, 0), "cube2": (2, 0), "col6": (1, 0),
         "pockets": (2, 0), "plane": (2, 0)}


@pytest.mark.parametrize("name", mg.CASES)
def test_apply_bits(ctx, name):
    mask, d, sp = mg.case(name)
    H = hierarchy(name)
    assert (2 if mask.shape[2] % 2 == 0 else 1, H.tail_level()) == PATHS[name]
    r = residual_vector(name)
    z, st = ctx.poisson_mg_apply(mask, *sp, r, dirichlet=d)
    check_stats(st, H)
    assert same_bits(z, H.apply(r))
    assert not z[~(mask & ~d)].any()
    z2, _ = ctx.poisson_mg_apply(mask, *sp, r, dirichlet=d)
    assert same_bits(z2, z)


def test_apply_without_a_dirichlet_grid(ctx):
    mask, _, sp = mg.case("g20")
    r = residual_vector("g20")
    z, _ = ctx.poisson_mg_apply(mask, *sp, r)
    assert same_bits(z, mg.Hierarchy(mask, None, *sp).apply(r))


def _dev_apply(ctx, name, offset, **kw):
    """poisson_mg_apply_dev on torch tensors that start ``offset`` elements into their allocations."""
    import torch

    dev = torch.device("cuda", 0)
    mask, d, sp = mg.case(name)
    n = mask.size

    def put(a, dtype):
        base = torch.zeros(n + offset, dtype=dtype, device=dev)
        base[offset:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return base, base[offset:]

    held = [put(residual_vector(name), torch.float64), put(mask.view(np.uint8), torch.uint8),
            put(d.view(np.uint8), torch.uint8), put(np.full(n, 7.0), torch.float64)]
    r, mk, dm, out = (t for _, t in held)
    torch.cuda.synchronize()
    nz, ny, nx = mask.shape
    st = ctx.poisson_mg_apply_dev(nx, ny, nz, mk.data_ptr(), r.data_ptr(), out.data_ptr(), *sp,
                                  dirichlet_ptr=dm.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(mask.shape), st


@pytest.mark.parametrize("name", ["g20", "half"])
def test_apply_dev_unaligned(ctx, name):
    ref = hierarchy(name).apply(residual_vector(name))
    for offset in (0, 1):  # nx is even: offset 1 leaves the grids 8 bytes off a 16-byte boundary
        z, st = _dev_apply(ctx, name, offset)
        assert same_bits(z, ref)


# max_levels moves the tail's first level, and past the coarsest level that fits there is no tail
@pytest.mark.parametrize("name,max_levels,tail", [("half", 1, 1), ("half", 2, 2), ("half", 3, 2), ("half", 4, 2),
                                                  ("half", 6, 2), ("g20", 1, 1), ("g20", 2, 1), ("odd", 1, 0),
                                                  ("odd", 3, 0)])
def test_tail_boundary(ctx, name, max_levels, tail):
    mask, d, sp = mg.case(name)
    H = hierarchy(name, max_levels=max_levels)
    assert H.tail_level() == tail and len(H.levels) == max_levels
    r = residual_vector(name)
    z, st = ctx.poisson_mg_apply(mask, *sp, r, dirichlet=d, multigrid={"max_levels": max_levels})
    check_stats(st, H)
    assert same_bits(z, H.apply(r))


# odd sweep counts take the other buffer parity, in the tail and above it
@pytest.mark.parametrize("name", ["odd", "half"])
@pytest.mark.parametrize("kw", [dict(nu=1, coarse_sweeps=5), dict(nu=3, coarse_sweeps=2, omega=0.8)])
def test_sweep_parity(ctx, name, kw):
    mask, d, sp = mg.case(name)
    r = residual_vector(name)
    z, _ = ctx.poisson_mg_apply(mask, *sp, r, dirichlet=d, multigrid=kw)
    assert same_bits(z, hierarchy(name, **kw).apply(r))


_oracle = {}


def oracle(name):
    """scipy's PCG on the fixture, the same recurrence with its inner products in another order, and
    their normwise difference (the fixture's PCG order_gap)."""
    if name not in _oracle:
        mask, d, sp, rhs = mg._golden(name)
        p, itn, info = mg.pcg(rhs, mask, d, *sp)
        p2, itn2, info2 = mg.pcg(rhs, mask, d, *sp, dot=mg.chunked_dot)
        assert info == info2
        _oracle[name] = dict(mask=mask, d=d, sp=sp, rhs=rhs, p=p, itn=itn, info=info, itn2=itn2,
                             gap=pref.normwise(p2, p))
    return _oracle[name]


def check_solution(o, x, st, what):
    ratio = pref.normwise(x, o["p"]) / o["gap"]
    print(f"{what}: ratio {ratio:.3f} of order_gap {o['gap']:.3e}, itn {st['itn']} (oracle {o['itn']} / {o['itn2']}), "
          f"info {st['info']}")
    assert st["info"] == o["info"]
    assert min(o["itn"], o["itn2"]) <= st["itn"] <= max(o["itn"], o["itn2"])
    assert (x[~o["mask"]] == 0).all() and (x[o["d"]] == 0).all()
    assert ratio <= FACTOR
    return ratio


@pytest.mark.parametrize("name", ["g12", "g20", "odd"])
def test_solve_against_the_oracle(ctx, name):
    """info and itn equal scipy's; x within FACTOR = 10 of the PCG order_gap.  The solve forms q = A p
    in the assembled matrix's form and order (k_pqm), so that only the inner products' order separates
    it from the oracle.  Measured on 1 x MI355X: 1.01 (g12), 1.12 (g20), 0.46 (odd) gaps."""
    o = oracle(name)
    x, st = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=o["rhs"], dirichlet=o["d"])
    check_solution(o, x, st, name)
    check_stats(st["multigrid"], mg.Hierarchy(o["mask"], o["d"], *o["sp"]))
    assert st["n_dirichlet"] == int(o["d"].sum()) and st["n_fluid"] == int(o["mask"].sum())
    x2, st2 = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=o["rhs"], dirichlet=o["d"])
    assert same_bits(x2, x) and st2["itn"] == st["itn"]


def true_residual(o, x):
    act = o["mask"] & ~o["d"]
    g = np.where(act, x, 0.0)
    b = np.where(act, o["rhs"], 0.0)
    res = np.where(act, b - pref.laplacian_apply(g, o["mask"], *o["sp"]), 0.0)
    return float(np.linalg.norm(res) / np.linalg.norm(b))


@pytest.mark.parametrize("name", ["g12", "g20", "odd"])
def test_true_residual(ctx, name):
    """Both recurrences stop at their first iterate whose recursively updated residual is below
    rtol |b|, so each of those lies somewhere in [0, rtol): they differ by at most rtol.  The true
    residual b - A x drifts from the updated one by the rounding of k updates r -= alpha q and
    x += alpha p, at most k * 2**-53 * (|A| |x| + |b|) / |b| with |A| <= 4 (dx^-2 + dy^-2 + dz^-2) for
    a run of k iterations.  The margin over the plain answer's true residual is rtol plus that drift
    for both runs."""
    o = oracle(name)
    x, st = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=o["rhs"], dirichlet=o["d"])
    plain, itn_plain, info = pref.cg_solve(o["rhs"], o["mask"], o["d"], *o["sp"])
    assert info == 0
    act = o["mask"] & ~o["d"]
    a_norm = 4.0 * sum(1.0 / (h * h) for h in o["sp"])
    scale = (a_norm * np.linalg.norm(x[act]) + np.linalg.norm(o["rhs"][act])) / np.linalg.norm(o["rhs"][act])
    margin = 1e-10 + (st["itn"] + itn_plain) * 2.0 ** -53 * scale
    dev, ref = true_residual(o, x), true_residual(o, plain)
    print(f"{name}: true relative residual device pcg {dev:.3e} ({st['itn']} iterations), scipy plain cg {ref:.3e} "
          f"({itn_plain}), margin {margin:.3e}")
    assert dev <= ref + margin


@pytest.mark.parametrize("maxiter", [0, 1, 7, 8, 9, 16, 17])
def test_truncated_solves(ctx, maxiter):
    o = oracle("g12")
    ref, itn, info = mg.pcg(o["rhs"], o["mask"], o["d"], *o["sp"], maxiter=maxiter)
    x, st = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=o["rhs"], dirichlet=o["d"], maxiter=maxiter)
    assert (st["info"], st["itn"]) == (info, itn) == (maxiter, maxiter)
    # to rounding, by BIG_TOL's count: per iteration three inner products of n = 1680 terms
    # (log2(n) = 11 units of 2**-53 either way) and a 6-term stencil sum, doubled for the two runs
    tol = 2 * max(maxiter, 1) * (3 * 11 + 6) * 2.0 ** -53
    r = pref.normwise(x, ref)
    print(f"maxiter {maxiter}: normwise {r:.3e} (tolerance {tol:.3e})")
    assert r <= tol


def test_zero_rhs_and_nan(ctx):
    o = oracle("g12")
    x, st = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=np.zeros_like(o["rhs"]), dirichlet=o["d"])
    assert not x.any() and (st["info"], st["itn"], st["bnorm"]) == (0, 0, 0.0)
    rhs = o["rhs"].copy()
    rhs[tuple(np.argwhere(o["mask"] & ~o["d"])[5])] = np.nan
    x, st = ctx.poisson_solve_mg(o["mask"], *o["sp"], rhs=rhs, dirichlet=o["d"])
    assert np.isnan(x[o["mask"]]).all() and (x[~o["mask"]] == 0).all()
    assert (st["info"], st["itn"]) == (3000, 3000)


def test_all_dirichlet_plane(ctx):
    mask, d, sp = mg.case("plane")
    rhs = np.random.default_rng(1).standard_normal(mask.shape)
    x, st = ctx.poisson_solve_mg(mask, *sp, rhs=rhs, dirichlet=d)
    assert not x.any() and (st["itn"], st["info"]) == (0, 0) and st["n_dirichlet"] == int(mask.sum())


@pytest.fixture(scope="module")
def big():
    """82 x 80 x 82: more than 256 first-stage partials in both lane widths; the oracle is scipy's PCG
    truncated at 16 iterations, computed once."""
    rng = np.random.default_rng(5)
    shape = (82, 80, 82)
    Z, Y, X = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    mask = np.ones(shape, bool)
    for _ in range(12):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        mask &= (Z - c[0]) ** 2 + (Y - c[1]) ** 2 + (X - c[2]) ** 2 > rng.uniform(6, 12) ** 2
    rhs = rng.standard_normal(shape)
    d = pref.dirichlet_grid(mask, shape[0] - 1)
    sp = (1.0, 1.25, 0.8)
    return dict(mask=mask, rhs=rhs, d=d, sp=sp, ref=mg.pcg(rhs, mask, d, *sp, maxiter=16)[0])


# 16 iterations, each with three inner products of n = 5e5 terms summed in another order than numpy's
# (either order errs by at most about log2(n) = 19 units of 2**-53 relative) and a 6-term stencil sum;
# z = M r is the same bits on both sides: 16 * (3 * 19 + 6) units, doubled for the two runs compared
BIG_TOL = 2 * 16 * (3 * 19 + 6) * 2.0 ** -53


def test_many_partials_both_widths(ctx, big):
    """Measured on 1 x MI355X: 8.8e-16 (two x per lane) and 5.8e-16 (one) normwise."""
    import torch

    dev = torch.device("cuda", 0)
    n = big["mask"].size
    assert n // (256 * 4 * 2) > 256  # blocks of a two-wide pass
    nz, ny, nx = big["mask"].shape
    outs = []
    for offset in (0, 1, 0):  # two x per lane, one x per lane (8 bytes off), and the first again
        def put(a, dtype):
            base = torch.zeros(n + offset, dtype=dtype, device=dev)
            base[offset:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            return base, base[offset:]

        held = [put(big["rhs"], torch.float64), put(big["mask"].view(np.uint8), torch.uint8),
                put(big["d"].view(np.uint8), torch.uint8), put(np.full(n, 7.0), torch.float64)]
        rhs, mk, dm, out = (t for _, t in held)
        torch.cuda.synchronize()
        st = ctx.poisson_solve_mg_dev(nx, ny, nz, mk.data_ptr(), out.data_ptr(), *big["sp"], rhs_ptr=rhs.data_ptr(),
                                      dirichlet_ptr=dm.data_ptr(), maxiter=16)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().reshape(big["mask"].shape))
        assert (st["itn"], st["info"]) == (16, 16)
        assert st["multigrid"]["tail_level"] == 3 and st["multigrid"]["levels"] == 7
    assert same_bits(outs[0], outs[2])  # fixed-order sums: a call repeats bit for bit
    for x in outs[:2]:
        r = pref.normwise(x, big["ref"])
        print(f"normwise {r:.3e} (tolerance {BIG_TOL:.3e})")
        assert r <= BIG_TOL
        assert (x[~big["mask"]] == 0).all() and (x[big["d"]] == 0).all()


def test_python_paths(ctx):
    from ptv_interpolation_amd import physics, velocity_analysis

    g = {k: v for k, v in np.load(mg.os_path_golden("g12"), allow_pickle=False).items()}
    o = oracle("g12")
    sp = o["sp"]
    x, st = ctx.poisson_solve_mg(o["mask"], *sp, rhs=o["rhs"], dirichlet=o["d"])
    p = physics.solve_poisson(o["rhs"], o["mask"], *sp, dirichlet_mask=o["d"], preconditioner="multigrid")
    assert same_bits(p, x) and physics.solve_poisson.last_stats["multigrid"]["levels"] == 4
    assert (physics.solve_poisson.last_stats["itn"], physics.solve_poisson.last_stats["info"]) == (st["itn"], 0)
    p3, _ = ctx.poisson_solve_mg(o["mask"], *sp, rhs=o["rhs"], dirichlet=o["d"], multigrid={"nu": 1})
    p4 = physics.solve_poisson(o["rhs"], o["mask"], *sp, dirichlet_mask=o["d"], preconditioner="multigrid",
                               multigrid={"nu": 1})
    assert same_bits(p4, p3) and not same_bits(p3, x)
    args = (g["u"], g["v"], g["w"], *sp, float(g["mu"]), float(g["rho"]), g["mask"], str(g["wall_bc"]),
            str(g["anchor"]), str(g["flow_direction"]))
    pr, str_ = velocity_analysis.recover_pressure(*args, preconditioner="multigrid")
    assert same_bits(pr, x) and (str_["itn"], str_["info"]) == (st["itn"], 0)  # item 3's answer, bit for bit
    pf = velocity_analysis.compute_pressure_field(*args, preconditioner="multigrid")
    assert same_bits(pf, pr)
    # the default is the existing call, bit for bit
    plain, _ = ctx.poisson_solve(o["mask"], *sp, rhs=o["rhs"], dirichlet=o["d"])
    assert same_bits(physics.solve_poisson(o["rhs"], o["mask"], *sp, dirichlet_mask=o["d"], preconditioner=None), plain)
    assert same_bits(velocity_analysis.recover_pressure(*args)[0], plain)
    # the refusals
    with pytest.raises(NotImplementedError):
        physics.solve_poisson(o["rhs"], o["mask"], *sp, preconditioner="multigrid")
    with pytest.raises(NotImplementedError):
        velocity_analysis.recover_pressure(*args[:-2], "none", "auto", preconditioner="multigrid")
    with pytest.raises(ValueError):
        physics.solve_poisson(o["rhs"], o["mask"], *sp, dirichlet_mask=o["d"], preconditioner="jacobi")
    with pytest.raises(ValueError):
        physics.solve_poisson(o["rhs"], o["mask"], *sp, dirichlet_mask=o["d"], preconditioner="multigrid",
                              multigrid={"sweeps": 3})


def test_c_argument_checks_leave_outputs_unwritten(ctx):
    import ctypes as C

    from ptv_interpolation_amd import _lib

    o = oracle("g12")
    L = _lib.lib()
    shape = o["mask"].shape
    mk = np.ascontiguousarray(o["mask"]).view(np.uint8)
    dm = np.ascontiguousarray(o["d"]).view(np.uint8)
    dmp = dm.ctypes.data_as(C.POINTER(C.c_uint8))
    f = [np.ascontiguousarray(o["rhs"]) for _ in range(3)]
    good_mg = _lib.MgParams()
    bad_mg = [_lib.MgParams(-1, 0, 0, 0.0), _lib.MgParams(0, -1, 0, 0.0), _lib.MgParams(0, 0, -2, 0.0),
              _lib.MgParams(0, 0, 0, float("nan")), _lib.MgParams(0, 0, 0, -0.5), _lib.MgParams(0, 0, 0, float("inf"))]
    bad_prm = [dict(dx=0.0), dict(dz=float("nan")), dict(maxiter=-1), dict(rtol=float("nan")), dict(nx=0),
               dict(mask=False)]
    cases = [(dict(), m, _lib.PTV_E_ARG) for m in bad_mg] + [(p, good_mg, _lib.PTV_E_ARG) for p in bad_prm]
    for case, mgp, code in cases:
        kw = dict(case)
        prm = ctx._pressure_params(shape, mk.ctypes.data if kw.pop("mask", True) else 0, kw.pop("dx", 1.0), 1.0,
                                   kw.pop("dz", 1.0), 1e-3, 0.0, anchor="outlet", maxiter=kw.pop("maxiter", 10),
                                   rtol=kw.pop("rtol", 1e-10))
        if "nx" in kw:
            prm.nx = kw.pop("nx")
        out = np.full(shape, 7.0)
        st, mst = _lib.PressureStats(), _lib.MgStats()
        calls = [lambda: L.ptv_poisson_mg_apply(ctx.h, C.byref(prm), C.byref(mgp), dmp, _lib.as_dp(f[0]), _lib.as_dp(out),
                                                C.byref(mst)),
                 lambda: L.ptv_poisson_solve_mg(ctx.h, C.byref(prm), _lib.as_dp(f[0]), None, None, None, dmp,
                                                _lib.as_dp(out), C.byref(mgp), C.byref(st), C.byref(mst)),
                 lambda: L.ptv_pressure_recover_mg(ctx.h, C.byref(prm), *map(_lib.as_dp, f), _lib.as_dp(out),
                                                   C.byref(mgp), C.byref(st), C.byref(mst))]
        for call in calls:
            assert call() == code, (case, mgp.max_levels, mgp.nu, mgp.coarse_sweeps, mgp.omega)
            assert (out == 7.0).all()
    # the LSQR branches are refused, with a message, before anything is written
    out = np.full(shape, 7.0)
    st, mst = _lib.PressureStats(), _lib.MgStats()
    prm = ctx._pressure_params(shape, mk.ctypes.data, 1.0, 1.0, 1.0, 1e-3, 0.0, anchor="none")
    assert L.ptv_poisson_solve_mg(ctx.h, C.byref(prm), _lib.as_dp(f[0]), None, None, None, None, _lib.as_dp(out),
                                  None, C.byref(st), C.byref(mst)) == _lib.PTV_E_UNSUPPORTED
    assert b"LSQR" in L.ptv_last_error()
    assert L.ptv_pressure_recover_mg(ctx.h, C.byref(prm), *map(_lib.as_dp, f), _lib.as_dp(out), None, C.byref(st),
                                     C.byref(mst)) == _lib.PTV_E_UNSUPPORTED
    assert L.ptv_poisson_mg_apply(ctx.h, C.byref(prm), None, dmp, None, _lib.as_dp(out), None) == _lib.PTV_E_ARG
    assert (out == 7.0).all()
