"""The GPU pressure recovery (csrc/ptv_pressure.hip) against the reference's fixtures
(tests/golden/pressure_*.npz) and the CPU restatement (tests/_pressure_ref.py).

The force field and the force divergence are elementwise chains: every comparison of them demands
identical bits at every voxel.  The unit of every normwise comparison of a pressure is the fixture's
``order_gap`` (the reference's CSR matrix against the numpy slice operator); the device, a third
ordering, is granted FACTOR = 10 such units, the factor of the two cleaning solvers' tests.
"""
import glob
import os

import numpy as np
import pytest

import _pressure_ref as pref

pytestmark = pytest.mark.gpu

FACTOR = 10.0
SP = (1.0, 1.25, 0.8)  # dx, dy, dz
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("pressure_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "pressure_*.npz")))
CG_CASES = [c for c in CASES if c != "none"]


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


_golden = {}


def golden(name):
    if name not in _golden:
        g = np.load(os.path.join(GOLDEN, f"pressure_{name}.npz"), allow_pickle=False)
        d = {k: g[k] for k in g.files}
        for k in ("wall_bc", "anchor", "flow_direction"):
            d[k] = str(d[k])
        for k in ("mu", "rho", "dx", "dy", "dz", "order_gap"):
            d[k] = float(d[k])
        _golden[name] = d
    return _golden[name]


def sp(g):
    return g["dx"], g["dy"], g["dz"]


def test_abi_sizes(ctx):
    from ptv_interpolation_amd import _lib

    c, py = _lib.abi_sizes9()
    assert c == py


@pytest.mark.parametrize("name", CASES)
def test_force_field_and_divergence_bits(ctx, name):
    g = golden(name)
    f, st = ctx.force_field(g["u"], g["v"], g["w"], g["mask"], *sp(g), g["mu"], g["rho"])
    for a, key in zip(f, ("fx", "fy", "fz")):
        assert np.array_equal(a, g[key]), key
    d = ctx.force_divergence(*f, g["mask"], *sp(g), g["wall_bc"])
    assert np.array_equal(d, g["rhs"])  # every voxel: under 'inhomogeneous' the solid ones too
    n = int(g["mask"].sum())
    assert st["n_fluid"] == n
    means = np.array([st["sum_abs_fx"], st["sum_abs_fy"], st["sum_abs_fz"]]) / n
    assert np.allclose(means, g["means"], rtol=n * 2.0 ** -53, atol=0)  # a reordered sum of n positive terms
    assert np.isclose(st["sum_w"], g["w"][g["mask"]].sum(), rtol=0, atol=n * 2.0 ** -53 * np.abs(g["w"]).sum())


def _shape_cases():
    rng = np.random.default_rng(11)
    out = {}

    def fields(shape):
        return [rng.standard_normal(shape).astype(np.float32).astype(np.float64) for _ in range(3)]

    ch = np.zeros((6, 7, 8), bool)
    ch[:, 3, 4] = True
    ch[2, :, 2] = True
    out["channels"] = (ch, fields(ch.shape))  # one-voxel-wide channels: no bulk voxel
    out["all_fluid"] = (np.ones((5, 6, 7), bool), fields((5, 6, 7)))
    out["all_solid"] = (np.zeros((5, 6, 7), bool), fields((5, 6, 7)))
    for shape in ((1, 6, 7), (5, 1, 7), (5, 6, 1), (1, 1, 1), (2, 5, 6)):
        out["x".join(map(str, shape))] = (rng.uniform(size=shape) > 0.2, fields(shape))
    return out


SHAPES = _shape_cases()


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("wall_bc", ["zero-neumann", "inhomogeneous"])
def test_force_shapes(ctx, name, wall_bc):
    mask, (u, v, w) = SHAPES[name]
    rho = 0.0 if min(mask.shape) < 2 else 1.5
    f, st = ctx.force_field(u, v, w, mask, *SP, 1e-3, rho)
    ref = pref.force_field(u, v, w, *SP, 1e-3, rho, mask)
    for a, b in zip(f, ref):
        assert np.array_equal(a, b)
    assert st["n_fluid"] == int(mask.sum())
    d = ctx.force_divergence(*f, mask, *SP, wall_bc)
    assert np.array_equal(d, pref.force_divergence(*ref, mask, *SP, wall_bc))


@pytest.mark.parametrize("byte", [2, 255])
def test_mask_bytes(ctx, byte):
    g = golden("g12")
    mk = g["mask"].astype(np.uint8) * np.uint8(byte)
    f, _ = ctx.force_field(g["u"], g["v"], g["w"], mk, *sp(g), g["mu"], g["rho"])
    assert np.array_equal(f[0], g["fx"])
    assert np.array_equal(ctx.force_divergence(*f, mk, *sp(g), "inhomogeneous"),
                          pref.force_divergence(*f, g["mask"], *sp(g), "inhomogeneous"))
    x, st = ctx.poisson_solve(mk, *sp(g), rhs=g["rhs"], dirichlet=g["dirichlet"].astype(np.uint8) * np.uint8(byte))
    x1, st1 = ctx.poisson_solve(g["mask"], *sp(g), rhs=g["rhs"], dirichlet=g["dirichlet"])
    assert np.array_equal(x, x1) and st["itn"] == st1["itn"]


def check_pressure(g, p, st):
    ratio = pref.normwise(p, g["p"]) / g["order_gap"]
    print(f"ratio {ratio:.3f} itn {st['itn']} (reference {int(g['itn'])} / {int(g['itn_free'])}) info {st['info']}")
    assert st["info"] == int(g["info"])
    if int(g["itn"]) == int(g["itn_free"]):
        assert st["itn"] == int(g["itn"])
    else:
        assert abs(st["itn"] - int(g["itn"])) <= 1
    assert (p[~g["mask"]] == 0).all() and (p[g["dirichlet"]] == 0).all()
    assert ratio <= FACTOR
    return ratio


@pytest.mark.parametrize("name", CASES)
def test_pressure_within_the_bar(ctx, name):
    g = golden(name)
    p, st = ctx.pressure_recover(g["u"], g["v"], g["w"], g["mask"], *sp(g), g["mu"], g["rho"], g["wall_bc"],
                                 g["anchor"], g["flow_direction"])
    assert st["n_dirichlet"] == int(g["dirichlet"].sum()) and st["n_fluid"] == int(g["mask"].sum())
    assert st["solver"] == (1 if name == "none" else 0)
    check_pressure(g, p, st)


@pytest.mark.parametrize("name", ["g12", "none"])
def test_public_functions(ctx, name, capsys):
    from ptv_interpolation_amd import physics, velocity_analysis

    g = golden(name)
    p = velocity_analysis.compute_pressure_field(g["u"], g["v"], g["w"], *sp(g), g["mu"], g["rho"], g["mask"],
                                                 g["wall_bc"], g["anchor"], g["flow_direction"])
    out = capsys.readouterr().out
    assert f"    Fx: mean={g['means'][0]: .4e}" in out and "Solving pressure Poisson equation" in out
    check_pressure(g, p, velocity_analysis.compute_pressure_field.last_stats)
    f = velocity_analysis.compute_force_field(g["u"], g["v"], g["w"], *sp(g), g["mu"], g["rho"], g["mask"])
    assert np.array_equal(f[2], g["fz"])
    assert np.array_equal(physics.compute_force_divergence(*f, g["mask"], *sp(g), g["wall_bc"]), g["rhs"])
    dm = None if name == "none" else g["dirichlet"]
    p2 = physics.solve_poisson(None, g["mask"], *sp(g), force_field=f, wall_bc=g["wall_bc"], dirichlet_mask=dm,
                               dirichlet_values=0.0)
    assert np.array_equal(p2, p)
    p3 = physics.solve_poisson(g["rhs"], g["mask"], *sp(g), dirichlet_mask=dm)
    assert np.array_equal(p3, p)
    # float32 fields are widened exactly
    p32 = velocity_analysis.recover_pressure(*(g[k].astype(np.float32) for k in "uvw"), *sp(g), g["mu"], g["rho"],
                                             g["mask"], g["wall_bc"], g["anchor"], g["flow_direction"])[0]
    assert p32.dtype == np.float64 and np.array_equal(p32, p)  # the fixtures' fields are float32 values


@pytest.mark.parametrize("maxiter", [0, 1, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("name", ["g12", "empty_plane"])
def test_truncated_solves(ctx, name, maxiter):
    g = dict(golden("g12"))
    if name == "empty_plane":  # an anchor plane without a fluid voxel: CG on the singular system
        g["dirichlet"] = np.zeros_like(g["dirichlet"])
    ref, itn, info = pref.cg_solve(g["rhs"], g["mask"], g["dirichlet"], *sp(g), maxiter=maxiter)
    x, st = ctx.poisson_solve(g["mask"], *sp(g), rhs=g["rhs"], dirichlet=g["dirichlet"], maxiter=maxiter)
    assert (st["info"], st["itn"]) == (info, itn) == (maxiter, maxiter)
    assert pref.normwise(x, ref) <= FACTOR * g["order_gap"]


def test_zero_rhs_and_nan(ctx):
    g = golden("g12")
    x, st = ctx.poisson_solve(g["mask"], *sp(g), rhs=np.zeros_like(g["rhs"]), dirichlet=g["dirichlet"])
    assert not x.any() and (st["info"], st["itn"], st["bnorm"]) == (0, 0, 0.0)
    u = g["u"].copy()
    # a bulk voxel: its raw Laplacian is kept (a voxel the fill overwrites would lose the NaN, in the
    # reference too), so the force, the divergence around it and b hold NaN
    bulk = np.argwhere(pref.voxel_codes(g["mask"]) == pref.BULK)
    iz, iy, ix = bulk[len(bulk) // 2]
    u[iz, iy, ix] = np.nan
    assert np.isnan(pref.force_divergence(*pref.force_field(u, g["v"], g["w"], *sp(g), g["mu"], g["rho"], g["mask"]),
                                          g["mask"], *sp(g))[g["mask"] & ~g["dirichlet"]]).any()
    p, st = ctx.pressure_recover(u, g["v"], g["w"], g["mask"], *sp(g), g["mu"], g["rho"])
    assert np.isnan(p[g["mask"]]).all() and (p[~g["mask"]] == 0).all()
    assert (st["info"], st["itn"]) == (3000, 3000)


def test_single_plane_is_all_dirichlet(ctx):
    rng = np.random.default_rng(3)
    shape = (1, 9, 12)
    mask = rng.uniform(size=shape) > 0.3
    u, v, w = (rng.standard_normal(shape) for _ in range(3))
    p, st = ctx.pressure_recover(u, v, w, mask, *SP, 1e-3)
    assert not p.any() and (st["itn"], st["info"]) == (0, 0) and st["n_dirichlet"] == int(mask.sum())


def _dev_solve(ctx, g, maxiter, offset, in_place):
    """poisson_solve_dev on torch tensors that start ``offset`` elements into their allocations."""
    import torch

    dev = torch.device("cuda", 0)
    n = g["mask"].size

    def put(a, dtype):
        base = torch.zeros(n + offset, dtype=dtype, device=dev)
        base[offset:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return base, base[offset:]

    held = [put(g["rhs"], torch.float64), put(g["mask"].view(np.uint8), torch.uint8),
            put(g["dirichlet"].view(np.uint8), torch.uint8), put(np.full(n, 7.0), torch.float64)]
    rhs, mk, dm, out = (t for _, t in held)
    if in_place:
        out = rhs
    torch.cuda.synchronize()
    nz, ny, nx = g["mask"].shape
    st = ctx.poisson_solve_dev(nx, ny, nz, mk.data_ptr(), out.data_ptr(), *sp(g), rhs_ptr=rhs.data_ptr(),
                               dirichlet_ptr=dm.data_ptr(), maxiter=maxiter)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(g["mask"].shape), st


def test_dev_alignment_and_aliasing(ctx):
    g = golden("g12")  # nx = 14 is even: offset 1 leaves the grids 8 bytes off a 16-byte boundary
    x0, st0 = _dev_solve(ctx, g, 3000, 0, False)
    x1, st1 = _dev_solve(ctx, g, 3000, 1, False)
    x2, st2 = _dev_solve(ctx, g, 3000, 0, True)
    host, sth = ctx.poisson_solve(g["mask"], *sp(g), rhs=g["rhs"], dirichlet=g["dirichlet"])
    assert np.array_equal(x0, host) and np.array_equal(x0, x2) and st0["itn"] == st2["itn"] == sth["itn"]
    for x, st in ((x0, st0), (x1, st1)):
        check_pressure(g, x, st)


@pytest.fixture(scope="module")
def big():
    """82 x 80 x 82: more than 256 first-stage partials in both lane widths; the reference is the
    restatement truncated at 16 iterations, computed once."""
    rng = np.random.default_rng(5)
    shape = (82, 80, 82)
    Z, Y, X = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    mask = np.ones(shape, bool)
    for _ in range(12):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        mask &= (Z - c[0]) ** 2 + (Y - c[1]) ** 2 + (X - c[2]) ** 2 > rng.uniform(6, 12) ** 2
    rhs = rng.standard_normal(shape)
    d = pref.dirichlet_grid(mask, shape[0] - 1)
    g = {"mask": mask, "rhs": rhs, "dirichlet": d, "dx": SP[0], "dy": SP[1], "dz": SP[2]}
    g["ref"] = pref.cg_solve(rhs, mask, d, *SP, maxiter=16)[0]
    return g


# 16 iterations, each with two dot products of n = 5e5 terms summed in another order than numpy's
# pairwise sum (either order errs by at most about log2(n) = 19 units of 2**-53 relative on these
# sums of squares) and a 6-term stencil sum: 16 * (2 * 19 + 6) units, doubled for the two runs compared
BIG_TOL = 2 * 16 * (2 * 19 + 6) * 2.0 ** -53


def test_many_partials_both_widths(ctx, big):
    n = big["mask"].size
    assert n // (256 * 4 * 2) > 256  # blocks of a two-wide pass
    x2, st2 = _dev_solve(ctx, big, 16, 0, False)  # aligned, nx even: two x per lane
    x1, st1 = _dev_solve(ctx, big, 16, 1, False)  # 8 bytes off: one x per lane
    again, _ = _dev_solve(ctx, big, 16, 0, False)
    assert np.array_equal(x2, again)  # fixed-order sums: a call repeats bit for bit
    for x, st in ((x2, st2), (x1, st1)):
        r = pref.normwise(x, big["ref"])
        print(f"normwise {r:.3e} (tolerance {BIG_TOL:.3e})")
        assert (st["itn"], st["info"]) == (16, 16)
        assert r <= BIG_TOL
        assert (x[~big["mask"]] == 0).all() and (x[big["dirichlet"]] == 0).all()


def test_consumers_read_the_resident_pressure(ctx):
    """The recovered pressure stays on the device for the drag and the pressure-based permeability."""
    import torch

    g = golden("g12")
    dev = torch.device("cuda", 0)
    nz, ny, nx = g["mask"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in "uvw"}
    mk = torch.from_numpy(g["mask"].view(np.uint8).copy()).to(dev)
    p = torch.full((nz, ny, nx), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = ctx.pressure_recover_dev(nx, ny, nz, [t[k].data_ptr() for k in "uvw"], mk.data_ptr(), p.data_ptr(), *sp(g),
                                  g["mu"], g["rho"], g["wall_bc"], g["anchor"], g["flow_direction"])
    torch.cuda.synchronize()
    host = p.cpu().numpy()
    check_pressure(g, host, st)
    assert ctx.gradient_sums_dev(nx, ny, nz, p.data_ptr(), *sp(g)) == ctx.gradient_sums(host, *sp(g))
    labels = torch.from_numpy((~g["mask"]).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    rec, _ = ctx.interface_drag_dev(nx, ny, nz, labels.data_ptr(), [t[k].data_ptr() for k in "uvw"], p.data_ptr(),
                                    g["mu"], *sp(g), [1])
    ref, _ = ctx.interface_drag((~g["mask"]).astype(np.int32), g["u"], g["v"], g["w"], host, g["mu"], *sp(g), [1])
    assert np.array_equal(rec, ref)


def test_c_argument_checks_leave_outputs_unwritten(ctx):
    import ctypes as C

    from ptv_interpolation_amd import _lib

    g = golden("g12")
    L = _lib.lib()
    mk = np.ascontiguousarray(g["mask"]).view(np.uint8)
    f = [np.ascontiguousarray(g[k]) for k in "uvw"]
    bad = [dict(dx=0.0), dict(dy=-1.0), dict(dz=float("nan")), dict(mu=float("inf")), dict(wall_bc_code=5),
           dict(maxiter=-1), dict(rtol=float("nan")), dict(nx=0), dict(mask=False)]
    for case in bad:
        kw = dict(case)
        prm = ctx._pressure_params(g["mask"].shape, mk.ctypes.data if kw.pop("mask", True) else 0,
                                   kw.pop("dx", 1.0), kw.pop("dy", 1.0), kw.pop("dz", 1.0), kw.pop("mu", 1e-3), 0.0,
                                   maxiter=kw.pop("maxiter", 10), rtol=kw.pop("rtol", 1e-10))
        if "wall_bc_code" in kw:
            prm.wall_bc = kw.pop("wall_bc_code")
        if "nx" in kw:
            prm.nx = kw.pop("nx")
        out = [np.full(g["mask"].shape, 7.0) for _ in range(3)]
        st = _lib.PressureStats()
        calls = [lambda: L.ptv_force_field(ctx.h, C.byref(prm), *map(_lib.as_dp, f), *map(_lib.as_dp, out), C.byref(st)),
                 lambda: L.ptv_force_divergence(ctx.h, C.byref(prm), *map(_lib.as_dp, f), _lib.as_dp(out[0])),
                 lambda: L.ptv_poisson_solve(ctx.h, C.byref(prm), _lib.as_dp(f[0]), None, None, None, None,
                                             _lib.as_dp(out[0]), C.byref(st)),
                 lambda: L.ptv_pressure_recover(ctx.h, C.byref(prm), *map(_lib.as_dp, f), _lib.as_dp(out[0]),
                                                C.byref(st))]
        for call in calls:
            assert call() == _lib.PTV_E_ARG, case
            assert all((o == 7.0).all() for o in out), case
    prm = ctx._pressure_params(g["mask"].shape, mk.ctypes.data, 1.0, 1.0, 1.0)
    out = np.full(g["mask"].shape, 7.0)
    assert L.ptv_force_divergence(ctx.h, C.byref(prm), _lib.as_dp(f[0]), None, _lib.as_dp(f[2]),
                                  _lib.as_dp(out)) == _lib.PTV_E_ARG
    assert L.ptv_poisson_solve(ctx.h, C.byref(prm), None, None, None, None, None, _lib.as_dp(out), None) == _lib.PTV_E_ARG
    assert (out == 7.0).all()
    # rho > 0 on a grid one voxel thick: np.gradient raises in the reference
    thin = ctx._pressure_params((1, 4, 5), mk.ctypes.data, 1.0, 1.0, 1.0, 1e-3, 1.0)
    assert L.ptv_force_field(ctx.h, C.byref(thin), *map(_lib.as_dp, f), *map(_lib.as_dp, [out, out, out]),
                             None) == _lib.PTV_E_ARG
    assert (out == 7.0).all()
