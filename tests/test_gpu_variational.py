"""The GPU variational divergence cleaning (csrc/ptv_variational.hip) against the reference's
fixtures (tests/golden/var_*.npz) and the CPU oracle (tests/_variational_ref.py).

The unit of every normwise comparison is the gap between the oracle's two orderings of the same
arithmetic (``order_gap``: the explicit CSR matrix against the matrix-free stencil), with a floor of
2**-52; the device, a third ordering, is granted FACTOR = 10 such units, the factor the projection
method's tests use.  The operator tests are componentwise against an np.longdouble product:
* A x: 16 roundings on the longest path (a 9-term inner sum, a 3-term outer sum, the lambda product
  and the identity add), as a multiple of 2**-53 (|x| + lambda |D^T| |D| |x|);
* D x: 9 products rounded once each and at most 8 additions on the path of any one of them: 9
  roundings, gamma_9 = 9u / (1 - 9u) with u = 2**-53, times |D| |x|.

``PTV_VARIATIONAL_DRY_RUN=1`` lets the oracle's stencil ordering answer in the GPU's place, to check
the oracle-side logic of this file on a CPU; tests of the library itself skip in that mode only.
"""
import glob
import os

import numpy as np
import pytest

import _variational_ref as vref
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

FACTOR = 10.0
EPS = 2.0 ** -52
U = 2.0 ** -53
SP = (1.0, 1.25, 0.8)  # dx, dy, dz
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "var_*.npz")))
DRY_RUN = os.environ.get("PTV_VARIATIONAL_DRY_RUN") == "1"


class _StencilStandIn:
    """Dry run only: the oracle's second ordering answers in the GPU's place."""

    def clean_variational(self, u, v, w, mask, dx, dy, dz, lambda_reg=1e3, rtol=1e-8, maxiter=2000):
        out, itn, info = vref.solve(u, v, w, mask, dx, dy, dz, lambda_reg, rtol, maxiter, form="stencil")
        mean = lambda f: float(np.mean(np.abs(cpu_ref.consistent_divergence(*f, mask, dx, dy, dz)[mask])))  # noqa: E731
        return tuple(out), {"n_fluid": int(mask.sum()), "itn": itn, "info": info,
                            "mean_abs_div_initial": mean((u, v, w)), "mean_abs_div_final": mean(out)}


@pytest.fixture(scope="module")
def ctx():
    if DRY_RUN:
        return _StencilStandIn()
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def needs_library():
    if DRY_RUN:
        pytest.skip("dry run: no library call on a CPU")


_golden = {}


def golden(case):
    if case not in _golden:
        g = np.load(os.path.join(GOLDEN, f"var_{case}.npz"), allow_pickle=False)
        _golden[case] = {k: g[k] for k in g.files}
    return _golden[case]


def spacings(g):
    return float(g["dx"]), float(g["dy"]), float(g["dz"])


def make_fields(shape, seed):
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    u = np.sin(X / 5.0) + 0.3 * np.cos(Y / 3.0) + 0.1 * rng.standard_normal(shape)
    v = np.cos(Y / 4.0) * np.sin(Z / 3.0) + 0.1 * rng.standard_normal(shape)
    w = 1.0 + 0.2 * np.sin(Z / 2.0 + X / 7.0) + 0.1 * rng.standard_normal(shape)
    return [u, v, w]


def uniform_mask(shape, p, seed):
    return np.random.default_rng(10_000 + seed).uniform(size=shape) < p


_oracle = {}


def oracle(key, f, mask, sp=SP, **kw):
    """(csr result, stencil result, unit) of a case, computed once per module and left unchanged;
    each result is (fields, itn, info)."""
    if key not in _oracle:
        a = vref.solve(*f, mask, *sp, form="csr", **kw)
        b = vref.solve(*f, mask, *sp, form="stencil", **kw)
        nan = np.isnan(np.stack(a[0])).any()
        _oracle[key] = (a, b, EPS if nan else max(vref.order_gap(a[0], b[0]), EPS))
    return _oracle[key]


def field_ratio(label, got, ref, unit, mask):
    g, r = np.stack(got), np.stack(ref)
    assert np.all(g[:, ~mask] == 0.0) and not np.signbit(g[:, ~mask]).any(), f"{label}: solid voxels"
    den = float(np.linalg.norm(r.ravel()))
    diff = float(np.linalg.norm((g - r).ravel())) / (den if den > 0 else 1.0)
    print(f"variational {label}: fields {diff:.3e} / unit {unit:.3e} = {diff / unit:.3f}")
    assert diff <= FACTOR * unit, label
    return diff / unit


def run(ctx, key, f, mask, sp=SP, **kw):
    """A GPU solve against the oracle of the same arguments: same itn and info, fields within the bar."""
    (ref, itn, info), (_, itn2, info2), unit = oracle(key, f, mask, sp, **kw)
    assert (itn, info) == (itn2, info2), f"{key}: the two CPU orderings stop differently"
    got, st = ctx.clean_variational(*f, mask, *sp, **kw)
    print(f"variational {key}: itn {st['itn']} info {st['info']} (CPU {itn} {info})")
    assert (st["itn"], st["info"]) == (itn, info), key
    assert st["n_fluid"] == int(mask.sum())
    field_ratio(key, got, ref, unit, mask)
    return got, st


# ---- 1. the operators against extended precision ------------------------------------------------
@pytest.mark.parametrize("case, sp", [(c, None) for c in CASES] + [("g12", (1e-3, 1e-3, 1e-3)), ("thin", (1e-3, 2e-3, 5e-4))])
def test_operators_against_longdouble(ctx, case, sp):
    needs_library()
    g = golden(case)
    mask, lam = g["mask"], float(g["lambda_reg"])
    sp = spacings(g) if sp is None else sp
    x = [g["ax_xu"], g["ax_xv"], g["ax_xw"]]
    de, ye, dmag, ymag = vref.exact_products(x, mask, *sp, lam)
    # solid entries of x must not be read: poison them
    xp = [np.where(mask, a, np.nan) for a in x]
    y = ctx.variational_apply(*xp, mask, *sp, lam)
    d = ctx.divergence_operator_apply(*xp, mask, *sp)
    worst = 0.0
    for k in range(3):
        assert np.all(y[k][~mask] == 0.0)
        err = np.abs(y[k].astype(np.longdouble) - ye[k])[mask]
        bound = (U * ymag[k])[mask]
        assert np.all(err[bound == 0] == 0)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"variational operator {case} {sp}: A x worst error {worst:.3f} x 2^-53 (|x| + lambda |D^T||D||x|), bar 16")
    assert worst <= 16.0
    assert np.all(d[~mask] == 0.0)
    err = np.abs(d.astype(np.longdouble) - de)[mask]
    bound = (U * dmag)[mask]
    assert np.all(err[bound == 0] == 0)
    worst_d = float(np.max(err[bound > 0] / bound[bound > 0]))
    print(f"variational operator {case} {sp}: D x worst error {worst_d:.3f} x 2^-53 |D||x|, bar gamma_9 / u")
    assert worst_d <= 9.0 / (1.0 - 9.0 * U)
    if sp == spacings(g):  # the recorded product of the reference's explicit matrix, same bar
        for k, name in enumerate("uvw"):
            err = np.abs(y[k] - g[f"ax_y{name}"])[mask]
            assert np.all(err <= 2 * 16 * (U * ymag[k])[mask].astype(np.float64))


# ---- 2. full solves on every fixture ------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_full_solve(ctx, case):
    g = golden(case)
    mask, sp = g["mask"], spacings(g)
    unit = max(float(g["order_gap"]), EPS)
    got, st = ctx.clean_variational(g["u"], g["v"], g["w"], mask, *sp, lambda_reg=float(g["lambda_reg"]))
    print(f"variational full {case}: itn {st['itn']} info {st['info']} (reference {int(g['itn'])} {int(g['info'])})")
    assert (st["itn"], st["info"]) == (int(g["itn"]), int(g["info"]))
    assert st["n_fluid"] == int(mask.sum())
    field_ratio(f"full {case}", got, [g["u_c"], g["v_c"], g["w_c"]], unit, mask)
    for key in ("mean_abs_div_initial", "mean_abs_div_final"):
        want = float(g[key])
        r = abs(st[key] - want) / want / unit
        print(f"variational full {case} {key}: {st[key]:.6e} vs {want:.6e}: {r:.3f} units")
        assert r <= FACTOR, (case, key)


# ---- 3. truncated solves around the polling batch -----------------------------------------------
@pytest.mark.parametrize("maxiter", [1, 2, 7, 8, 9, 16, 17])
def test_truncated_solve(ctx, maxiter):
    g = golden("g12")
    f = [g["u"], g["v"], g["w"]]
    got, st = run(ctx, f"trunc {maxiter}", f, g["mask"], spacings(g), lambda_reg=1e3, maxiter=maxiter)
    assert st["info"] == maxiter and st["itn"] == maxiter


# ---- 4. the stop rules --------------------------------------------------------------------------
def test_lambda_zero_no_test_after_the_last_step(ctx):
    g = golden("iso")
    f, mask = [g["u"], g["v"], g["w"]], g["mask"]
    got, st = run(ctx, "lam0 maxiter1", f, mask, lambda_reg=0.0, maxiter=1)
    assert st["info"] == 1 and st["itn"] == 1  # r is 0, and nothing looks
    for a, b in zip(got, f):
        assert np.array_equal(a[mask], b[mask])
    got, st = run(ctx, "lam0 maxiter2", f, mask, lambda_reg=0.0, maxiter=2)
    assert st["info"] == 0 and st["itn"] == 1


def test_zero_rhs_and_zero_maxiter(ctx):
    g = golden("iso")
    f, mask = [g["u"], g["v"], g["w"]], g["mask"]
    z = [np.zeros_like(a) for a in f]
    got, st = run(ctx, "b0", z, mask)
    assert st["info"] == 0 and st["itn"] == 0 and not np.stack(got).any()
    got, st = run(ctx, "maxiter0", f, mask, maxiter=0)
    assert st["info"] == 0 and st["itn"] == 0 and not np.stack(got).any()


def test_rtol_zero_runs_to_maxiter(ctx):
    g = golden("thin")
    got, st = run(ctx, "rtol0", [g["u"], g["v"], g["w"]], g["mask"], lambda_reg=200.0, rtol=0.0, maxiter=20)
    assert st["info"] == 20 and st["itn"] == 20


def test_nan_in_a_fluid_voxel(ctx):
    g = golden("iso")
    mask = g["mask"]
    f = [g["u"].copy(), g["v"].copy(), g["w"].copy()]
    at = tuple(np.argwhere(mask)[7])
    f[1][at] = np.nan
    ref, itn, info = vref.solve(*f, mask, *SP, maxiter=5)
    assert info == 5 and all(np.isnan(a[mask]).all() for a in ref)  # what the reference's solver returns
    got, st = ctx.clean_variational(*f, mask, *SP, maxiter=5)
    assert st["info"] == 5
    for a in got:
        assert np.isnan(a[mask]).all() and np.all(a[~mask] == 0.0)


def test_nan_in_a_solid_voxel_changes_nothing(ctx):
    g = golden("iso")
    mask = g["mask"]
    f = [g["u"], g["v"], g["w"]]
    want, st0 = ctx.clean_variational(*f, mask, *SP, maxiter=9)
    p = [np.where(mask, a, np.nan) for a in f]
    got, st1 = ctx.clean_variational(*p, mask, *SP, maxiter=9)
    assert np.stack(got).tobytes() == np.stack(want).tobytes()
    for k in ("itn", "info", "mean_abs_div_final"):
        assert st0[k] == st1[k], k
    # the report's initial divergence is the reference's stencil on the caller's fields, whose
    # minus-side face average reads the solid neighbour of a fluid voxel (physics.py:44-46)
    want = float(np.mean(np.abs(cpu_ref.consistent_divergence(*p, mask, *SP)[mask])))
    assert np.isnan(want) and np.isnan(st1["mean_abs_div_initial"])


# ---- 5. layout ----------------------------------------------------------------------------------
def _dev_call(ctx, f, mask_u8, sp=SP, offset_fields=0, offset_mask=0, in_place=False, fill=0.0, **kw):
    """clean_variational_dev on torch tensors; the fields start ``offset_fields`` float64 into their
    allocation, the mask ``offset_mask`` bytes into its.  Returns ((u, v, w) as numpy, stats)."""
    import torch

    dev = torch.device("cuda", 0)
    nz, ny, nx = f[0].shape
    n = f[0].size

    def put(a, off, dtype):
        base = torch.zeros(n + off, dtype=dtype, device=dev)
        base[off:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return base, base[off:]

    held = [put(a, offset_fields, torch.float64) for a in f]
    mbase, m = put(mask_u8, offset_mask, torch.uint8)
    outs = held if in_place else [put(np.full(n, fill), offset_fields, torch.float64) for _ in f]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for _, t in held]
    assert all(p % 16 == 8 * (offset_fields % 2) for p in ptrs) and m.data_ptr() % 2 == offset_mask % 2
    try:
        st = ctx.clean_variational_dev(nx, ny, nz, ptrs, m.data_ptr(), [t.data_ptr() for _, t in outs], *sp, **kw)
    finally:
        torch.cuda.synchronize()
        res = [t.cpu().numpy().reshape(nz, ny, nx) for _, t in outs]
        _dev_call.last = res
    return res, st


def test_in_place_host_and_dev_and_repeats_agree_bit_for_bit(ctx):
    needs_library()
    g = golden("g12")
    f, mask, sp = [g["u"], g["v"], g["w"]], g["mask"], spacings(g)
    host, st = ctx.clean_variational(*f, mask, *sp, maxiter=9)
    again, st2 = ctx.clean_variational(*f, mask, *sp, maxiter=9)
    out, st3 = _dev_call(ctx, f, mask.view(np.uint8), sp, maxiter=9)
    inp, st4 = _dev_call(ctx, f, mask.view(np.uint8), sp, in_place=True, maxiter=9)
    want = np.stack(host).tobytes()
    for name, r, s in (("second call", again, st2), ("_dev", out, st3), ("in place", inp, st4)):
        assert np.stack(r).tobytes() == want, name
        for k in ("itn", "info", "bnorm", "rnorm", "mean_abs_div_initial", "mean_abs_div_final"):
            assert s[k] == st[k], (name, k)


@pytest.mark.parametrize("shape, off_f, off_m", [((9, 11, 13), 0, 0), ((9, 11, 14), 1, 0), ((9, 11, 14), 0, 1),
                                                 ((9, 11, 14), 0, 0)],
                         ids=["odd_nx", "fields_8_off", "mask_1_off", "aligned"])
def test_one_wide_path(ctx, shape, off_f, off_m):
    """Odd nx, fields 8 bytes off 16-byte alignment and a mask 1 byte off 2-byte alignment all take
    the one-wide kernels; (9, 11, 14) aligned is the two-wide control.  1287 / 1386 voxels: 2 blocks."""
    needs_library()
    f, mask = make_fields(shape, 3), uniform_mask(shape, 0.8, 3)
    (ref, itn, info), _, unit = oracle(f"onewide {shape}", f, mask, maxiter=9)
    got, st = _dev_call(ctx, f, mask.view(np.uint8), offset_fields=off_f, offset_mask=off_m, maxiter=9)
    assert (st["itn"], st["info"]) == (itn, info) == (9, 9)
    field_ratio(f"onewide {shape} {off_f} {off_m}", got, ref, unit, mask)


def test_mask_bytes_1_2_255(ctx):
    needs_library()
    shape = (5, 6, 8)
    f, mask = make_fields(shape, 4), uniform_mask(shape, 0.7, 4)
    want, st = _dev_call(ctx, f, mask.view(np.uint8), maxiter=9)
    for byte in (2, 255):
        got, st2 = _dev_call(ctx, f, mask.view(np.uint8) * np.uint8(byte), maxiter=9)
        assert np.stack(got).tobytes() == np.stack(want).tobytes(), byte
        for k in ("itn", "info", "rnorm", "n_fluid", "mean_abs_div_final"):
            assert st2[k] == st[k], (byte, k)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (1, 1, 2), (2, 6, 7), (6, 1, 1)],
                         ids=["point", "line_x", "two_voxels", "sheet_two_thick", "line_z"])
def test_extents_of_one(ctx, shape):
    f, mask = make_fields(shape, 5), np.ones(shape, bool)
    got, st = run(ctx, f"extent {shape}", f, mask, lambda_reg=50.0, maxiter=60)
    assert st["info"] == 0
    if shape == (1, 1, 1):  # every neighbour is outside the grid: c = 0, D = 0, A = I
        assert st["itn"] == 1 and all(np.array_equal(a, b) for a, b in zip(got, f))


def test_two_disconnected_regions(ctx):
    shape = (6, 7, 9)
    f, mask = make_fields(shape, 6), uniform_mask(shape, 0.9, 6)
    mask[:, :, 4] = False  # a solid wall between x < 4 and x > 4
    run(ctx, "two regions", f, mask, lambda_reg=1e3, maxiter=12)


@pytest.mark.parametrize("shape", [(66, 64, 63), (65, 90, 90)], ids=["vec1_260_blocks", "vec2_258_blocks"])
def test_more_than_256_partials(ctx, shape):
    """The second stride step of the one-block sum over the partials, for rho, p.q and the three
    rows of the divergence statistics (a sum that took one step only would be off by 1e-2)."""
    f, mask = make_fields(shape, 7), uniform_mask(shape, 0.9, 7)
    got, st = run(ctx, f"partials {shape}", f, mask, lambda_reg=200.0, maxiter=3)
    assert st["info"] == 3
    n = int(mask.sum())
    for key, fld in (("mean_abs_div_initial", f), ("mean_abs_div_final", got)):
        want = float(np.mean(np.abs(cpu_ref.consistent_divergence(*fld, mask, *SP)[mask])))
        err = abs(st[key] - want) / want
        print(f"variational partials {shape} {key}: rel err {err:.3e} / bound {n * U:.3e}")
        assert err <= n * U  # two summation orders of n terms of one sign


# ---- 6. the C argument checks -------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_alone(ctx):
    needs_library()
    shape = (3, 4, 6)
    f, mask = make_fields(shape, 9), uniform_mask(shape, 0.8, 9)
    m8 = mask.view(np.uint8)
    nan, inf = float("nan"), float("inf")
    bad = [(ValueError, dict(mask_u8=np.zeros(shape, np.uint8))),
           (ValueError, dict(sp=(0.0, 1.25, 0.8))), (ValueError, dict(sp=(1.0, -1.25, 0.8))),
           (ValueError, dict(sp=(1.0, 1.25, nan))), (ValueError, dict(sp=(inf, 1.25, 0.8))),
           (ValueError, dict(lambda_reg=nan)), (ValueError, dict(lambda_reg=inf)),
           (ValueError, dict(rtol=nan)), (ValueError, dict(rtol=inf)), (ValueError, dict(maxiter=-1)),
           (NotImplementedError, dict(lambda_reg=-1.0))]
    for exc, kw in bad:
        kw = dict(kw)
        mk = kw.pop("mask_u8", m8)
        with pytest.raises(exc):
            _dev_call(ctx, f, mk, fill=7.5, **kw)
        assert all(np.all(a == 7.5) for a in _dev_call.last), kw
    got, st = _dev_call(ctx, f, m8, fill=7.5, maxiter=2)  # the same call is accepted once valid
    assert st["info"] == 2 and all(np.all(a[~mask] == 0.0) for a in got)


# ---- 7. the Python entry point ------------------------------------------------------------------
def test_python_entry_point_report(ctx, capsys):
    needs_library()
    from ptv_interpolation_amd import physics

    g = golden("g12_l200")
    mask, sp = g["mask"], spacings(g)
    capsys.readouterr()
    out = physics.clean_divergence_variational(g["u"], g["v"], g["w"], mask, *sp, lambda_reg=200)
    text = capsys.readouterr().out
    n = 3 * int(mask.sum())
    mi, mf = float(g["mean_abs_div_initial"]), float(g["mean_abs_div_final"])
    want = (f"Starting Variational Divergence Cleaning (lambda=200)...\n"
            f"  Solving Variational System (A: {n}x{n})...\n"
            "\n" + "=" * 40 + "\nVARIATIONAL CLEANING COMPLETE\n"
            f"Mean Abs Div (Initial): {mi:.6e}\nMean Abs Div (Final):   {mf:.6e}\n"
            f"Total Reduction:        {mi / mf:.2f}x\n" + "=" * 40 + "\n\n")
    assert text == want
    st = physics.clean_divergence_variational.last_stats
    assert (st["itn"], st["info"], st["n_fluid"]) == (int(g["itn"]), 0, int(mask.sum()))
    assert st["ms_total"] > 0 and st["ms_solve"] > 0 and st["ms_iter_median"] > 0 and st["bnorm"] > 0
    field_ratio("python entry", out, [g["u_c"], g["v_c"], g["w_c"]], max(float(g["order_gap"]), EPS), mask)
    # info > 0: a NaN in a fluid voxel never converges, and the reference's warning line appears
    u = g["u"].copy()
    u[tuple(np.argwhere(mask)[0])] = np.nan
    physics.clean_divergence_variational(u, g["v"], g["w"], mask, *sp, lambda_reg=200)
    text = capsys.readouterr().out
    assert "  Warning: CG did not converge after 2000 iterations.\n" in text
    assert physics.clean_divergence_variational.last_stats["info"] == 2000
