"""Every stop path and edge of the GPU divergence cleaning (csrc/ptv_clean.hip) against the CPU oracle
``oracle.cpu_ref.clean_projection`` (scipy's lsqr on the masked Laplacian), computed at test time on
seeded inputs.  tests/test_gpu_clean.py holds the five stored fixtures (istop 1, 2, 7 after 555-3000
iterations); this file holds what they never run.

The bar.  The unit of every solver output is the gap between the oracle's two CPU orderings of the
same call (CSR matrix / matrix-free stencil, ``cpu_ref.clean_order_gap``); where the two agree to
the bit the unit is 2**-52 relative.  The GPU must lie within FACTOR = 10 units of the CSR run, the
project's factor (tests/test_gpu_clean.py).  Before anything is measured each test asserts that the
two CPU orderings stop every solve for the same reason; the seeds below were chosen on a CPU so
that they do, and a case that violates it fails.  Every measured ratio is printed
(profiles/clean_edges_parity.txt keeps one run's output).

``mean |div|`` is a mean of n_fluid non-negative terms that the GPU sums in another order than
numpy; the worst-case relative error of such a sum is n_fluid * 2**-53, so that much is granted on
top of the solver's units wherever a mean |div| is compared.  The mid-plane flux is a signed sum of
rows = ny * nz terms: |error| <= rows * 2**-53 * sum|u_mid| * |dy dz|.

What each test would catch (a reading of the kernel, no broken kernel was built):

* truncated LSQR (iter_lim 1..17): after so few steps the two CPU orderings differ by some 1e-16,
  so t1 and t2 swapped, a missing rotation, a stale rho or phibar or psi in rnorm each move x or
  rnorm by many orders of magnitude more than 10 units.  iter_lim 7, 8, 9, 16, 17 straddle the
  polling batch (kPoll = 8): a stop test that fires one iteration late or a batch that enqueues
  one iteration too many changes itn and x.  damp = 0 runs the undamped branch of PH_ALFA.
* stop reasons 3, 4, 5: anorm (test2, t1), xnorm (t1), acond = anorm * sqrt(ddnorm) (test3) only
  feed the stopping tests.  An anorm without dampsq or a ddnorm that misses a term moves the
  iteration at which 1 + t1 <= 1, 1 + test2 <= 1 or test3 <= 1e-8 first holds, by more than the
  spread of the two CPU orderings plus ITN_MARGIN, or flips the istop.  istop 6 cannot be reached
  with conlim = 1e8: 1 + test3 <= 1 implies test3 <= ctol, and the istop 3 assignment follows the
  istop 6 one in lsqr (and in PH_TEST), so no input stops with 6 in either ordering; left out.
* istop 0 three ways (b = 0, A = 0 with b != 0, iter_lim = 0), S_SKIPV, nan_stop: exact outputs.
* more than 256 first-stage partials: a k_scalar that takes only one stride step drops the blocks
  past 256 from beta, alfa and ddnorm: wrong at the first iteration by a relative 1e-2, not 1e-15.
* iterations = 18: the stats hold 16 solves; entry 15 must stay solve 16's.

A CPU-only dry run of the oracle-side logic (the matrix-free ordering standing in for the GPU, so
every istop agreement condition and every bound is evaluated once without a device):
``PTV_CLEAN_EDGES_DRY_RUN=1 python -m pytest tests/test_gpu_clean_edges.py``; the tests that need
the library itself (device pointers, the C argument checks, the printed report) skip in that mode
only.
"""
import os

import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu

FACTOR = 10.0
EPS = 2.0 ** -52
SP = (1.0, 1.25, 0.8)  # dx, dy, dz
MAX_OUTER = 16
# itn of a tolerance or machine-precision stop (istop 1..5) may leave the range of the two CPU
# orderings by this much.  It is the largest spread between the two CPU orderings measured on such
# cases: 0..3 iterations over the cases of this file (printed with every case), 0..12 over the wider
# seed probe that accompanied these tests.  A third ordering of the same arithmetic is granted, on
# either side of the CPU range, what the two CPU orderings were seen to differ by.
ITN_MARGIN = 12
DRY_RUN = os.environ.get("PTV_CLEAN_EDGES_DRY_RUN") == "1"


class _MatrixFreeStandIn:
    """Dry run only: the oracle's second ordering answers in the GPU's place."""

    def clean_divergence(self, u, v, w, mask, dx, dy, dz, **kw):
        f, i = cpu_ref.clean_projection(u, v, w, mask, dx, dy, dz, operator=True, **kw)
        st = {k: i[k] for k in ("n_outer", "nan_stop", "n_fluid", "mean_abs_div_final", "flux_initial", "flux_final")}
        for k, src in (("istop", "istop"), ("itn", "itn"), ("rnorm", "r2norm"), ("mean_abs_div", "mean_abs_div")):
            st[k] = i[src][:MAX_OUTER]
        return f, st


@pytest.fixture(scope="module")
def ctx():
    if DRY_RUN:
        return _MatrixFreeStandIn()
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def needs_library():
    if DRY_RUN:
        pytest.skip("dry run: no library call on a CPU")


def printed_by(capsys, fn):
    """(result, lines printed by fn); what the test printed before stays in its output."""
    before = capsys.readouterr().out
    res = fn()
    text = capsys.readouterr().out
    print(before, end="")
    return res, text.split("\n")


# ---- seeded inputs -------------------------------------------------------------------------------
def make_fields(shape, seed):
    """Smooth fields plus 0.1 * normal noise, float64 (nz, ny, nx)."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    u = np.sin(X / 5.0) + 0.3 * np.cos(Y / 3.0) + 0.1 * rng.standard_normal(shape)
    v = np.cos(Y / 4.0) * np.sin(Z / 3.0) + 0.1 * rng.standard_normal(shape)
    w = 1.0 + 0.2 * np.sin(Z / 2.0 + X / 7.0) + 0.1 * rng.standard_normal(shape)
    return [u, v, w]


def uniform_mask(shape, p, seed):
    return np.random.default_rng(10_000 + seed).uniform(size=shape) < p


def grains_mask(shape, seed):
    """Fluid outside six random spherical grains."""
    rng = np.random.default_rng(20_000 + seed)
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.ones(shape, bool)
    for _ in range(6):
        c = rng.uniform(0, 1, 3) * np.array([nz, ny, nx])
        r = rng.uniform(0.12, 0.22) * max(min(ny, nx), 6)
        mask &= (Z - c[0]) ** 2 + (Y - c[1]) ** 2 + (X - c[2]) ** 2 > r * r
    return mask


# ---- the comparison ------------------------------------------------------------------------------
_oracle = {}


def oracle(key, f, mask, sp=SP, **kw):
    """clean_order_gap of a case, computed once per module and left unchanged."""
    if key not in _oracle:
        _oracle[key] = cpu_ref.clean_order_gap(*f, mask, *sp, **kw)
    return _oracle[key]


def rel_unit(a, b):
    """The relative gap of two CPU numbers, 2**-52 where they agree to the bit."""
    return abs(a - b) / abs(a) if a != b else EPS


def compare(label, got, st, orc, mask):
    """The GPU's ((u, v, w), stats) against the oracle's two runs: conditions, then the bar."""
    gap_f, gap_d, agree, (f_csr, i_csr), (f_free, i_free) = orc
    assert agree, f"{label}: the two CPU orderings stop differently: {i_csr['istop']} / {i_free['istop']}"
    n = min(i_csr["n_outer"], MAX_OUTER)
    assert st["n_outer"] == i_csr["n_outer"] and bool(st["nan_stop"]) == i_csr["nan_stop"]
    assert st["n_fluid"] == i_csr["n_fluid"] == int(mask.sum())
    assert st["istop"] == i_csr["istop"][:n], label
    assert len(st["itn"]) == len(st["rnorm"]) == n and len(st["mean_abs_div"]) == max(n, 1)
    for i in range(n):
        lo, hi = sorted((i_csr["itn"][i], i_free["itn"][i]))
        margin = 0 if st["istop"][i] in (0, 7) else ITN_MARGIN  # 0 and 7 fix itn: 0, iter_lim
        assert lo - margin <= st["itn"][i] <= hi + margin, (label, i, st["itn"], i_csr["itn"], i_free["itn"])
    ref, g = np.stack(f_csr), np.stack(got)
    assert g[:, ~mask].tobytes() == ref[:, ~mask].tobytes(), f"{label}: solid voxels"
    den = float(np.linalg.norm(ref.ravel()))
    diff_f = float(np.linalg.norm((g - ref).ravel())) / (den if den > 0 else 1.0)
    unit_f = gap_f if gap_f > 0 else EPS
    ratios_r = []
    for i in range(n):
        rc, rf = i_csr["r2norm"][i], i_free["r2norm"][i]
        if rc == 0.0:
            assert st["rnorm"][i] == 0.0
            ratios_r.append(0.0)
        else:
            ratios_r.append(abs(st["rnorm"][i] - rc) / rc / rel_unit(rc, rf))
    m_ref = i_csr["mean_abs_div_final"]
    grant = st["n_fluid"] * 2.0 ** -53
    diff_d = abs(st["mean_abs_div_final"] - m_ref) / m_ref if m_ref != 0 else abs(st["mean_abs_div_final"])
    bar_d = FACTOR * (gap_d if gap_d > 0 else EPS) + grant
    print(f"clean edges {label}: istop {st['istop']} itn {st['itn']} (CPU {i_csr['itn'][:n]} / {i_free['itn'][:n]}, margin "
          f"{ITN_MARGIN}); "
          f"fields {diff_f:.3e} / unit {unit_f:.3e} = {diff_f / unit_f:.3f}; rnorm / unit max "
          f"{max(ratios_r, default=0.0):.3f}; mean|div| {diff_d:.3e} / bar {bar_d:.3e} = {diff_d / bar_d:.3f}")
    assert diff_f <= FACTOR * unit_f, label
    assert all(r <= FACTOR for r in ratios_r), (label, ratios_r)
    assert diff_d <= bar_d, label
    return diff_f / unit_f


def run(ctx, key, f, mask, sp=SP, **kw):
    orc = oracle(key, f, mask, sp, **kw)
    got, st = ctx.clean_divergence(*f, mask, *sp, **kw)
    compare(key, got, st, orc, mask)
    return got, st, orc


def check_stats(label, got, st, f_in, mask, sp, entries):
    """mean |div| and flux entries against numpy on the very fields they were measured on.
    ``entries``: [(name, reported value, (u, v, w) it was measured on)]."""
    dx, dy, dz = sp
    n = int(mask.sum())
    rows = mask.shape[0] * mask.shape[1]
    for name, val, f in entries:
        if name.startswith("flux"):
            mid = f[0][:, :, f[0].shape[2] // 2]
            want = cpu_ref.mid_plane_flux(f[0], dy, dz)
            bound = rows * 2.0 ** -53 * float(np.abs(mid).sum()) * abs(dy * dz)
            print(f"clean edges {label} {name}: |err| {abs(val - want):.3e} / bound {bound:.3e} = {abs(val - want) / bound:.3f}")
            assert abs(val - want) <= bound, (label, name)
        else:
            want = float(np.mean(np.abs(cpu_ref.consistent_divergence(*f, mask, dx, dy, dz)[mask])))
            bound = n * 2.0 ** -53
            err = abs(val - want) / want
            print(f"clean edges {label} {name}: rel err {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
            assert err <= bound, (label, name)


# ---- a. truncated LSQR ---------------------------------------------------------------------------
@pytest.mark.parametrize("damp", [1e-8, 0.0])
@pytest.mark.parametrize("iter_lim", [1, 2, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("shape", [(9, 11, 13), (9, 11, 14)], ids=["nx13_vec1", "nx14_vec2"])
def test_truncated_lsqr(ctx, shape, iter_lim, damp):
    """The only tight check of the t1, t2, rho, phibar recurrences; iter_lim around the polling
    batch of 8; damp = 0 takes PH_ALFA's undamped branch.  (9, 11, 13): odd nx, VEC = 1, 1287
    voxels = 2 blocks; (9, 11, 14): VEC = 2."""
    f, mask = make_fields(shape, 0), uniform_mask(shape, 0.8, 0)
    got, st, _ = run(ctx, f"trunc {shape} lim={iter_lim} damp={damp:g}", f, mask, iterations=1, iter_lim=iter_lim, damp=damp)
    assert st["istop"] == [7] and st["itn"] == [iter_lim] and st["n_outer"] == 1
    assert st["n_fluid"] == int(mask.sum())


# ---- b. iter_lim = 0 and iterations = 0 ----------------------------------------------------------
def test_iter_lim_zero_and_iterations_zero(ctx):
    shape = (9, 11, 13)
    f, mask = make_fields(shape, 1), uniform_mask(shape, 0.8, 1)
    got, st, orc = run(ctx, "iter_lim=0", f, mask, iterations=1, iter_lim=0)
    assert st["istop"] == [0] and st["itn"] == [0]
    # x = 0: the correction subtracts zeros on the fluid and zeroes the solid, as the oracle does
    for a, b, c in zip(got, orc[3][0], f):
        assert a.tobytes() == b.tobytes()
        assert a[mask].tobytes() == c[mask].tobytes() and (a[~mask] == 0).all()
    got, st, orc = run(ctx, "iterations=0", f, mask, iterations=0)
    assert st["n_outer"] == 0 and st["istop"] == [] and st["itn"] == []
    for a, c in zip(got, f):
        assert a.tobytes() == c.tobytes()  # copies: nothing is zeroed without a correction


# ---- c. zero right-hand side ---------------------------------------------------------------------
def test_zero_rhs_stops_at_once(ctx, capsys):
    shape = (7, 8, 10)
    mask = grains_mask(shape, 0)
    f = [np.zeros(shape) for _ in range(3)]
    got, st, orc = run(ctx, "zero rhs", f, mask, iterations=3)
    assert st["istop"] == [0] * 3 and st["itn"] == [0] * 3 and st["rnorm"] == [0.0] * 3
    assert st["mean_abs_div"] == [0.0] * 3 and st["mean_abs_div_final"] == 0.0
    assert st["flux_initial"] == 0.0 and st["flux_final"] == 0.0
    for a in got:
        assert a.tobytes() == np.zeros(shape).tobytes()
    needs_library()
    from ptv_interpolation_amd import physics

    out, lines = printed_by(capsys, lambda: physics.clean_divergence_projection(*f, mask, *SP, iterations=3))
    for a in out:
        assert a.tobytes() == np.zeros(shape).tobytes()
    info = orc[3][1]
    with np.errstate(invalid="ignore"):
        ratio = np.float64(info["mean_abs_div"][0]) / np.float64(info["mean_abs_div_final"])
    assert f"Total Reduction:      {ratio:.2f}x" == "Total Reduction:      nanx"  # 0/0 in numpy floats
    assert f"Total Reduction:      {ratio:.2f}x" in lines
    assert "Initial Mean Abs Div: 0.000000e+00" in lines and "Final Mean Abs Div:   0.000000e+00" in lines
    assert sum(line.startswith("--- Iteration ") for line in lines) == 3


# ---- d. A = 0 with b != 0, extents of 1 ----------------------------------------------------------
def test_isolated_voxels_a_zero_b_nonzero(ctx):
    """Only [1,1,1] and [1,1,3] are fluid: every row of A is zero, b is not.  alfa = 0, so
    alfa * beta == 0 stops with istop 0, x = 0, rnorm = ||b||."""
    shape = (3, 3, 5)
    mask = np.zeros(shape, bool)
    mask[1, 1, 1] = mask[1, 1, 3] = True
    f = make_fields(shape, 2)
    got, st, orc = run(ctx, "A=0 b!=0", f, mask, iterations=2)
    assert st["istop"] == [0, 0] and st["itn"] == [0, 0] and st["n_fluid"] == 2
    assert orc[3][1]["r2norm"][0] > 0 and st["rnorm"] == orc[3][1]["r2norm"]  # ||b|| of two terms: exact
    for a, c in zip(got, f):
        assert a[mask].tobytes() == c[mask].tobytes() and (a[~mask] == 0).all()


def test_single_voxel(ctx):
    f = [np.full((1, 1, 1), x) for x in (0.5, -1.25, 2.0)]
    mask = np.ones((1, 1, 1), bool)
    got, st, _ = run(ctx, "1x1x1", f, mask, iterations=2)
    assert st["istop"] == [0, 0] and st["itn"] == [0, 0] and st["n_fluid"] == 1
    for a, c in zip(got, f):
        assert a.tobytes() == c.tobytes()


@pytest.mark.parametrize("shape,seed", [((1, 1, 300), 0), ((1, 40, 1), 0), ((40, 1, 2), 0)],
                         ids=["1x1x300", "1x40x1", "40x1x2"])
def test_extent_one_axes_full_solve(ctx, shape, seed):
    """Lines and a two-voxel-wide sheet: two axes contribute no stencil term; p = 0.8 cuts the
    line into several disconnected fluid runs (and isolated voxels).  Full iter_lim."""
    f, mask = make_fields(shape, seed), uniform_mask(shape, 0.8, seed)
    run(ctx, f"extent-1 {shape}", f, mask, iterations=2)


def test_two_disconnected_regions(ctx):
    """A solid wall splits the fluid into two regions (A has a two-dimensional null space)."""
    shape = (6, 7, 9)
    f = make_fields(shape, 3)
    mask = np.ones(shape, bool)
    mask[:, :, 4] = False
    run(ctx, "two regions", f, mask, iterations=2)


# ---- e. every stop reason ------------------------------------------------------------------------
def test_istop_3_condition_limit(ctx):
    """dz = 1e-3 makes cond(A) pass conlim = 1e8: acond = anorm * sqrt(ddnorm) decides."""
    shape = (6, 7, 8)
    f, mask = make_fields(shape, 3), uniform_mask(shape, 0.85, 3)
    _, st, orc = run(ctx, "istop 3", f, mask, sp=(1.0, 1.0, 1e-3), iterations=1)
    assert st["istop"] == [3] and orc[3][1]["acond"][0] >= 1e8


@pytest.mark.parametrize("damp,want", [(0.0, 4), (1e-8, 5)], ids=["istop4", "istop5"])
def test_istop_4_and_5_machine_precision(ctx, damp, want):
    """atol = btol = 0 leaves only the machine-precision stops: 1 + t1 <= 1 (xnorm, anorm) without
    damping, 1 + test2 <= 1 (arnorm, anorm, rnorm) with it."""
    shape = (4, 5, 6)
    f, mask = make_fields(shape, 0), uniform_mask(shape, 0.85, 0)
    _, st, _ = run(ctx, f"istop {want}", f, mask, iterations=1, atol=0.0, btol=0.0, damp=damp)
    assert st["istop"] == [want]


# ---- f. NaN --------------------------------------------------------------------------------------
def test_nan_in_a_fluid_voxel_stops_the_loop(ctx, capsys):
    """b is all NaN: beta is not > 0 (S_SKIPV), no test fires, the solve runs to iter_lim with a
    NaN phi; its correction is not applied and the outer loop ends."""
    shape = (4, 5, 6)
    mask = np.ones(shape, bool)
    f = make_fields(shape, 4)
    f[0][2, 2, 3] = np.nan
    orc = oracle("nan fluid", f, mask, iterations=3)
    assert orc[2] and orc[3][1]["nan_stop"] and orc[4][1]["nan_stop"]
    got, st = ctx.clean_divergence(*f, mask, *SP, iterations=3)
    assert st["nan_stop"] and st["n_outer"] == 1 and st["istop"] == [7] and st["itn"] == [3000]
    assert st["istop"] == orc[3][1]["istop"] and st["itn"] == orc[3][1]["itn"]
    for a, b, c in zip(got, orc[3][0], f):
        assert a.tobytes() == c.tobytes() == b.tobytes()  # the inputs, NaN included
    needs_library()
    from ptv_interpolation_amd import physics

    out, lines = printed_by(capsys, lambda: physics.clean_divergence_projection(*f, mask, *SP, iterations=3))
    assert "  Warning: Solve failed. Stopping iterations." in lines
    assert sum(line.startswith("--- Iteration ") for line in lines) == 1
    for a, c in zip(out, f):
        assert a.tobytes() == c.tobytes()


@pytest.mark.parametrize("where", ["interior", "last_x"])
def test_nan_in_a_solid_voxel_follows_the_oracle(ctx, where):
    """interior: the face average with the fluid voxel above is NaN, so the divergence and the
    solve are; last_x: a solid voxel at x = nx - 1 feeds only its own (excluded) divergence, the
    cleaning runs and the correction writes 0 over the NaN."""
    shape = (4, 5, 6)
    mask = np.ones(shape, bool)
    pos = (2, 2, 3) if where == "interior" else (2, 2, 5)
    mask[pos] = False
    f = make_fields(shape, 5)
    f[0][pos] = np.nan
    orc = oracle(f"nan solid {where}", f, mask, iterations=2)
    assert orc[2] and orc[3][1]["nan_stop"] == orc[4][1]["nan_stop"] == (where == "interior")
    got, st = ctx.clean_divergence(*f, mask, *SP, iterations=2)
    if where == "interior":
        assert st["nan_stop"] and st["n_outer"] == 1 and st["istop"] == orc[3][1]["istop"] == [7]
        assert st["itn"] == orc[3][1]["itn"]
        for a, b in zip(got, orc[3][0]):
            assert a.tobytes() == b.tobytes()
    else:
        compare(f"nan solid {where}", got, st, orc, mask)
        assert not np.isnan(np.stack(got)).any()


# ---- g. more than 256 first-stage partials -------------------------------------------------------
@pytest.mark.parametrize("shape", [(66, 64, 63), (65, 90, 90)], ids=["vec1_260_blocks", "vec2_258_blocks"])
def test_more_than_256_partials(ctx, shape):
    """The second stride step of k_scalar's sum over the partials (k += kFinalThreads), for the
    solver's norms and for the three rows of the divergence statistics."""
    f, mask = make_fields(shape, 6), uniform_mask(shape, 0.9, 6)
    got, st, _ = run(ctx, f"partials {shape}", f, mask, iterations=1, iter_lim=9)
    assert st["istop"] == [7] and st["itn"] == [9]
    check_stats(f"partials {shape}", got, st, f, mask, SP,
                [("mean_abs_div[0]", st["mean_abs_div"][0], f), ("flux_initial", st["flux_initial"], f),
                 ("mean_abs_div_final", st["mean_abs_div_final"], got), ("flux_final", st["flux_final"], got)])


def test_reported_numbers_every_entry(ctx):
    """Every mean_abs_div entry and both fluxes against numpy on the fields they were measured
    on: entry i of a 3-iteration call is the final mean |div| of an i-iteration call on the same
    input (two calls give identical bits, tests/test_gpu_clean.py), whose output fields are known."""
    shape = (9, 11, 13)
    f, mask = make_fields(shape, 7), grains_mask(shape, 7)
    got3, st3, _ = run(ctx, "stats its=3", f, mask, iterations=3, iter_lim=17)
    entries = [("mean_abs_div[0]", st3["mean_abs_div"][0], f), ("flux_initial", st3["flux_initial"], f),
               ("mean_abs_div_final", st3["mean_abs_div_final"], got3), ("flux_final", st3["flux_final"], got3)]
    for i in (1, 2):
        got_i, st_i = ctx.clean_divergence(*f, mask, *SP, iterations=i, iter_lim=17)
        assert st_i["mean_abs_div_final"] == st3["mean_abs_div"][i]
        assert st_i["rnorm"] == st3["rnorm"][:i] and st_i["mean_abs_div"] == st3["mean_abs_div"][:i]
        entries.append((f"mean_abs_div[{i}]", st3["mean_abs_div"][i], got_i))
    check_stats("stats its=3", got3, st3, f, mask, SP, entries)


# ---- h. more outer iterations than the stats hold ------------------------------------------------
def test_eighteen_outer_iterations(ctx, capsys):
    shape = (5, 6, 7)
    f, mask = make_fields(shape, 8), uniform_mask(shape, 0.85, 8)
    got, st, orc = run(ctx, "iterations=18", f, mask, iterations=18, iter_lim=8)
    info, info2 = orc[3][1], orc[4][1]
    assert st["n_outer"] == 18 and info["n_outer"] == 18
    for key in ("istop", "itn", "rnorm", "mean_abs_div"):
        assert len(st[key]) == MAX_OUTER, key
    assert st["istop"] == info["istop"][:MAX_OUTER] and st["itn"] == info["itn"][:MAX_OUTER] == [8] * MAX_OUTER
    grant = st["n_fluid"] * 2.0 ** -53
    worst = 0.0
    for i in range(MAX_OUTER):  # entry 15 is solve 16's, not solve 18's
        a, b = info["mean_abs_div"][i], info2["mean_abs_div"][i]
        bar = FACTOR * rel_unit(a, b) + grant
        err = abs(st["mean_abs_div"][i] - a) / a
        worst = max(worst, err / bar)
        assert err <= bar, (i, st["mean_abs_div"][i], a)
    print(f"clean edges iterations=18: mean_abs_div[0..15] max err / bar = {worst:.3f}")
    assert abs(info["mean_abs_div"][15] - info["mean_abs_div"][17]) / info["mean_abs_div"][15] > 100 * (
        FACTOR * rel_unit(info["mean_abs_div"][15], info2["mean_abs_div"][15]) + grant), "entries 15 and 17 must differ"
    needs_library()
    from ptv_interpolation_amd import physics

    out, lines = printed_by(capsys, lambda: physics.clean_divergence_projection(*f, mask, *SP, iterations=18))
    assert [line for line in lines if line.startswith("--- Iteration ")] == [f"--- Iteration {i + 1}/18 ---" for i in range(18)]
    assert sum(line.startswith("  Solving Poisson") for line in lines) == 18
    full, st_full = ctx.clean_divergence(*f, mask, *SP, iterations=18)  # the entry point's lsqr defaults
    assert st_full["n_outer"] == 18 and len(st_full["mean_abs_div"]) == MAX_OUTER
    for a, b in zip(out, full):
        assert a.tobytes() == b.tobytes()
    want = [f"  Current Mean Abs Div: {m:.6e}" for m in st_full["mean_abs_div"]]
    assert [line for line in lines if line.startswith("  Current Mean Abs Div: ")] == want


# ---- i. alignment fallback, in place, mask bytes (device pointers) -------------------------------
def _dev_call(ctx, f, mask_u8, offset_fields=0, offset_mask=0, in_place=False, **kw):
    """clean_divergence_dev on torch tensors; the fields start ``offset_fields`` float64 into their
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
    outs = held if in_place else [put(np.zeros(n), offset_fields, torch.float64) for _ in f]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for _, t in held]
    assert all(p % 16 == 8 * (offset_fields % 2) for p in ptrs) and m.data_ptr() % 2 == offset_mask % 2
    st = ctx.clean_divergence_dev(nx, ny, nz, ptrs, m.data_ptr(), [t.data_ptr() for _, t in outs], *SP, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy().reshape(nz, ny, nx) for _, t in outs], st


def test_alignment_fallback_in_place_and_mask_bytes(ctx):
    """Even nx takes the VEC = 2 kernels only when every field is 16-byte and the mask 2-byte
    aligned; fields one float64 in, or the mask one byte in, fall back to VEC = 1 and must meet
    the same oracle.  In place equals out of place; any nonzero mask byte means fluid, in
    ptv_div.hip and ptv_clean.hip alike."""
    needs_library()
    shape = (9, 11, 14)
    f, mask = make_fields(shape, 0), uniform_mask(shape, 0.8, 0)
    kw = dict(iterations=1, iter_lim=9)
    orc = oracle(f"trunc {shape} lim=9 damp=1e-08", f, mask, damp=1e-8, **kw)
    m8 = mask.view(np.uint8)
    base, st = _dev_call(ctx, f, m8, **kw)
    compare("dev aligned", base, st, orc, mask)
    for label, of, om in (("fields +8 bytes", 1, 0), ("mask +1 byte", 0, 1), ("both", 1, 1)):
        got, st_o = _dev_call(ctx, f, m8, offset_fields=of, offset_mask=om, **kw)
        compare(f"dev misaligned: {label}", got, st_o, orc, mask)
    inpl, st_i = _dev_call(ctx, f, m8, in_place=True, **kw)
    for a, b in zip(base, inpl):
        assert a.tobytes() == b.tobytes()
    assert st_i["rnorm"] == st["rnorm"] and st_i["mean_abs_div_final"] == st["mean_abs_div_final"]
    odd = m8.copy()
    fl = np.flatnonzero(odd.reshape(-1))
    odd.reshape(-1)[fl[1::3]] = 2
    odd.reshape(-1)[fl[2::3]] = 255
    other, st_m = _dev_call(ctx, f, odd, **kw)
    for a, b in zip(base, other):
        assert a.tobytes() == b.tobytes()
    for key in ("n_fluid", "rnorm", "mean_abs_div", "mean_abs_div_final", "flux_final"):
        assert st_m[key] == st[key], key


# ---- j. C-level argument checks ------------------------------------------------------------------
def test_argument_checks_leave_the_result_alone(ctx):
    needs_library()
    import torch

    shape = (3, 4, 6)
    nz, ny, nx = shape
    f, mask = make_fields(shape, 9), uniform_mask(shape, 0.8, 9)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in f]
    outs = [torch.full((f[0].size,), -7.0, dtype=torch.float64, device=dev) for _ in f]
    m = torch.from_numpy(mask.view(np.uint8).copy()).to(dev)
    solid = torch.zeros(mask.size, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def call(mk=m, sp=SP, **kw):
        return ctx.clean_divergence_dev(nx, ny, nz, [a.data_ptr() for a in t], mk.data_ptr(),
                                        [a.data_ptr() for a in outs], *sp, **kw)

    bad = [dict(sp=(0.0, 1.25, 0.8)), dict(sp=(1.0, 0.0, 0.8)), dict(sp=(1.0, 1.25, 0.0)),
           dict(sp=(float("nan"), 1.25, 0.8)), dict(sp=(1.0, float("nan"), 0.8)), dict(sp=(1.0, 1.25, float("nan"))),
           dict(damp=-1e-8), dict(atol=-1e-10), dict(btol=-1e-10), dict(iter_lim=-1), dict(iterations=-1),
           dict(damp=float("nan")), dict(mk=solid)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == -7.0).all()), kw
    with pytest.raises(ValueError):  # the host entry point reports the same errors
        ctx.clean_divergence(*f, np.zeros_like(mask), *SP)
    with pytest.raises(ValueError):
        ctx.clean_divergence(*f, mask, 1.0, float("nan"), 0.8)
    st = call(iterations=1, iter_lim=2)  # and the same buffers work once the arguments are right
    assert st["istop"] == [7] and not bool((outs[0] == -7.0).any())
