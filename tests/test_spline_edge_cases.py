"""The long-double spline chain (tests/_mesh_ref.py) against scipy on the seeded cases of
tests/_spline_edges.py, before the GPU tests lean on it as "exact": no device needed.

The bars are those of test_mesh_ref.test_spline_fixtures: the coefficients and the order-3 samples
within 64 eps max|coefficient|, the order-1 samples within 16 eps max|field|, order 0 equal.
Measured with scipy 1.15.3 over all cases: coefficients <= 9.5 eps max|coefficient|, order 1 <= 2.1
eps max|field|, order 3 <= 8 eps max|coefficient| on the short axes and 14.5, 16.4 and 42.7 on the
axes of 105, 70 and 200 samples.  That growth is scipy's own: it forms the fraction from the float64
sum coordinate + 12, whose rounding grows with the coordinate; sampling scipy's own coefficients
with the chain's weights shows the same distance.  The printed figures separate the coordinates
within the padded extent from those past it.

scipy's rule past the pad, as probed below.  For order 3 and mode='nearest' scipy samples the
coefficients of the field padded by 12 samples, N = n + 24 per axis, at the padded coordinate
p = c + 12 clamped to [-1, N] -- one sample past either end, not [0, N - 1] -- and edge-extends only
the four indices floor(p) - 1 .. floor(p) + 2 to [0, N - 1].  Between -1 and 0 and between N - 1 and N
the fraction still moves the weights, so the sample keeps changing (by 1e-8 of the field on a normal
field); at -1 and at N it saturates, and stays there out to 1e18.  A clamp of p to [0, N - 1] stands
1e-8 off from c = -12.25 outward, some 1e7 times the bar.
"""
import numpy as np
import pytest
from scipy import ndimage

import _mesh_ref as mref
import _spline_edges as se


@pytest.mark.parametrize("case", se.CASES, ids=se.case_id)
def test_long_double_chain_stands_on_scipy(case):
    r = se.reference(*case)
    assert r.coef.shape == tuple(n + 24 for n in r.shape) == r.coef_scipy.shape
    q = r.coef_gap().max() / (mref.EPS * r.cmax)
    print(f"{se.case_id(case)} coefficients: max |scipy - chain| = {q:.2f} eps max|coef|")
    assert q <= 64
    for order, bar in ((3, 64), (1, 16)):
        g = r.gap(order) / (mref.EPS * r.scale[order])
        for name, sel in (("within the pad", ~r.far), ("past the pad", r.far)):
            print(f"{se.case_id(case)} order {order} {name}: max |scipy - chain| = {g[sel].max():.2f} eps scale")
        assert np.all(g <= bar), (order, r.points[:, g > bar][:, :5])
    assert np.array_equal(r.exact[0], r.scipy[0])


def _along(field, axis, values, at):
    co = np.repeat(np.asarray(at, dtype=np.float64).reshape(3, 1), len(values), axis=1)
    co[axis] = values
    return co


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_scipys_rule_past_the_pad(axis):
    """One axis leaves the padded extent, the other two stay inside the field."""
    r = se.reference("normal", (5, 6, 7))
    field, n, N = r.field, r.shape[axis], r.shape[axis] + 24
    at = [1.3, 2.6, 3.1]
    tol = 64 * mref.EPS * r.cmax

    def both(raw):
        co = _along(field, axis, raw, at)
        return ndimage.map_coordinates(field, co, order=3, mode="nearest"), co

    def clamped(co, lo, hi):  # the chain's arithmetic with the padded coordinate clamped to [lo, hi]
        c = co.astype(mref.LD)
        c[axis] = np.clip(c[axis] + mref.PAD, lo, hi) - mref.PAD
        return mref.sample3(r.coef, c)

    for side, edge, sat, sign in (("low", -12.0, -13.0, -1.0), ("high", n + 11.0, n + 12.0, 1.0)):
        # between the last padded sample and one past it the value still moves ...
        between = edge + sign * np.array([0.0, 0.125, 0.25, 0.5, 0.75, 0.875, 1.0])
        s, co = both(between)
        assert np.all(np.abs(np.diff(s)) > tol) and abs(s[-1] - s[0]) > 1e3 * tol, (side, s)
        # ... as the spline over the edge-extended indices does: a clamp to [-1, N], not to [0, N - 1]
        assert np.all(np.abs(s - clamped(co, -1, N)) <= tol), side
        assert np.all(np.abs(s[1:] - clamped(co, 0, N - 1)[1:]) > 1e3 * tol), side
        # saturation one sample past the padded extent: nothing changes from there to 1e18
        beyond = sat + sign * np.array([0.0, 2.0 ** -40, 0.25, 0.5, 1.0, 17.0, 1e6, 1e18])
        s2, co2 = both(beyond)
        assert np.all(np.abs(s2 - s[-1]) <= tol), (side, s2 - s[-1])
        assert np.all(np.abs(s2 - clamped(co2, -1, N)) <= tol), side
        # and right before it the value is not yet there
        s3, _ = both(np.array([sat - sign * 0.25]))
        assert abs(s3[0] - s[-1]) > 10 * tol, side


def test_orders_0_and_1_have_no_pad():
    """Orders 0 and 1 read the raw field at the coordinate clamped to [0, n - 1]: constant outside."""
    r = se.reference("normal", (5, 6, 7))
    at, tol = [1.3, 2.6, 3.1], 16 * mref.EPS * r.fmax
    for axis in range(3):
        n = r.shape[axis]
        for order in (0, 1):
            for values in ([0.0, -0.25, -12.5, -13.0, -1e18], [n - 1.0, n - 0.75, n + 11.5, n + 12.0, 1e18]):
                s = ndimage.map_coordinates(r.field, _along(r.field, axis, values, at), order=order, mode="nearest")
                assert np.all(np.abs(s - s[0]) <= tol), (axis, order, s)


def test_the_cases_reach_their_paths():
    px = sorted({s[2] + 24 for s in se.SHAPES})
    chunks = {n: (-(-n // 64), n % 64) for n in px}
    assert chunks[64] == (1, 0) and chunks[65] == (2, 1) and chunks[128] == (2, 0) and chunks[129] == (3, 1)
    assert chunks[224] == (4, 32)
    assert (8 + 24) * (2 + 24) % 64 == 0 and (2, 8, 3) in se.SHAPES  # a last block of exactly 64 rows
    assert (5 + 24) * (6 + 24) % 64  # and the plain case has a partial one
    for axis in range(3):  # both sides of the start sum's switch (whole line up to 41 padded samples), per pass
        assert {17, 18} <= {s[axis] for s in se.SHAPES if sorted(s)[:2] == [2, 2]}
    assert (70, 2, 2) in se.SHAPES and (2, 70, 2) in se.SHAPES and (1, 1, 1) in se.SHAPES
    for shape in se.SHAPES:
        co = se.coordinates(shape)
        n = np.array(shape, dtype=np.float64).reshape(3, 1)
        assert co["inside"].min() >= -0.25 and np.all(co["inside"] <= n - 0.75)
        assert co["wide"].min() >= -14 and np.all(co["wide"] <= n + 13)
        for kind in ("inside", "wide"):
            assert 200 <= co[kind].shape[1] <= 400
        assert co["excursion"].shape[1] >= 200
        assert not se.past_the_pad(shape, co["inside"]).any()
        for kind in ("wide", "lattice", "lattice_half"):
            far = se.past_the_pad(shape, co[kind])
            assert far.any() and not far.all(), kind
        assert se.past_the_pad(shape, co["excursion"]).all()
        lat = {tuple(c) for c in co["lattice"].T}
        assert (-13.0, -12.0, shape[2] + 12.0) in lat and (shape[0] - 1.0, float(shape[1]), -1.0) in lat
        assert len(lat) == np.prod([len({-13, -12, -1, 0, m - 1, m, m + 11, m + 12}) for m in shape])
        for v in se.LOW:
            for axis in range(3):
                assert np.any(co["excursion"][axis] == v)
        assert np.any(co["excursion"] == 1e18) and np.any(co["excursion"] == 1e6)
        assert all(np.abs(c).max() <= 1e18 and np.isfinite(c).all() for c in co.values())
    assert {k for k, _ in se.CASES} == set(se.KINDS + se.TYPED)
    assert [se.field(k, (5, 6, 7)).dtype for k in se.TYPED] == [np.float32, np.int16, np.bool_]
    huge = se.field("huge", (5, 6, 7))
    assert np.abs(huge).max() > 1e153 and np.isfinite(huge).all()
