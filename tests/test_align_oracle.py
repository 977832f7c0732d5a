"""The numpy restatement of the mask alignment (tests/_align_ref.py) held to scipy and to the
reference's own fixtures (tests/golden/align_*.npz, recorded by make_align_golden.py from
auto_align.find_best_offset).  No device needed."""
import os

import numpy as np
import pytest
from scipy.optimize import minimize

import _align_ref as aref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("shape, fill", [((9, 10, 11), 0.5), ((3, 4, 5), 0.9), ((1, 1, 7), 0.6), ((2, 2, 2), 0.5)])
def test_brute_force_equals_scipy(shape, fill):
    rng = np.random.default_rng(5)
    mask = rng.random(shape) < fill
    mask.flat[rng.integers(mask.size)] = False
    d2 = aref.edt2_brute(mask)
    assert np.array_equal(d2, aref.edt2(mask))
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), aref.edt(mask))


def test_scipy_is_the_square_root_of_an_integer():
    rng = np.random.default_rng(6)
    mask = rng.random((33, 40, 47)) < 0.995
    d = aref.edt(mask)
    assert np.array_equal(np.sqrt(np.rint(d * d)), d)


@pytest.mark.parametrize("name", sorted(aref.CASES))
def test_seeded_cases_are_the_fixtures(name):
    g = np.load(os.path.join(GOLDEN, f"align_{name}.npz"), allow_pickle=False)
    mask, pts, initial = aref.CASES[name]()
    assert np.array_equal(mask, g["mask"]) and np.array_equal(pts, g["points"])
    assert np.array_equal(np.asarray(initial, dtype=np.float64), g["initial"])
    assert np.array_equal(aref.PROBE_OFFSETS, g["probe_offsets"])


@pytest.mark.parametrize("name", sorted(aref.CASES))
def test_objective_equals_the_references(name):
    g = np.load(os.path.join(GOLDEN, f"align_{name}.npz"), allow_pickle=False)
    dt = aref.edt(~g["mask"])
    got = np.array([aref.objective(g["points"], dt, o) for o in g["probe_offsets"]], dtype=np.float64)
    assert np.array_equal(got, g["probe_values"]), (got, g["probe_values"])
    assert got[4] == aref.OUTSIDE_SCORE  # the probe that moves every point out


@pytest.mark.parametrize("name", sorted(aref.CASES))
def test_powell_over_the_restatement_ends_where_the_reference_did(name):
    g = np.load(os.path.join(GOLDEN, f"align_{name}.npz"), allow_pickle=False)
    dt = aref.edt(~g["mask"])
    calls = []

    def f(o):
        calls.append(1)
        return aref.objective(g["points"], dt, o)

    res = minimize(f, tuple(g["initial"]), method="Powell", tol=1e-1)
    assert np.array_equal(res.x, g["res_x"]) and res.fun == g["res_fun"]
    assert len(calls) == int(g["nfev"])


def test_layered_distances_are_integers():
    mask, _, _ = aref.layered_case()
    d = aref.edt(~mask)
    assert np.array_equal(d, np.rint(d)) and d.max() == 3.0


def test_record_and_bound():
    mask, pts, _ = aref.blob_case()
    dt = aref.edt(~mask)
    n_in, n_out, s, e = aref.record(pts, dt, (0.5, -0.5, 1.5))
    assert n_in + n_out == len(pts) and n_in > 0 and n_out > 0
    assert abs(s - e) <= aref.sum_bound(n_in, e)
    assert aref.objective(pts, dt, (0.5, -0.5, 1.5)) == s + n_out * dt.max()
    assert aref.record(pts[:0], dt, (0, 0, 0)) == (0, 0, 0.0, 0.0)
    assert aref.objective(pts[:0], dt, (0, 0, 0)) == aref.OUTSIDE_SCORE
