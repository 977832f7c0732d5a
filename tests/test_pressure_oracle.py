"""CPU checks of the pressure recovery's oracle: tests/_pressure_ref.py against the reference's own
results in tests/golden/pressure_*.npz (written by tests/golden/make_pressure_golden.py)."""
import glob
import os

import numpy as np
import pytest

import _pressure_ref as pref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("pressure_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "pressure_*.npz")))


def load(name):
    g = np.load(os.path.join(GOLDEN, f"pressure_{name}.npz"), allow_pickle=False)
    d = {k: g[k] for k in g.files}
    for k in ("wall_bc", "anchor", "flow_direction"):
        d[k] = str(d[k])
    for k in ("mu", "rho", "dx", "dy", "dz", "order_gap"):
        d[k] = float(d[k])
    return d


def test_every_case_is_there():
    assert CASES == sorted(["g12", "g20", "inhom", "rho", "neg", "autoneg", "odd", "none", "wrap"])


@pytest.mark.parametrize("name", CASES)
def test_force_field_and_rhs_bits(name):
    g = load(name)
    f = pref.force_field(g["u"], g["v"], g["w"], g["dx"], g["dy"], g["dz"], g["mu"], g["rho"], g["mask"])
    for a, key in zip(f, ("fx", "fy", "fz")):
        assert np.array_equal(a, g[key]), key
    rhs = pref.force_divergence(*f, g["mask"], g["dx"], g["dy"], g["dz"], g["wall_bc"])
    assert np.array_equal(rhs, g["rhs"])
    means = [np.mean(np.abs(a[g["mask"]])) for a in f]
    assert np.array_equal(means, g["means"])


@pytest.mark.parametrize("name", CASES)
def test_dirichlet_set(name):
    g = load(name)
    plane = pref.anchor_plane(g["mask"].shape, g["anchor"], g["flow_direction"], g["w"], g["mask"])
    assert np.array_equal(pref.dirichlet_grid(g["mask"], plane), g["dirichlet"])
    assert (g["p"][~g["mask"]] == 0).all() and (g["p"][g["dirichlet"]] == 0).all()


@pytest.mark.parametrize("name", [c for c in CASES if c != "none"])
def test_pressure_within_the_bar(name):
    g = load(name)
    p, itn, info = pref.cg_solve(g["rhs"], g["mask"], g["dirichlet"], g["dx"], g["dy"], g["dz"])
    assert info == int(g["info"]) and itn == int(g["itn_free"])
    assert pref.normwise(p, g["p"]) <= g["order_gap"]


def test_wrap_fixture_exercises_the_wrap():
    g = load("wrap")
    args = (g["u"], g["v"], g["w"], g["dx"], g["dy"], g["dz"], g["mu"], g["rho"], g["mask"])
    off = pref.force_field(*args, wrap=False)
    assert not np.array_equal(off[0], g["fx"])
    last = g["mask"].shape[0] - 1  # the difference sits on the plane round 2 fills across the z wrap
    assert not np.array_equal(off[0][last], g["fx"][last])


def test_symmetric_elimination_gives_the_reference_bits():
    """CG from x0 = 0 with b = 0 on the Dirichlet rows never multiplies a leftover column by anything
    but 0: the reference's matrix and the symmetric one give identical bits."""
    from scipy.sparse.linalg import cg

    from _variational_ref import single_threaded_blas

    g = load("g12")
    m, d = g["mask"], g["dirichlet"]
    b = g["rhs"][m].copy()
    b[d[m]] = 0.0
    A = pref.laplacian_matrix(m, g["dx"], g["dy"], g["dz"], d, symmetric=False)
    S = pref.laplacian_matrix(m, g["dx"], g["dy"], g["dz"], d, symmetric=True)
    assert (A != A.T).nnz > 0 and (S != S.T).nnz == 0
    with single_threaded_blas():
        xa, ia = cg(A, b, rtol=1e-10, atol=0.0, maxiter=3000)
        xs, i_s = cg(S, b, rtol=1e-10, atol=0.0, maxiter=3000)
    assert ia == i_s == 0
    assert np.array_equal(xa, xs)
    assert (xa[d[m]] == 0).all()
