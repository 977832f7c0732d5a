"""CPU preconditions of tests/test_gpu_geometry.py: the properties of the case table
(tests/_geometry.py) that the GPU comparisons rely on, so that no GPU test can pass by exclusion.

* every (case, k) the GPU tests run has no value-heterogeneous distance tie (near_planar: at most
  1 % of the voxels), and the oracle's output is finite (all NaN only where that is the case's point);
* the oracle is invariant under the power-of-two scalings (same neighbour indices);
* the outlier-filter cases have no tie-order dependent particle;
* the oracle raises ValueError for NaN coordinates, which the GPU path mirrors.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _geometry as G
from tests._util import filter_ties


@pytest.mark.parametrize("name,k", G.runs())
def test_tie_cap_and_finite_oracle(name, k):
    het = G.hetero(name, k)
    cap = G.TIE_CAP.get(name.split("@")[0], 0.0)
    print(f"{name} k={k}: value-heterogeneous tie share {het.mean():.4%} (cap {cap:.0%})")
    assert het.mean() <= cap
    for a in G.oracle_knn(name, k):
        assert np.isfinite(a).all()


def test_case_shapes():
    """The shapes the cases are meant to have: a padded x tile, n = k, one particle, every voxel of
    grid_far outside the particle box, grid_inside_gap's grid between its two slabs of particles."""
    P, Q, ax, ay, az = G.case("base")
    assert (len(ax), len(ay), len(az)) == (13, 10, 9) and len(P) == G.N
    for k in G.K_ALL:
        assert len(G.case("n_eq_k", k)[0]) == k
    assert len(G.case("n_1")[0]) == 1
    P, _, ax, ay, az = G.case("grid_far")
    assert ax.min() > P[:, 0].max() and ay.max() < P[:, 1].min() and az.min() > P[:, 2].max()
    P, _, ax, _, _ = G.case("grid_inside_gap")
    assert len(P) >= 50 and not ((P[:, 0] >= 2.0) & (P[:, 0] <= 10.0)).any() and ax.min() == 3.0 and ax.max() == 9.0
    P = G.case("near_planar")[0]
    ext = np.ptp(P, axis=0)
    assert 0.0 < ext[2] < 1e-9 * ext.max()  # below the library's dimension-count threshold
    ax = G.case("axes_irregular")[2]
    assert (np.diff(ax) < 0).all() and np.ptp(np.diff(ax)) > 0.1


def test_dense_grid_builds_the_lattice():
    """The lattice-sized grid and its slab are above the library's 50 000-voxel lattice threshold
    (ptv_search.cpp kLatticeStopPoints) with every extent >= 9; the small grid is not."""
    nx, ny, nz = G.DENSE
    z0, z1 = G.DENSE_SLAB
    assert nx * ny * (z1 - z0) > 50000 and min(nx, ny, z1 - z0) >= 9 and 0 < z0 < z1 < nz
    _, _, ax, ay, az = G.case("planar@dense")
    assert (len(ax), len(ay), len(az)) == G.DENSE
    assert 13 * 10 * 9 <= 50000


@pytest.mark.parametrize("e", G.SCALE_EXPONENTS)
def test_oracle_scale_invariance(e):
    """Scaling by 2^e is exact, so every comparison the tree makes is preserved: the neighbour
    indices equal the base case's, the distances are the base case's times 2^e."""
    Pb = G.case("base")[0]
    Ps = G.case(f"scale_2^{e}")[0]
    for k in (1, 8, 20, 130):
        db, ib = cpu_ref.knn_kdtree(Pb, G.queries("base"), k)
        ds, is_ = cpu_ref.knn_kdtree(Ps, G.queries(f"scale_2^{e}"), k)
        assert np.array_equal(ib, is_)
        assert np.array_equal(db * 2.0 ** e, ds)


@pytest.mark.parametrize("name", G.FILTER_CASES)
@pytest.mark.parametrize("k", G.FILTER_K)
def test_filter_cases_have_no_ties(name, k):
    assert filter_ties(G.case(name)[0], k).mean() == 0.0


@pytest.mark.parametrize("name", G.RADIUS_CASES)
def test_radius_cases(name):
    """grid_far's balls are all empty (the NaN pattern is the whole grid), the others' are not."""
    P, Q, *_ = G.case(name)
    ref = cpu_ref.idw_radius_points(P, Q, G.queries(name), G.RADIUS * G.scale_of(name))
    assert np.isnan(ref).all() if name == "grid_far" else np.isfinite(ref).any()


def test_oracle_rejects_nan_coordinates():
    """cKDTree refuses a NaN in the particles and in the queries: the behaviour the GPU path has to
    mirror (ValueError, not a number)."""
    P, Q, *_ = G.case("base")
    q = G.queries("base")
    bad = P.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError):
        cpu_ref.interp_points(bad, Q, q)
    badq = q.copy()
    badq[5, 2] = np.nan
    with pytest.raises(ValueError):
        cpu_ref.interp_points(P, Q, badq)
