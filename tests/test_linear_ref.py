"""The oracle of tests/test_gpu_linear_location.py (tests/_linear_ref.py) is right and has teeth.  CPU only.

* The restated brute-force scan equals ``Delaunay.find_simplex(bruteforce=True)`` query by query
  (with find_simplex's ``eps_broad = sqrt(100 DBL_EPSILON)``).
* ``LinearNDInterpolator`` itself (what ``griddata(method='linear')`` calls) leaves no voxel
  unexplained, on any case, with the interpolator's ``eps_broad = sqrt(DBL_EPSILON)``.
* Which of the two constants the interpolator uses is settled by probes across faces shared with
  flat simplices (test_eps_broad_of_the_interpolator).
* Every mutation of the location rule or of the arithmetic is rejected.
"""
import numpy as np
import pytest

from tests import _linear_ref as R

CASES = list(R.CASES)
DELTAS = (5e-9, 3e-8, 5e-8, 1e-7, 5e-7)  # below both constants, three in the band, above both


def _reference(name):
    from scipy.interpolate import LinearNDInterpolator

    P, Q, axes, d = R.case(name)
    return LinearNDInterpolator(d, Q, fill_value=R.FILL)(R.grid_queries(*axes))


@pytest.fixture(scope="module")
def probes():
    """(Delaunay, values, queries, delta per query, one-query-per-call reference output)."""
    from scipy.interpolate import LinearNDInterpolator

    P, Q, _, d = R.case("lattice_on")
    q, dl = R.flat_face_probes(d, P, DELTAS)
    it = LinearNDInterpolator(d, Q, fill_value=R.FILL)
    got = np.stack([it(x[None, :])[0] for x in q])  # one query per call: every walk starts at simplex 0
    return d, Q, q, dl, got


@pytest.mark.parametrize("name", CASES)
def test_restated_scan_equals_scipy(name):
    P, Q, axes, d = R.case(name)
    q = R.grid_queries(*axes)
    assert np.array_equal(R.brute_force(d, q, R.EPS_BROAD_FIND_SIMPLEX), d.find_simplex(q, bruteforce=True))


def test_restated_scan_equals_scipy_on_the_probes(probes):
    d, Q, q, dl, got = probes
    mine = R.brute_force(d, q, R.EPS_BROAD_FIND_SIMPLEX)
    assert np.array_equal(mine, d.find_simplex(q, bruteforce=True))
    # the constant matters: sqrt(DBL_EPSILON) gives other answers in the band, and only there
    other = R.brute_force(d, q, R.EPS_BROAD) != mine
    band = (dl > R.EPS_BROAD) & (dl < R.EPS_BROAD_FIND_SIMPLEX)
    assert other.any() and not other[~band].any()


@pytest.mark.parametrize("name", CASES)
def test_reference_is_explained(name):
    """No voxel of scipy's own output is unexplained: no share is left out."""
    un = R.unexplained(_reference(name), R.case_admissible(name))
    assert len(un) == 0, f"{name}: {len(un)} voxels of LinearNDInterpolator unexplained, first {un[:5]}"


@pytest.mark.parametrize("name", CASES)
def test_ambiguous_share(name):
    """Each case keeps the ambiguity it was built for; fill and a value are never both admissible
    (the bounds case may have such voxels: its grid has planes within eps of the bounding box)."""
    adm = R.case_admissible(name)
    print(R.share_line(name))
    if R.CASES[name]:
        assert (adm.n_accepting > 1).any()
    else:
        assert (adm.n_accepting <= 1).all()
    assert adm.fill_ok.any() == (name != "walk_from_0")  # every case but this one leaves the hull
    assert adm.has_value().any()
    if name != "bounds":
        assert not (adm.fill_ok & adm.has_value()).any()
    if name == "lattice_on":  # the one grid where two accepting simplices give different bits
        assert (adm.n_distinct() > 1).any()


def test_eps_broad_of_the_interpolator(probes):
    """LinearNDInterpolator scans with eps_broad = sqrt(DBL_EPSILON) (1.49e-8), not find_simplex's
    sqrt(100 DBL_EPSILON) (1.49e-7).  Probes at c = -delta across faces shared with flat simplices:
    at delta = 5e-9 (below both) the interpolator returns the neighbour-rule answer, the extrapolant
    of a simplex that does not accept the probe, so its walks do reach the scan there; at 3e-8, 5e-8
    and 1e-7 it never returns the answer of the larger constant, and returns that of the smaller."""
    d, Q, q, dl, got = probes
    narrow = R.brute_values(d, Q, q, R.FILL, R.EPS_BROAD)
    broad = R.brute_values(d, Q, q, R.FILL, R.EPS_BROAD_FIND_SIMPLEX)
    differ = (R._bits(narrow) != R._bits(broad)).any(axis=1)
    is_narrow = (R._bits(got) == R._bits(narrow)).all(axis=1)
    is_broad = (R._bits(got) == R._bits(broad)).all(axis=1)
    s_broad, step = R.brute_force(d, q, R.EPS_BROAD_FIND_SIMPLEX, with_step=True)
    acc = R.accepting(d, q)
    ok = R.valid_simplices(d)
    via_rule = (s_broad >= 0) & ~ok[np.maximum(step, 0)] & ~acc[np.arange(len(q)), np.maximum(s_broad, 0)]
    for x in DELTAS:
        s = dl == x
        print(f"delta {x:g}: probes {s.sum()}, the constants give different bits {np.sum(s & differ)}, "
              f"interpolator = sqrt(DBL_EPSILON) answer only {np.sum(s & differ & is_narrow & ~is_broad)}, "
              f"= sqrt(100 DBL_EPSILON) answer only {np.sum(s & differ & is_broad & ~is_narrow)}, neither "
              f"{np.sum(s & differ & ~is_broad & ~is_narrow)}; neighbour-rule answers {np.sum(s & via_rule)}, "
              f"returned {np.sum(s & via_rule & is_broad)}")
    band = (dl > R.EPS_BROAD) & (dl < R.EPS_BROAD_FIND_SIMPLEX)
    assert np.sum(band & differ) >= 100 and not (differ & ~band).any()
    assert not (band & differ & is_broad).any()
    assert np.sum(band & differ & is_narrow) >= 0.9 * np.sum(band & differ)
    low = dl == DELTAS[0]
    assert np.sum(low & via_rule & is_broad) >= 0.5 * np.sum(low & via_rule) > 0  # the scan was reached
    # and with the settled constant every probe is explained (with the other one, the band is not)
    assert len(R.unexplained(got, R.admissible(d, Q, q, R.FILL, R.EPS_BROAD))) == 0


@pytest.mark.parametrize("name", CASES)
def test_find_simplex_route_cannot_differ_on_the_fixtures(name):
    """oracle/cpu_ref.linear_points locates with Delaunay.find_simplex, whose scan uses the larger
    eps_broad.  On every grid of the suite the scan gives one answer under both constants (no voxel
    has a coordinate in [-1.49e-7, -1.49e-8) towards a flat simplex), so that route cannot differ."""
    P, Q, axes, d = R.case(name)
    if R.valid_simplices(d).all():
        return  # eps_broad enters the scan through a degenerate simplex only
    q = R.grid_queries(*axes)
    assert np.array_equal(R.brute_force(d, q, R.EPS_BROAD), R.brute_force(d, q, R.EPS_BROAD_FIND_SIMPLEX))


# -------------------------------------------------------------------------------------------------
# mutations: each must leave unexplained voxels (or, for the scan's pick, fail the bitwise comparison)
# -------------------------------------------------------------------------------------------------
MUTATION_CASES = ["lattice_off", "walk_from_0"]


def _scan(name, **kw):
    P, Q, axes, d = R.case(name)
    if not kw:  # the scan's answers are part of the cached admissible set
        adm = R.case_admissible(name)
        out = R.interpolate_in(d, Q, R.grid_queries(*axes), np.maximum(adm.scan, 0))
        out[adm.scan < 0] = R.FILL
        return out
    return R.brute_values(d, Q, R.grid_queries(*axes), R.FILL, R.EPS_BROAD, **kw)


@pytest.mark.parametrize("name", MUTATION_CASES + ["lattice_on"])
def test_mutation_non_accepting_neighbour(name):
    """Voxels with one accepting simplex, interpolated in a valid neighbour of it instead."""
    P, Q, axes, d = R.case(name)
    q = R.grid_queries(*axes)
    adm = R.case_admissible(name)
    got = _scan(name)
    ok = R.valid_simplices(d)
    one = np.nonzero(adm.n_accepting == 1)[0]
    s = adm.scan[one]
    nb = d.neighbors[s]  # (m, 4)
    usable = (nb >= 0) & ok[np.maximum(nb, 0)]
    one, nb, usable = one[usable.any(axis=1)], nb[usable.any(axis=1)], usable[usable.any(axis=1)]
    wrong = nb[np.arange(len(one)), usable.argmax(axis=1)]
    got[one] = R.interpolate_in(d, Q, q[one], wrong)
    un = R.unexplained(got, adm)
    print(f"{name}: {len(un)} of {len(one)} voxels moved to a neighbour are unexplained")
    assert len(one) > 0 and np.isin(un, one).all()
    assert len(un) >= 0.9 * len(one)  # an extrapolant equals the interpolant only where the gradients agree


@pytest.mark.parametrize("name", MUTATION_CASES)
def test_mutation_one_ulp(name):
    P, Q, axes, d = R.case(name)
    adm = R.case_admissible(name)
    got = _scan(name)
    assert len(R.unexplained(got, adm)) == 0
    v = int(np.nonzero(adm.has_value())[0][len(got) // 7 % int(adm.has_value().sum())])
    for c in range(3):
        bumped = got.copy()
        bumped[v, c] = np.nextafter(bumped[v, c], np.inf)
        assert np.array_equal(R.unexplained(bumped, adm), [v])
    # and one particle's value off by one ulp: seen at voxels of its simplices
    i = d.simplices[adm.scan[v]][np.argmax(R.barycentric_in(d, R.grid_queries(*axes)[[v]], adm.scan[[v]])[0])]
    Q2 = Q.copy()
    Q2[i, 0] = np.nextafter(Q2[i, 0], np.inf)
    un = R.unexplained(R.brute_values(d, Q2, R.grid_queries(*axes), R.FILL, R.EPS_BROAD), adm)
    assert len(un) > 0 and (d.simplices[adm.scan[un]] == i).any(axis=1).all()


@pytest.mark.parametrize("name", ["walk_from_0"])
def test_mutation_c3_summed_first(name):
    """c_3 = 1 - (c_0 + c_1 + c_2) rounds differently from ((1 - c_0) - c_1) - c_2 in general
    position.  (Not on the lattice: its transforms hold 0 and +-1 only, each c_i is one coordinate
    difference, and the two orders round alike on its grids.)"""
    un = R.unexplained(_scan(name, c3="sum"), R.case_admissible(name))
    print(f"{name}: {len(un)} voxels unexplained")
    assert len(un) > 0


def test_mutation_eps_tenfold():
    """A locator with eps = 1000 DBL_EPSILON: nodes of the on-plane grid moved 5e-14 (between eps and
    10 eps) across the lattice planes x = k.  The simplices behind the plane then accept, the scan
    stops at the first of them, and its extrapolant is off by 5e-14 times the jump of the gradient;
    beyond the hull plane the mutant writes a value where scipy writes the fill value."""
    P, Q, axes, d = R.case("lattice_on")
    q = R.grid_queries(*axes)
    q = q[(q[:, 0] == np.round(q[:, 0])) & (q[:, 0] >= 0) & (q[:, 0] <= 5)]
    q = np.concatenate([q + [5e-14, 0, 0], q - [5e-14, 0, 0]])
    adm = R.admissible(d, Q, q, R.FILL, R.EPS_BROAD)
    assert len(R.unexplained(R.brute_values(d, Q, q, R.FILL, R.EPS_BROAD), adm)) == 0
    un = R.unexplained(R.brute_values(d, Q, q, R.FILL, R.EPS_BROAD, eps=10 * R.EPS), adm)
    print(f"{len(un)} of {len(q)} probes unexplained")
    assert len(un) > 0
    assert (adm.fill_ok[un] & ~adm.has_value()[un]).any() and adm.has_value()[un].any()


def test_mutation_second_accepting_index():
    """The scan's answer is held bit for bit, not by the admissible set (the second accepting simplex
    is admissible by construction): stopping at the second index fails that comparison."""
    P, Q, axes, d = R.case("lattice_on")
    q = R.grid_queries(*axes)
    first = R.brute_force(d, q, R.EPS_BROAD)
    second = R.brute_force(d, q, R.EPS_BROAD, nth=1)
    has = second >= 0
    assert has.sum() > 100 and (first[has] >= 0).all()
    a = R.interpolate_in(d, Q, q[has], first[has])
    b = R.interpolate_in(d, Q, q[has], second[has])
    n = int((R._bits(a) != R._bits(b)).any(axis=1).sum())
    print(f"{n} of {has.sum()} voxels with a second accepting index change bits")
    assert n > 0


@pytest.mark.parametrize("name", MUTATION_CASES + ["lattice_on"])
def test_mutation_shifted_by_one_plane(name):
    """A correct value at the wrong voxel: the whole output moved by one z plane."""
    P, Q, axes, d = R.case(name)
    nz, ny, nx = len(axes[2]), len(axes[1]), len(axes[0])
    got = np.roll(_scan(name).reshape(nz, ny, nx, 3), 1, axis=0).reshape(-1, 3)
    un = R.unexplained(got, R.case_admissible(name))
    print(f"{name}: {len(un)} voxels unexplained")
    assert len(un) > 0.3 * len(got)
