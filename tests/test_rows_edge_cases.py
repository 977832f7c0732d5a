"""The oracle of the mask, divergence and outlier-filter rows (oracle/cpu_ref.py) against scipy and
numpy themselves, on the edge cases of tests/_rows_edges.py: the GPU tests of those cases
(tests/test_gpu_{mask,div,filter}_edges.py) then compare against something proven.  No GPU.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _rows_edges as E
from tests._util import filter_ties


# ----------------------------------------------------------------------------- mask sampling
def _scipy_sample(raw, bounds, X, Y, Z):
    """sample_mask_on_grid as the reference states it: RegularGridInterpolator 'nearest' over the raw
    axes linspace(min, max - 1, n), fill 0, then > 0.5."""
    from scipy.interpolate import RegularGridInterpolator

    nz, ny, nx = raw.shape
    (xmin, xmax), (ymin, ymax), (zmin, zmax) = bounds
    z, y, x = (np.linspace(lo, hi - 1, n) for lo, hi, n in ((zmin, zmax, nz), (ymin, ymax, ny), (xmin, xmax, nx)))
    rgi = RegularGridInterpolator((z, y, x), raw.astype(float), method="nearest", bounds_error=False, fill_value=0)
    return rgi(np.stack([Z.ravel(), Y.ravel(), X.ravel()], -1)).reshape(X.shape) > 0.5


@pytest.mark.parametrize("case", E.mask_sample_cases() + [("slab",) + E.slab_case()], ids=lambda c: c[0])
def test_sample_mask_oracle_equals_scipy(case):
    """Exact half-way points, descending axes, both in-bounds end points and their neighbouring
    floats, length-1 raw axes.  scipy 1.15 accepts a length-1 axis (every other coordinate than the
    axis point itself is out of bounds), so that rule too is checked against scipy, not restated."""
    _, raw, bounds, (ax, ay, az) = case
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    with np.errstate(invalid="ignore"):
        exp = _scipy_sample(raw, bounds, X, Y, Z)
        got = cpu_ref.sample_mask_nearest(raw, bounds, X, Y, Z)
    assert got.dtype == np.bool_ and np.array_equal(got, exp)
    assert exp.any() and not exp.all()


def test_rgi_nearest_index_rules():
    """The rules ptv_mask.hip states: t <= 0.5 keeps the lower voxel (of the ascending axis, so the
    higher index of a descending one), the end points are in bounds, and on a length-1 axis only
    x == g[0] is."""
    g = np.arange(4.0)
    x = np.array([-1e-300, 0.0, 0.5, np.nextafter(0.5, 1), 1.5, 2.5, 3.0, np.nextafter(3.0, 4), np.nan])
    assert cpu_ref.rgi_nearest_index(g, x).tolist() == [-1, 0, 0, 1, 1, 2, 3, -1, -1]
    assert cpu_ref.rgi_nearest_index(g[::-1], x).tolist() == [-1, 3, 3, 2, 2, 1, 0, -1, -1]
    one = np.array([2.0])
    assert cpu_ref.rgi_nearest_index(one, [np.nextafter(2.0, 0), 2.0, np.nextafter(2.0, 3)]).tolist() == [-1, 0, -1]


# ----------------------------------------------------------------------------- boundary particles
def _scipy_boundary(mask, bounds, step, thickness):
    from scipy import ndimage

    nz, ny, nx = mask.shape
    iz, iy, ix = np.where(ndimage.binary_dilation(mask != 0, iterations=thickness) & ~mask)
    if len(ix) == 0:
        return (np.array([]),) * 3
    iz, iy, ix = iz[::step], iy[::step], ix[::step]
    return tuple(lo + i * (hi - 1 - lo) / (n - 1) if n > 1 else np.full_like(i, lo)
                 for i, (lo, hi), n in zip((ix, iy, iz), bounds, (nx, ny, nz)))


def _same_particles(got, exp):
    assert len(got) == len(exp) == 3
    for a, e in zip(got, exp):
        assert a.dtype == e.dtype and a.shape == e.shape and np.array_equal(a, e)


@pytest.mark.parametrize("shape", E.SWAR_SHAPES + E.GENERIC_SHAPES, ids=str)
@pytest.mark.parametrize("kind", E.MASK_KINDS)
def test_boundary_oracle_equals_scipy(kind, shape):
    m = E.bool_mask(kind, shape)
    b = E.shape_bounds(shape)
    for t in E.THICKNESSES:
        for step in E.STEPS:
            _same_particles(cpu_ref.boundary_particles(m, b, step, t), _scipy_boundary(m, b, step, t))


@pytest.mark.parametrize("dtype", E.WIDE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(6, 9, 48), (6, 9, 47)], ids=str)
def test_boundary_oracle_wide_integers_equal_scipy(shape, dtype):
    m = E.wide_mask(shape, dtype)
    assert (m == 0).any() and (m & 1).any() and ((m != 0) & (m & 1 == 0)).any()
    if np.dtype(dtype).itemsize > 1:
        assert ((m != 0) & (m.astype(np.uint8) == 0)).any()  # non-zero with a zero low byte
    b = E.shape_bounds(shape)
    for t in (1, 3):
        for step in E.STEPS:
            exp = _scipy_boundary(m, b, step, t)
            assert len(exp[0]) > 0
            _same_particles(cpu_ref.boundary_particles(m, b, step, t), exp)


@pytest.mark.parametrize("shape", E.SCAN_SHAPES, ids=str)
def test_boundary_oracle_scan_cases_equal_scipy(shape):
    m = E.scan_mask(shape)
    assert m.size > 1024 * 4096  # more than 1024 count blocks
    b = E.shape_bounds(shape)
    for step in (1, 5):
        exp = _scipy_boundary(m, b, step, 2)
        assert len(exp[0]) > 1000
        _same_particles(cpu_ref.boundary_particles(m, b, step, 2), exp)


@pytest.mark.parametrize("shape", E.DEGENERATE_SHAPES, ids=str)
def test_boundary_oracle_degenerate_axes_equal_scipy(shape):
    m = E.degenerate_mask(shape)
    b = E.shape_bounds(shape)
    for t in E.THICKNESSES:
        for step in E.STEPS + (10**6,):
            _same_particles(cpu_ref.boundary_particles(m, b, step, t), _scipy_boundary(m, b, step, t))


# ----------------------------------------------------------------------------- divergence
@pytest.mark.parametrize("dtype", [np.int16, np.int64], ids=lambda d: np.dtype(d).name)
def test_divergence_oracle_integer_fields(dtype):
    """(int + int) / 2.0 is float64 in the reference: the faces of an integer field keep their
    halves, so the oracle on integers equals the oracle on the same values as float64."""
    rng = np.random.default_rng(5)
    shape = (5, 6, 7)
    u, v, w = (rng.integers(-9, 10, shape).astype(dtype) for _ in range(3))
    m = rng.uniform(size=shape) < 0.6
    got = cpu_ref.consistent_divergence(u, v, w, m, 0.5, 1.0, 2.0)
    exp = cpu_ref.consistent_divergence(u.astype(float), v.astype(float), w.astype(float), m, 0.5, 1.0, 2.0)
    assert got.dtype == np.float64 and np.array_equal(got, exp)
    assert (got * 4 % 2 != 0).any()  # some face average ends in .5


# ----------------------------------------------------------------------------- outlier filter
@pytest.mark.parametrize("case", E.all_filter_clouds(), ids=lambda c: c[0])
def test_filter_clouds_free_of_ties(case):
    name, P, ks, may_tie = case
    for k in ks:
        ties = filter_ties(P, k)
        if may_tie:
            assert 0 < ties.mean() < E.DUP_CAP, (k, ties.mean())
        else:
            assert not ties.any(), (name, k)


def _agree(P, Q, k, **kw):
    with np.errstate(all="ignore"):
        a, da = E.filter_ref(P, Q, k, knn="kdtree", **kw)
        b, db = E.filter_ref(P, Q, k, knn="bruteforce", **kw)
    assert np.array_equal(a, b) and np.array_equal(da, db), k
    return a


@pytest.mark.parametrize("group", range(6))
def test_filter_sweep_tree_and_bruteforce_agree(group):
    P, Q = E.sweep_cloud()
    for k in E.SWEEP_KS[group::6]:
        keep = _agree(P, Q, k)
        a, _ = cpu_ref.outlier_filter(P, Q, k, 3.0, knn="kdtree")
        b, _ = cpu_ref.outlier_filter(P, Q, k, 3.0, knn="bruteforce")
        assert np.array_equal(a, b) and np.array_equal(a, keep)  # filter_ref restates the oracle at 1e-6
        assert not keep.all()


def test_filter_tiny_tree_and_bruteforce_agree():
    for k, n in E.tiny_cases():
        P, Q = E.tiny_cloud(k, n)
        keep = _agree(P, Q, k)
        assert np.array_equal(keep, cpu_ref.outlier_filter(P, Q, k, 3.0)[0])


def test_filter_nonfinite_tree_and_bruteforce_agree():
    P, Q = E.nonfinite_cloud()
    bad = ~np.isfinite(Q).all(axis=1)
    assert bad.sum() == 24
    for k in E.NONFINITE_KS:
        keep = _agree(P, Q, k)
        with np.errstate(all="ignore"):
            assert np.array_equal(keep, cpu_ref.outlier_filter(P, Q, k, 3.0)[0])
        assert not keep[bad].any() and not keep[~bad].all() and keep.any()


@pytest.mark.parametrize("kind", E.QUANT_KINDS)
def test_filter_quantised_tree_and_bruteforce_agree(kind):
    P, Q = E.quantised_cloud(kind)
    for k in E.QUANT_KS:
        keep = _agree(P, Q, k)
        assert np.array_equal(keep, cpu_ref.outlier_filter(P, Q, k, 3.0)[0])
        if kind == "levels":
            assert keep.any() and (k > 9 or not keep.all())  # MAD exactly 0 in the short lists
        elif kind == "one_outlier":
            assert (~keep).nonzero()[0].tolist() == [137]
        else:
            assert keep.all()


def test_filter_parameters_tree_and_bruteforce_agree():
    for name, (P, Q) in E.param_clouds().items():
        for k in E.PARAM_KS:
            for thr in E.THRESHOLDS:
                for eps in E.MAD_EPS:
                    _agree(P, Q, k, threshold=thr, mad_eps=eps)
    # mad_eps = 0 on repeated speeds: 0/0 -> NaN and x/0 -> inf both remove the particle
    P, Q = E.param_clouds()["levels"]
    with np.errstate(all="ignore"):
        keep0, _ = E.filter_ref(P, Q, 8, threshold=1e9, mad_eps=0.0)
        keep1, _ = E.filter_ref(P, Q, 8, threshold=1e9, mad_eps=1.0)
    assert keep1.all() and not keep0.all() and keep0.any()


def test_filter_coincident_case_agrees_off_the_ties():
    P, Q = E.coincident_cloud()
    assert len(P) == 1000 and len(np.unique(P, axis=0)) == 970
    for k in E.DUP_KS:
        ties = filter_ties(P, k)
        with np.errstate(all="ignore"):
            a, da = E.filter_ref(P, Q, k, knn="kdtree")
            b, db = E.filter_ref(P, Q, k, knn="bruteforce")
        assert np.array_equal(a[~ties], b[~ties]) and np.array_equal(da, db)
