"""GPU checks of the cubic B-spline prefilter and the order 0 / 1 / 3 sampling
(ptv_interpolation_amd/csrc/ptv_mesh.hip behind ``sampling.spline_filter_nearest`` and
``sampling.map_coordinates``) off the recorded fixtures: the seeded shapes, fields and coordinates of
tests/_spline_edges.py, which reach every chunk count of the x pass, a full last block of rows, both
sides of the start sum's switch on each axis, long strided axes, one sample, format extremes, and
coordinates across the pad, past it and out to 1e18.

The bar is test_gpu_mesh.py's: a value g passes when |g - exact| <= 8 * max(gap, eps * scale), with
``exact`` the long-double chain of tests/_mesh_ref.py (held to scipy in test_spline_edge_cases.py),
``gap`` = |scipy - exact| computed here from scipy on the same case, and ``scale`` max|coefficient|
for the coefficients and order 3, max|field| for order 1.  Order 0 is compared bit for bit.  The
ratios |g - exact| / max(gap, eps * scale) are printed before each assertion and, with
PTV_MESH_PARITY_OUT set to a path, appended to that file (profiles/spline_edges_parity.txt is such a
run).

Measured on an MI355X (profiles/spline_edges_parity.txt): every ratio lies within the bar, the
largest being 4.7 for the coefficients, 1.6 for the order-3 samples (1.1 within the padded extent)
and 0.42 for the order-1 samples.
"""
import numpy as np
import pytest
from scipy import ndimage

import _mesh_ref as mref
import _spline_edges as se
from test_gpu_mesh import note, ratios

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sampling():
    from ptv_interpolation_amd import _lib, sampling

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return sampling


@pytest.mark.parametrize("case", se.CASES, ids=se.case_id)
def test_prefilter_and_samples_within_the_bar(sampling, case):
    r = se.reference(*case)
    name = se.case_id(case)
    coef = sampling.spline_filter_nearest(r.field)
    assert coef.shape == r.coef.shape and coef.dtype == np.float64
    q = ratios(coef, r.coef, r.coef_gap(), r.cmax)
    note(f"spline-edges {name} coefficients: max |g - exact| / max(gap, eps scale) = {q.max():.3f}")
    assert np.all(q <= 8.0)
    for order in (3, 1):
        s = sampling.map_coordinates(r.field, r.points, order=order)
        assert s.shape == (r.points.shape[1],) and s.dtype == np.float64
        q = ratios(s, r.exact[order], r.gap(order), r.scale[order])
        for where, sel in (("within the pad", ~r.far), ("past the pad", r.far)):
            note(f"spline-edges {name} order {order} {where}: max |g - exact| / max(gap, eps scale) = "
                 f"{q[sel].max():.3f}")
        assert np.all(q <= 8.0), (order, r.points[:, q > 8.0][:, :5], q[q > 8.0][:5])
    assert np.array_equal(sampling.map_coordinates(r.field, r.points, order=0), r.exact[0])


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_point_counts_around_a_block(sampling, count):
    """Blocks of 256 points: a count gives the first ``count`` samples of the whole set, which the
    case above holds to the bar."""
    r = se.reference("normal", (5, 6, 7))
    for order in (0, 1, 3):
        whole = sampling.map_coordinates(r.field, r.points, order=order)
        part = sampling.map_coordinates(r.field, r.points[:, :count], order=order)
        assert part.shape == (count,) and np.array_equal(part, whole[:count]), order


def test_small_field_after_a_larger_one(sampling):
    """The context's buffers have grown for the larger field and its coefficients are resident: the
    small field's samples are the same bits as before, fresh and from its resident coefficients."""
    small, large = se.reference("normal", (1, 1, 1)), se.reference("normal", (1, 1, 200))
    before = sampling.map_coordinates(small.field, small.points, order=3)
    coef_before = sampling.spline_filter_nearest(small.field)
    sampling.map_coordinates(large.field, large.points, order=3)
    fresh = sampling.map_coordinates(small.field, small.points, order=3)
    resident = sampling.map_coordinates(None, small.points, order=3, shape=small.shape)
    assert np.array_equal(fresh, before) and np.array_equal(resident, fresh)
    sampling.spline_filter_nearest(large.field)
    assert np.array_equal(sampling.spline_filter_nearest(small.field), coef_before)
    # and the larger one's resident coefficients, after the small field's orders 0 and 1 (which filter nothing)
    first = sampling.map_coordinates(large.field, large.points, order=3)
    sampling.map_coordinates(small.field, small.points, order=1)
    sampling.map_coordinates(small.field, small.points, order=0)
    assert np.array_equal(sampling.map_coordinates(None, large.points, order=3, shape=large.shape), first)


@pytest.mark.parametrize("kind", se.TYPED)
def test_typed_input_is_its_float64_widening(sampling, kind):
    r = se.reference(kind, (5, 6, 7))
    wide = se.widen(r.field)
    assert r.field.dtype != np.float64
    assert np.array_equal(sampling.spline_filter_nearest(r.field), sampling.spline_filter_nearest(wide))
    for order in (0, 1, 3):
        assert np.array_equal(sampling.map_coordinates(r.field, r.points, order=order),
                              sampling.map_coordinates(wide, r.points, order=order)), order


def test_trailing_shape_and_repeatability(sampling):
    r = se.reference("normal", (2, 2, 105))
    pts = r.points[:, :300]
    for order in (0, 1, 3):
        flat = sampling.map_coordinates(r.field, pts, order=order)
        shaped = sampling.map_coordinates(r.field, pts.reshape(3, 4, 75), order=order)
        assert shaped.shape == (4, 75) and shaped.tobytes() == flat.tobytes(), order
        assert sampling.map_coordinates(r.field, pts, order=order).tobytes() == flat.tobytes(), order
    assert sampling.spline_filter_nearest(r.field).tobytes() == sampling.spline_filter_nearest(r.field).tobytes()


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_non_finite_sample(sampling, value):
    """Orders 0 and 1 read the raw field: NaN and Inf appear exactly where scipy has them (Inf under a
    positive weight, NaN under a zero one) and the other samples stay within the bar.  Order 3: one
    non-finite sample reaches every coefficient through the three backward sweeps; scipy's are NaN
    or Inf, the double-double recursion's NaN, so finiteness is compared and not the kind."""
    field, pts = se.nonfinite_case(value)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = {o: ndimage.map_coordinates(field, pts, order=o, mode="nearest") for o in (0, 1, 3)}
        ref_coef = ndimage.spline_filter(np.pad(field, mref.PAD, mode="edge"), 3, mode="nearest")
        exact1 = mref.sample1(field, pts)
    got0 = sampling.map_coordinates(field, pts, order=0)
    assert (~np.isfinite(ref[0])).any() and np.array_equal(got0, ref[0], equal_nan=True)
    got1 = sampling.map_coordinates(field, pts, order=1)
    assert np.isnan(ref[1]).any() and np.isfinite(ref[1]).any() and (np.isnan(value) or np.isinf(ref[1]).any())
    assert np.array_equal(np.isnan(got1), np.isnan(ref[1]))
    inf = np.isinf(ref[1])
    assert np.array_equal(np.isinf(got1), inf) and np.array_equal(got1[inf], ref[1][inf])
    ok = np.isfinite(ref[1])
    fmax = np.abs(field[np.isfinite(field)]).max()
    q = ratios(got1[ok], exact1[ok], np.abs(ref[1][ok].astype(mref.LD) - exact1[ok]).astype(np.float64), fmax)
    note(f"spline-edges one {value} sample, order 1 finite samples: max |g - exact| / max(gap, eps scale) = "
         f"{q.max():.3f}")
    assert np.all(q <= 8.0)
    coef = sampling.spline_filter_nearest(field)
    assert np.array_equal(~np.isfinite(coef), ~np.isfinite(ref_coef))
    got3 = sampling.map_coordinates(field, pts, order=3)
    assert np.array_equal(~np.isfinite(got3), ~np.isfinite(ref[3]))


def test_beyond_scipys_range_the_sample_is_the_saturated_one(sampling):
    """From 1e19 scipy's integer cast overflows and it returns garbage; the device keeps the value it
    saturates to one sample past the pad, the same bits as at +-1e6."""
    r = se.reference("normal", (5, 6, 7))
    base = np.repeat(np.array([[1.3], [2.6], [3.1]]), 6, axis=1)
    for axis in range(3):
        far, ref = base.copy(), base.copy()
        far[axis] = [2.0 ** 63, 1e19, 1e300, -2.0 ** 63, -1e19, -1e300]
        ref[axis] = [1e6, 1e6, 1e6, -1e6, -1e6, -1e6]
        for order in (0, 1, 3):
            assert np.all(sampling.map_coordinates(r.field, far, order=order) ==
                          sampling.map_coordinates(r.field, ref, order=order)), (axis, order)
