"""The k-NN outlier filter (csrc/ptv_filter.hip and the filter epilogue of the search kernel) held to
the oracle at its edges: ``keep`` against ``cpu_ref.outlier_filter`` and the (k+1)-th distance
against ``KDTree.query(points, k + 1)``, bit for bit.

Every list length k = 1..126 (each a different pick position and padding of the epilogue's median
network), clouds barely larger than k and around one wave tile and one block of queries, NaN and
infinite velocities (a real +inf speed beside the network's +inf padding), speeds that repeat
exactly (medians on a tie, MAD exactly 0), thresholds and MAD offsets other than the defaults, the
device-pointer entry, and coincident particles off their tie-dependent decisions.

Cases: tests/_rows_edges.py.  tests/test_rows_edge_cases.py shows the clouds free of ties and the
oracle's tree and brute-force searches agreeing on them.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _rows_edges as E
from tests._util import filter_ties

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _expected(P, Q, k, threshold=3.0, mad_eps=1e-6):
    """(keep, kth): the oracle's keep mask (its restatement with `mad_eps` free where that is not
    1e-6; test_rows_edge_cases.py holds the two equal at 1e-6) and the tree's (k+1)-th distance."""
    with np.errstate(all="ignore"):
        keep, kth = E.filter_ref(P, Q, k, threshold=threshold, mad_eps=mad_eps)
        if mad_eps == 1e-6:
            oracle, radius = cpu_ref.outlier_filter(P, Q, k, threshold)
            assert np.array_equal(keep, oracle) and radius == np.median(kth)
    return keep, kth


def _check(ctx, P, Q, k, threshold=3.0, mad_eps=1e-6, skip=None):
    keep, kth = ctx.filter_outliers_knn(P, Q, k=k, threshold=threshold, mad_eps=mad_eps)
    exp_keep, exp_kth = _expected(P, Q, k, threshold, mad_eps)
    assert keep.dtype == np.uint8 and keep.shape == exp_keep.shape and set(np.unique(keep)) <= {0, 1}
    assert kth.dtype == np.float64 and np.array_equal(kth, exp_kth), (k, threshold, mad_eps)
    sel = slice(None) if skip is None else ~skip
    assert np.array_equal(keep.view(bool)[sel], exp_keep[sel]), (k, threshold, mad_eps)
    return exp_keep


@pytest.mark.parametrize("k", E.SWEEP_KS)
def test_filter_every_list_length(ctx, k):
    """700 particles (not a multiple of 64), 20 planted outliers, every k served by the search
    kernel's epilogue."""
    P, Q = E.sweep_cloud()
    exp = _check(ctx, P, Q, k)
    assert not exp.all()


@pytest.mark.parametrize("k,n", E.tiny_cases(), ids=lambda v: str(v))
def test_filter_tiny_clouds(ctx, k, n):
    P, Q = E.tiny_cloud(k, n)
    _check(ctx, P, Q, k)


@pytest.mark.parametrize("k", E.NONFINITE_KS)
def test_filter_nonfinite_velocities(ctx, k):
    """A NaN among the neighbours' speeds makes median, MAD and z NaN, which compares False: removed.
    An infinite speed sorts beside the median network's +inf padding."""
    P, Q = E.nonfinite_cloud()
    exp = _check(ctx, P, Q, k)
    assert not exp[~np.isfinite(Q).all(axis=1)].any() and exp.any()


@pytest.mark.parametrize("k", E.QUANT_KS)
@pytest.mark.parametrize("kind", E.QUANT_KINDS)
def test_filter_quantised_speeds(ctx, kind, k):
    P, Q = E.quantised_cloud(kind)
    _check(ctx, P, Q, k)


@pytest.mark.parametrize("mad_eps", E.MAD_EPS)
@pytest.mark.parametrize("threshold", E.THRESHOLDS)
@pytest.mark.parametrize("k", E.PARAM_KS)
@pytest.mark.parametrize("name", ["continuous", "levels"])
def test_filter_parameters(ctx, name, k, threshold, mad_eps):
    """mad_eps = 0 with MAD = 0: 0/0 -> NaN and x/0 -> inf, both removed, as numpy decides."""
    P, Q = E.param_clouds()[name]
    _check(ctx, P, Q, k, threshold=threshold, mad_eps=mad_eps)


@pytest.mark.parametrize("k", E.DUP_KS)
def test_filter_coincident_points(ctx, k):
    """30 coincident pairs: the decisions that depend on the tree's tie order are excluded (under the
    stated cap); everything else, and every (k+1)-th distance, is compared."""
    P, Q = E.coincident_cloud()
    ties = filter_ties(P, k)
    assert 0 < ties.mean() < E.DUP_CAP
    _check(ctx, P, Q, k, skip=ties)
    print(f"coincident points, k = {k}: excluded share {ties.mean():.4f}")


@pytest.mark.parametrize("case", ["continuous", "nonfinite"])
def test_filter_device_entry_equals_host_entry(ctx, case):
    import torch

    P, Q = E.sweep_cloud() if case == "continuous" else E.nonfinite_cloud()
    k = 25
    n = len(P)
    keep_h, kth_h = ctx.filter_outliers_knn(P, Q, k=k, threshold=2.5, mad_eps=1e-3)
    cols = [torch.from_numpy(np.ascontiguousarray(A[:, i])).cuda() for A in (P, Q) for i in range(3)]
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    kth = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.filter_outliers_knn_dev(n, [c.data_ptr() for c in cols], keep.data_ptr(), kth.data_ptr(), k=k, threshold=2.5,
                                mad_eps=1e-3, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert keep.cpu().numpy().tobytes() == keep_h.tobytes()
    assert kth.cpu().numpy().tobytes() == kth_h.tobytes()
    exp_keep, exp_kth = _expected(P, Q, k, 2.5, 1e-3)
    assert np.array_equal(keep_h.view(bool), exp_keep) and np.array_equal(kth_h, exp_kth)
