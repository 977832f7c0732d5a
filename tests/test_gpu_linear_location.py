"""method='linear' held to scipy's point-location rule voxel by voxel (tests/_linear_ref.py; the
oracle's own checks are tests/test_linear_ref.py).  Runs only on an MI355X (``-m gpu``).

* ``k_linear_walk``: every voxel's (u, v, w) must be, to the bit, the interpolant of a simplex that
  scipy's rule accepts (or of the brute-force answer), and the fill value only where scipy's rule can
  end without a simplex.  No tolerance, no share left out.
* ``k_linear_brute``: walks forced to start in a degenerate simplex hand every in-box voxel to the
  scan, whose answer does not depend on a start: bit for bit scipy's first-index rule, alone and
  combined with z slabs, chunks, point grids, a fluid mask, NAN_TO_NUM and a fill value.
* The flag list exactly at its capacity (2^20 voxels) and one grid over it.

Not covered: the walk's step limit (4096 steps, then the scan).  No input of test size reaches it
and the library has no knob for it.
"""
import numpy as np
import pytest

from tests import _linear_ref as R

pytestmark = pytest.mark.gpu

FLAG_CAP = 1 << 20  # kLinearFlagCap (ptv_run_chunked.cpp)


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


# -------------------------------------------------------------------------------------------------
# the walk: explained, every voxel
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_voxel_is_explained(ctx, name):
    from ptv_interpolation_amd import _lib

    P, Q, axes, d = R.case(name)
    tri = _lib.Triangulation(d)
    if name == "walk_from_0":
        tri.vertex_to_simplex[:] = -1  # no start simplex: every walk starts at simplex 0
    got = ctx.interp_linear(P, Q, tri, axes=axes, fill_value=R.FILL)
    n_singular = ctx.stats["n_singular"]
    un = R.unexplained(got, R.case_admissible(name))
    print(f"{name}: brute-force voxels {n_singular}, unexplained {len(un)}")
    assert len(un) == 0, f"{len(un)} voxels unexplained, first {un[:5]}"
    if name == "lattice_off":
        assert n_singular > 0
    if name in ("one_simplex", "two_simplices", "walk_from_0", "bounds"):
        assert n_singular == 0  # no degenerate simplex to meet


# -------------------------------------------------------------------------------------------------
# the scan: forced, bit for bit
# -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced():
    """The on-plane lattice grid with every walk started in a degenerate simplex: (P, Q, axes,
    Triangulation, Delaunay, queries, in-box voxels), after the CPU-side checks that
    the inputs reach every part of the scan kernel."""
    from ptv_interpolation_amd import _lib

    P, Q, axes, d = R.case("lattice_on")
    ok = R.valid_simplices(d)
    tri = _lib.Triangulation(d)
    tri.vertex_to_simplex[:] = np.nonzero(~ok)[0][0]
    q = R.grid_queries(*axes)
    table = R.scan_table(d, q, R.EPS_BROAD)
    inbox = ~R.fully_outside(d, q)
    s, step = R.brute_force(d, q, R.EPS_BROAD, with_step=True)
    assert (s[inbox] >= 0).all() and not inbox.all()  # the lattice's hull is its box; outside it: fill
    # more than one round of 256 simplices
    assert ((step >= 0) & (step < 256)).any() and (step >= 256).any()
    # two accepting indices within the block of 256 that holds the first: the atomicMin pick
    hit = table >= 0
    first = hit.argmax(axis=1)
    blk = np.arange(table.shape[1])[None, :] // 256 == (first // 256)[:, None]
    assert ((hit & blk).sum(axis=1)[inbox & (s >= 0)] > 1).any()
    # answers through the degenerate-neighbour branch
    assert (~ok[step[(step >= 0) & inbox]]).any()
    return P, Q, axes, tri, d, q, inbox


def _expected(d, Q, q, fill, shape):
    return R.brute_values(d, Q, q, fill, R.EPS_BROAD).reshape(shape + (3,))


def test_forced_scan_whole_grid(ctx, forced):
    P, Q, axes, tri, d, q, inbox = forced
    got = ctx.interp_linear(P, Q, tri, axes=axes, fill_value=R.FILL)
    assert ctx.stats["n_singular"] == int(inbox.sum())
    ref = _expected(d, Q, q, R.FILL, (13, 13, 13))
    for c, a in enumerate(got):
        assert np.array_equal(a, ref[..., c]), f"{np.sum(a != ref[..., c])} voxels differ"


@pytest.mark.parametrize("z0,z1", [(0, 5), (5, 13)])
def test_forced_scan_slabs_and_chunks(ctx, forced, z0, z1):
    """flag_list holds slab-relative voxels of several chunks; the scan rebuilds the point from them."""
    P, Q, axes, tri, d, q, inbox = forced
    got = ctx.interp_linear(P, Q, tri, axes=axes, fill_value=R.FILL, z_range=(z0, z1), chunk_planes=2)
    assert ctx.stats["n_singular"] == int(inbox.reshape(13, 13, 13)[z0:z1].sum())
    ref = _expected(d, Q, q, R.FILL, (13, 13, 13))[z0:z1]
    for c, a in enumerate(got):
        assert a.shape == (z1 - z0, 13, 13)
        assert np.array_equal(a, ref[..., c]), f"{np.sum(a != ref[..., c])} voxels differ"


def test_forced_scan_point_grid(ctx, forced):
    P, Q, axes, tri, d, q, inbox = forced
    got = ctx.interp_linear(P, Q, tri, grid_points=(q[:, 0], q[:, 1], q[:, 2]), shape=(13, 13, 13), fill_value=R.FILL)
    assert ctx.stats["n_singular"] == int(inbox.sum())
    ref = _expected(d, Q, q, R.FILL, (13, 13, 13))
    for c, a in enumerate(got):
        assert np.array_equal(a, ref[..., c])
    sl = ctx.interp_linear(P, Q, tri, grid_points=(q[:, 0], q[:, 1], q[:, 2]), shape=(13, 13, 13), fill_value=R.FILL,
                           z_range=(5, 13), chunk_planes=2)
    for c, a in enumerate(sl):
        assert np.array_equal(a, ref[5:, ..., c])


def test_forced_scan_mask_nan_to_num_fill(ctx, forced):
    """Solid voxels are 0 and are not flagged; NaN values become 0 under NAN_TO_NUM; -5 where the
    scan finds no simplex."""
    from ptv_interpolation_amd import _lib

    P, Q, axes, tri, d, q, inbox = forced
    rng = np.random.default_rng(13)
    mask = rng.random((13, 13, 13)) < 0.7
    Qn = Q.copy()
    Qn[::7, 1] = np.nan
    got = ctx.interp_linear(P, Qn, tri, axes=axes, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM, fill_value=-5.0)
    assert ctx.stats["n_singular"] == int((inbox & mask.ravel()).sum())
    ref = _expected(d, Qn, q, -5.0, (13, 13, 13))
    assert np.isnan(ref[mask]).any() and (ref[mask] == -5.0).any()
    for c, a in enumerate(got):
        assert np.array_equal(a, np.where(mask, np.nan_to_num(ref[..., c]), 0.0))


# -------------------------------------------------------------------------------------------------
# the flag list's capacity
# -------------------------------------------------------------------------------------------------
def test_flag_list_exactly_full(ctx, forced):
    """1024 x 1024 x 1 voxels strictly inside the lattice's box, all flagged: 2^20, the capacity."""
    P, Q, _, tri, d, _, _ = forced
    ax = np.linspace(0.013, 4.987, 1024)
    ay = np.linspace(0.021, 4.979, 1024)
    az = np.array([2.3])
    got = ctx.interp_linear(P, Q, tri, axes=(ax, ay, az), fill_value=R.FILL)
    assert ctx.stats["n_singular"] == FLAG_CAP
    sel = np.unique(np.concatenate([[0, FLAG_CAP - 1], np.random.default_rng(14).integers(0, FLAG_CAP, 20000)]))
    q = np.stack([ax[sel % 1024], ay[sel // 1024], np.full(len(sel), az[0])], -1)
    ref = R.brute_values(d, Q, q, R.FILL, R.EPS_BROAD)
    assert (ref != R.FILL).all()
    for c, a in enumerate(got):
        assert np.array_equal(a.ravel()[sel], ref[:, c]), f"{np.sum(a.ravel()[sel] != ref[:, c])} voxels differ"


def test_flag_list_over_capacity_raises(ctx, forced):
    """102^3 = 1,061,208 flagged voxels: refused (PTV_E_UNSUPPORTED), naming the limit."""
    P, Q, _, tri, d, _, _ = forced
    a = np.linspace(0.013, 4.987, 102)
    with pytest.raises(NotImplementedError, match=rf"{102 ** 3} voxels.*limit {FLAG_CAP}"):
        ctx.interp_linear(P, Q, tri, axes=(a, a, a), fill_value=R.FILL)
    # the context is usable afterwards
    got = ctx.interp_linear(P, Q, tri, axes=(a[:3], a[:3], a[:3]), fill_value=R.FILL)
    assert ctx.stats["n_singular"] == 27 and np.isfinite(got[0]).all()
