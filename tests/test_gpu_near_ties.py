"""GPU parity at near ties the packed keys merge (tests/_near_ties.py): two different d2 that share a
key truncation, on particles with different values, so that the order inside the list and, at the
k-th / (k+1)-th boundary, the neighbour set have one right answer.  Runs only on an MI355X (``-m gpu``).

For 13 <= k <= 127 the search orders its candidates by (truncated d2, slot).  What makes the result
exact is the ``same_trunc(k-th, (k+1)-th)`` test of the k-NN kernel, the ascending check of the exact
d2 (``keys_ascend``, and the one in ``keylist_interp``) and the exact pair-list rerun of the tiles
they list, with ``kscale`` widening every key-derived bound.  The tests with exact ties on one value
(tests/test_gpu_keys.py) give the same bits for any order and any set; these do not: with the
same_trunc test off, or the ascending check off, the tests of this file fail
(profiles/near_ties_parity.txt).

Every comparison is against ``oracle.cpu_ref`` on brute-force lists of the same arrays, leaves out
only the voxels with an exact d2 tie on differing values among the first k + 1
(tests/test_near_tie_cases.py holds their share at 5 % at most) and asserts that at least 95 %
remain: IDW p = 2 and nearest bit for bit, Sibson normwise 1e-10, the outlier filter's keep mask and
k-th distance equal, local RBF against the extended-precision solve.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _geometry as G
from tests import _near_ties as NT
from tests._util import normwise

pytestmark = pytest.mark.gpu

TOL_SIBSON = 1e-10  # tests/test_gpu_keys.py
TOL_RBF = 1e-10     # tests/test_gpu_rbf.py: gpu-vs-exact <= max(TOL, lapack-vs-exact)
KEPT_MIN = 1.0 - NT.EXCLUDED_CAP


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _knn(ctx, name, k, method="idw", **kw):
    from ptv_interpolation_amd import _lib

    m = _lib.METHOD_NEAREST if k == 1 else {"sibson": _lib.METHOD_SIBSON, "idw": _lib.METHOD_IDW}[method]
    P, Q, ax, ay, az = NT.case(name, k)
    return ctx.interp_knn(P, Q, axes=(ax, ay, az), method=m, k=k, **kw)


def _uses_keys(k):
    return 13 <= k <= 127


def _compare(ctx, got, name, k, what="", planes=slice(None), method="idw"):
    """got against the oracle on the voxels without an exact tie on differing values; the figures are
    printed before anything is asserted.  Returns n_repair_tiles of the call."""
    rep = ctx.stats["n_repair_tiles"]
    keep = NT.keep(name, k)[planes]
    ref = [a[planes] for a in NT.oracle_knn(name, k, method)]
    inl, bnd = NT.near_tie_shares(name, k)
    diff = [int(np.sum(a[keep] != b[keep])) for a, b in zip(got, ref)]
    print(f"{name} k={k} {'nearest' if k == 1 else method}{what} (2^-{NT.exponent(name, k)}): excluded {1.0 - keep.mean():.2%}, "
          f"near tie in list {inl:.2%}, at boundary {bnd:.2%}, n_repair_tiles {rep}, differing voxels {diff} of {keep.sum()}")
    if method == "sibson":
        err = [normwise(a[keep], b[keep]) for a, b in zip(got, ref)]
        print(f"{name} k={k} sibson: normwise {err}")
        assert max(err) <= TOL_SIBSON
    else:
        assert diff == [0, 0, 0]
    assert keep.mean() >= KEPT_MIN
    return rep


# ---------------------------------------------------------------------------------------------
# twins: every list kind against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", NT.K_PAIRS + NT.K_KEYS + NT.K_BIG)
def test_idw_twins(ctx, k):
    """The exact pair lists (k = 7, 8, 12), every key-list length with an odd and an even k, and the
    large-k path (129, 130), bit for bit.  With key lists and an odd k the list ends inside a pair of
    twins at most voxels (tests/test_near_tie_cases.py), so tiles must have gone to the repair."""
    rep = _compare(ctx, _knn(ctx, "twins", k), "twins", k)
    if _uses_keys(k) and k % 2 == 1:
        assert rep > 0


@pytest.mark.parametrize("k", NT.K_SIBSON)
def test_sibson_twins(ctx, k):
    rep = _compare(ctx, _knn(ctx, "twins", k, method="sibson"), "twins", k, method="sibson")
    if k % 2 == 1:
        assert rep > 0


def test_nearest_twins(ctx):
    """The nearest particle and its twin are a near tie; the output is the nearer one's value."""
    _compare(ctx, _knn(ctx, "twins", 1), "twins", 1)


# ---------------------------------------------------------------------------------------------
# the displacement from separable to a few ulps; scaled and lattice-sized variants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", NT.GAPS)
@pytest.mark.parametrize("k", NT.K_VARIANT)
def test_idw_twins_gap(ctx, k, e):
    """Twins 2^-36 (few near ties), 2^-40 (on the truncation step), 2^-43 and 2^-47 apart."""
    _compare(ctx, _knn(ctx, f"twins_gap_{e}", k), f"twins_gap_{e}", k)


@pytest.mark.parametrize("k", NT.K_VARIANT)
def test_fewer_repairs_when_the_twins_are_separable(ctx, k):
    """At 2^-36 few pairs share a truncation, at 2^-43 almost all: fewer tiles go to the repair."""
    rep = {}
    for e in (36, 43):
        _knn(ctx, f"twins_gap_{e}", k)
        rep[e] = ctx.stats["n_repair_tiles"]
    print(f"k={k}: n_repair_tiles {rep}")
    assert rep[36] < rep[43]


@pytest.mark.parametrize("variant", [f"scale_2^{e}" for e in NT.SCALES] + ["dense"])
@pytest.mark.parametrize("k", NT.K_VARIANT)
def test_idw_twins_variants(ctx, k, variant):
    """Scaled by 2^80 and 2^-80 (kscale and the truncation are relative), and on the 45 x 41 x 40 grid,
    where the coarse lattice's k-distance launch takes its bounds from near-tied key lists
    (``bd[KMAX-2] * kscale``)."""
    _compare(ctx, _knn(ctx, "twins@" + variant, k), "twins@" + variant, k)


@pytest.mark.parametrize("k", NT.K_VARIANT)
def test_slab_cull_map_on_the_lattice_grid(ctx, k):
    """PTV_FLAG_SLAB_CULL_AUTO on the slab G.DENSE_SLAB of twins@dense, three calls (binned whole,
    culled with the cached map and proven, speculative), as tests/test_gpu_geometry.py runs it: equal
    bits each time, the proven cull on the second and third call."""
    from ptv_interpolation_amd import _lib

    z0, z1 = G.DENSE_SLAB
    outs, proven = [], []
    for call in range(3):
        got = _knn(ctx, "twins@dense", k, z_range=(z0, z1), flags=_lib.FLAG_SLAB_CULL_AUTO)
        proven.append(ctx.stats["halo_required"])
        _compare(ctx, got, "twins@dense", k, what=f" slab call {call}, binned {ctx.stats['n_binned']}", planes=slice(z0, z1))
        outs.append(got)
    for c in range(3):
        assert np.array_equal(outs[0][c], outs[1][c]) and np.array_equal(outs[0][c], outs[2][c])
    assert proven[1:] == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------
# call modes at k = 21
# ---------------------------------------------------------------------------------------------
def test_call_modes(ctx):
    """Point-list queries, a fluid mask, the whole-launch rerun (PTV_FLAG_KNN_REPAIR_ALL) and two uneven
    z-slabs equal the oracle; the whole-launch rerun also equals the listed rerun on every voxel."""
    from ptv_interpolation_amd import _lib

    k = NT.K_MODES
    P, Q, ax, ay, az = NT.case("twins", k)
    listed = _knn(ctx, "twins", k)
    assert _compare(ctx, listed, "twins", k, what=" listed rerun") > 0
    whole = _knn(ctx, "twins", k, flags=_lib.FLAG_KNN_REPAIR_ALL)
    assert _compare(ctx, whole, "twins", k, what=" whole-launch rerun") > 1
    for a, b in zip(listed, whole):
        assert np.array_equal(a, b)
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    pl = ctx.interp_knn(P, Q, grid_points=(X, Y, Z), shape=X.shape, k=k)
    _compare(ctx, pl, "twins", k, what=" point list")
    mask = np.random.default_rng(7).uniform(size=X.shape) < 0.6
    mk = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)
    rep = ctx.stats["n_repair_tiles"]
    keep = NT.keep("twins", k) & mask
    print(f"twins k={k} fluid mask: fluid {mask.mean():.2%}, n_repair_tiles {rep}")
    assert rep > 0
    for a, b in zip(mk, NT.oracle_knn("twins", k)):
        assert np.array_equal(a[keep], b[keep]) and (a[~mask] == 0).all()
    for z0, z1 in ((0, 2), (2, len(az))):
        _compare(ctx, _knn(ctx, "twins", k, z_range=(z0, z1)), "twins", k, what=f" planes {z0}:{z1}", planes=slice(z0, z1))


# ---------------------------------------------------------------------------------------------
# outlier filter: k + 1 listed entries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", NT.K_FILTER)
def test_filter_twins(ctx, k):
    """keep and the per-particle (k+1)-th distance equal the brute-force restatement of the reference's
    filter.  The list holds the particle itself and k neighbours: for even k it ends inside a pair of
    twins (k = 12: a 13-entry key list, 24: 25 entries, 63 + 1: the 64-slot list).  Left out: the
    particles whose (k+1)-th and (k+2)-th d2 tie exactly."""
    P, Q, *_ = NT.case("twins")
    keep, kth = ctx.filter_outliers_knn(P, Q, k=k, threshold=3.0)
    rep = ctx.stats["n_repair_tiles"]
    ref_keep, _ = cpu_ref.outlier_filter(P, Q, k, 3.0, knn="bruteforce")
    ref_kth = np.sqrt(NT.filter_lists("twins")[0][:, k])
    ok = ~NT.filter_ties("twins", k)
    bad = int(np.sum(keep.view(bool)[ok] != ref_keep[ok]))
    print(f"filter twins k={k}: excluded {1.0 - ok.mean():.2%}, n_repair_tiles {rep}, rejected {np.mean(~ref_keep):.2%}, "
          f"decisions differing {bad}, k-th distances differing {int(np.sum(kth[ok] != ref_kth[ok]))}")
    assert bad == 0
    assert np.array_equal(kth[ok], ref_kth[ok])
    assert ok.mean() >= KEPT_MIN
    if k % 2 == 0:
        assert rep > 0


# ---------------------------------------------------------------------------------------------
# local RBF: neighbour sets through the slot lists
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", NT.K_RBF)
def test_rbf_mirror(ctx, k):
    """Thin-plate spline on ``mirror``: an odd k ends inside a mirror pair at most voxels, and the wrong
    one of the pair is another system.  Bar per component as tests/test_gpu_geometry.py:
    gpu-vs-exact <= max(1e-10, lapack-vs-exact), neighbour sets from the brute-force order."""
    from ptv_interpolation_amd.rbf import LocalRBFInterpolator

    P, Q, ax, ay, az = NT.case("mirror")
    U, V, W = LocalRBFInterpolator(P, Q, neighbors=k, kernel="thin_plate_spline").evaluate_grid(ax, ay, az, ctx=ctx)
    ok = ~NT.rbf_ties("mirror", k)
    lap, ext = NT.oracle_rbf("mirror", k, "lapack"), NT.oracle_rbf("mirror", k, "extended")
    inl, bnd = NT.near_tie_shares("mirror", k)
    print(f"mirror TPS k={k}: excluded {1.0 - ok.mean():.2%}, near tie in list {inl:.2%}, at boundary {bnd:.2%}")
    for c, a in enumerate((U, V, W)):
        e_exact = normwise(a.ravel()[ok], ext[ok, c])
        gap = normwise(lap[ok, c], ext[ok, c])
        print(f"mirror TPS k={k} {'UVW'[c]}: gpu-vs-lapack {normwise(a.ravel()[ok], lap[ok, c]):.3e}  "
              f"gpu-vs-exact {e_exact:.3e}  lapack-vs-exact {gap:.3e}")
        assert e_exact <= max(TOL_RBF, gap)
    assert ok.mean() >= KEPT_MIN


# ---------------------------------------------------------------------------------------------
# metamorphic: the particle order (no oracle)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", NT.K_PERMUTED)
def test_particle_order_changes_no_bit(ctx, k):
    """Permuting the particles changes every slot and with it the low bits of every key, so every pair
    of one truncation may swap; no output bit may change outside the exact ties on differing values."""
    P, Q, ax, ay, az = NT.case("twins", k)
    perm = np.random.default_rng(99).permutation(len(P))
    a3 = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k)
    b3 = ctx.interp_knn(P[perm].copy(), Q[perm].copy(), axes=(ax, ay, az), k=k)
    keep = NT.keep("twins", k)
    diff = [int(np.sum(a[keep] != b[keep])) for a, b in zip(a3, b3)]
    print(f"twins k={k} permuted: excluded {1.0 - keep.mean():.2%}, differing voxels {diff} of {keep.sum()}")
    assert diff == [0, 0, 0] and keep.mean() >= KEPT_MIN
