"""Fill-then-sort pair lists (k <= 12): the first KMAX merges of a tile write list positions
0 .. KMAX-1 and one stable sorting network orders them; later merges use the insertion sweep.

Every case is bit for bit against ``oracle.cpu_ref`` (IDW p = 2: IEEE-exact operations only), on
every voxel: the inputs have n >= k, so the reference defines all of them (asserted).  Grid
24 x 20 x 12: no multiple of the 4^3 tile, so padded lanes and the partial x-tile are exercised.
Runs only on an MI355X (``-m gpu``).

What this file does NOT cover: the ORDER of equal-d2 entries (the stability of ``sort_pairs``).
The oracle's cKDTree orders equidistant neighbours by its own traversal, so no reference tells
which of two tied particles with different values comes first; the lattice case therefore gives
every particle the same value, which checks the distance multiset, lost or duplicated entries
and the k-th boundary, but would also pass with an unstable network.  Stability rests on the
argument in the ``sort_pairs`` comment (adjacent comparators, strict ``<``) and on a one-off
comparison of this build with the insertion-only parent build on a value-heterogeneous lattice
(``profiles/r07_ab/tie_order_parent_vs_new.txt``).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AX, AY, AZ = np.arange(24.0), np.arange(20.0), np.arange(12.0)
HI = np.array([23.0, 19.0, 11.0])
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _random(n=1500, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, 3)) * HI, rng.standard_normal((n, 3))


def _corner(n=40):
    rng = np.random.default_rng(11)
    return rng.uniform(0.0, 3.0, (n, 3)), rng.standard_normal((n, 3))


def _clump():
    """The random set plus ~300 particles inside a ball of radius 0.7 in the middle of one tile."""
    P, Q = _random()
    rng = np.random.default_rng(13)
    e = rng.standard_normal((300, 3))
    e *= (0.7 * rng.uniform(0.0, 1.0, (300, 1)) ** (1.0 / 3.0)) / np.linalg.norm(e, axis=1, keepdims=True)
    return np.concatenate([P, np.array([9.5, 9.5, 5.5]) + e]), np.concatenate([Q, rng.standard_normal((300, 3))])


def _lattice():
    """Particles on the integer lattice covering the grid, one value per component: every distance
    boundary is an exact tie and every tie value-homogeneous (the result is the same in any tie
    order; a wrong distance multiset or a lost entry is not)."""
    Z, Y, X = np.meshgrid(np.arange(13.0), np.arange(21.0), np.arange(25.0), indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)
    return P, np.tile([1.5, -2.0, 0.25], (len(P), 1))


SETS = {"random": _random, "corner": _corner, "clump": _clump, "lattice": _lattice,
        "n8": lambda: _random(8, 3)}


def _ref(name, k, off=0.0):
    """Oracle outputs of a case, computed once and shared (read-only)."""
    from oracle import cpu_ref

    key = (name, k, off)
    if key not in _REF:
        P, Q = SETS[name]()
        ref = cpu_ref.interp_grid(P, Q, AX + off, AY + off, AZ + off, "idw", k, 2.0)
        for r in ref:
            assert np.isfinite(r).all()  # the reference defines every voxel: none is left out
            r.setflags(write=False)
        _REF[key] = (P, Q, ref)
    return _REF[key]


def _check(ctx, name, k, off=0.0, **kw):
    P, Q, ref = _ref(name, k, off)
    out = ctx.interp_knn(P, Q, axes=(AX + off, AY + off, AZ + off), k=k, power=2.0, **kw)
    for c, (a, b) in enumerate(zip(out, ref)):
        bad = int(np.sum(a != b))
        print(f"{name} k={k} off={off} {'UVW'[c]}: {bad} of {a.size} voxels differ")
        assert np.array_equal(a, b), f"{bad} voxels differ"
    return out


@pytest.mark.parametrize("k", [4, 8, 12])
def test_fill_path_k_equals_kmax(ctx, k):
    _check(ctx, "random", k)


@pytest.mark.parametrize("k", [5, 7, 11])
def test_insert_path_k_below_kmax(ctx, k):
    """k < KMAX: front sentinels, the fill is off and the insertion sweep builds the whole list."""
    _check(ctx, "random", k)


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("off", [0.0, 0.5])
def test_particle_lattice_ties(ctx, k, off):
    """Voxels on the particle lattice (off = 0) and at its cell centres (off = 0.5): exact d2 ties
    among the first KMAX candidates of every voxel."""
    _check(ctx, "lattice", k, off)


def test_sparse_exactly_k_particles(ctx):
    """n = k = 8: every list is exactly full from the fill alone."""
    _check(ctx, "n8", 8)


def _stamped(ctx, name, k=8):
    """The case again through the stamped k = 8 kernel: per-wave counters of the search (the
    largest over the waves), outputs still bit-exact."""
    ctx.debug_stamps(1)
    try:
        _check(ctx, name, k)
        c = ctx.debug_stamps(2)
    finally:
        ctx.debug_stamps(0)
    print(f"{name} k={k}: waves {c['waves']:.0f}, max per wave {c['max']}")
    assert c["waves"] > 0
    return c["max"]


def test_sparse_corner_cluster(ctx):
    """40 particles in one corner: far tiles grow their radius over several passes, so a partly
    filled list is sorted before each radius decision (asserted: some wave ran more than one
    pass)."""
    _check(ctx, "corner", 8)
    assert _stamped(ctx, "corner")["passes"] > 1


@pytest.mark.parametrize("k", [4, 8, 12])
def test_dense_clump_many_groups(ctx, k):
    """More than 64 kept candidates in one tile: the fill ends inside the first group and the
    insertion sweep goes on across groups and flushes."""
    _check(ctx, "clump", k)
    if k == 8:  # the stamped kernel exists for 8 slots: some wave kept > 64 candidates and merged > 8
        mx = _stamped(ctx, "clump")
        assert mx["kept"] > 64 and mx["merges"] > 8


def test_fluid_mask_k8(ctx):
    """Masked-out voxels are inactive lanes: their -1 entries go through the sort untouched."""
    from ptv_interpolation_amd import _lib

    P, Q, ref = _ref("random", 8)
    mask = np.random.default_rng(2).uniform(size=(12, 20, 24)) < 0.6
    out = ctx.interp_knn(P, Q, axes=(AX, AY, AZ), k=8, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)
    for a, b in zip(out, ref):
        assert np.array_equal(a[mask], b[mask]) and (a[~mask] == 0).all()


@pytest.mark.parametrize("k", [3, 7, 11])
def test_outlier_filter_full_lists(ctx, k):
    """The outlier filter searches k + 1 neighbours (the particle itself included): k + 1 = 4, 8
    and 12 are pair lists without front sentinels, so the filter's instantiation takes the fill."""
    from oracle import cpu_ref

    rng = np.random.default_rng(k)
    P = rng.uniform(0.0, 1.0, (5000, 3)) * HI
    Q = rng.standard_normal((len(P), 3))
    Q[rng.choice(len(P), 50, replace=False)] *= 8.0
    keep, kth = ctx.filter_outliers_knn(P, Q, k=k, threshold=3.0)
    exp, radius = cpu_ref.outlier_filter(P, Q, k, 3.0)
    assert np.array_equal(keep.view(bool), exp)
    assert np.median(kth) == radius


def test_nearest_untouched(ctx):
    """method='nearest' (KMAX = 1) takes no part in the fill."""
    from oracle import cpu_ref
    from ptv_interpolation_amd import _lib

    P, Q = _random()
    out = ctx.interp_knn(P, Q, axes=(AX, AY, AZ), method=_lib.METHOD_NEAREST, k=1)
    ref = cpu_ref.interp_grid(P, Q, AX, AY, AZ, "nearest")
    for a, b in zip(out, ref):
        assert np.isfinite(b).all() and np.array_equal(a, b)


@pytest.mark.parametrize("k", [4, 8])
def test_lattice_level_k_distance(ctx, k):
    """The k-distance lattice level (the same pair list, kModeKDist): a z-slab call with the
    per-column cull map runs an exact k-th distance level over the slab, whose bounds and seed
    records steer the main launch and the cull.  A cold call (map built) and a warm one (culled,
    proven on the device) equal the oracle on the slab; a k-th distance that came out too small
    would cut neighbours off or fail the proof."""
    from oracle import cpu_ref
    from ptv_interpolation_amd import _lib, synth

    G, z0, z1 = 64, 16, 32
    P, Q = synth.sphere_pack(40000, G, values="normal")
    ax = np.linspace(0, G - 1, G)
    ref = cpu_ref.interp_grid(P, Q, ax, ax, ax, "idw", k, 2.0, z0=z0, z1=z1)
    for r in ref:
        assert np.isfinite(r).all()
    c = _lib.Context(0)
    try:
        for call in range(2):
            out = c.interp_knn(P, Q, axes=(ax, ax, ax), k=k, z_range=(z0, z1), flags=_lib.FLAG_SLAB_CULL_AUTO)
            st = c.stats
            print(f"lattice level k={k} call {call}: binned {st['n_binned']} of {len(P)}, "
                  f"lattice {st['ms_lattice']:.3f} ms")
            assert st["ms_lattice"] > 0.0
            for a, b in zip(out, ref):
                assert np.array_equal(a, b), f"call {call}: {np.sum(a != b)} voxels differ"
        assert st["n_binned"] < len(P)  # the warm call culled
    finally:
        c.close()
