"""The k-NN search kernel's prefilter bit masks, sub-ball copy filter and row setup.

The prefilter builds each lane's candidate mask by a compare into the carry register and an
add-with-carry, in two 32-bit halves per group of 64 candidates; the copy window tests a
candidate against the eight sub-balls with packed arithmetic and scalar lane masks; the row
setup skips the previous pass's chord on a scalar branch.  None of this may change a list.

Every case is bit for bit against ``oracle.cpu_ref`` (IDW p = 2: IEEE-exact operations only),
U, V and W by ``array_equal``.  Particle coordinates come from seeded continuous distributions,
and each case first asserts on the CPU that the oracle's k-th and (k+1)-th distances differ at
every voxel: no ties, so one answer exists and no voxel is left out.  Runs only on an MI355X
(``-m gpu``).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _axes(shape, perturb_seed=None):
    """Unit-spaced axes of an (nx, ny, nz) grid, or a seeded monotone perturbation of them (each
    value moved by less than 0.3 of the spacing, the end points kept)."""
    axes = [np.arange(float(n)) for n in shape]
    if perturb_seed is not None:
        rng = np.random.default_rng(perturb_seed)
        for a in axes:
            a[1:-1] += rng.uniform(-0.3, 0.3, len(a) - 2)
            assert (np.diff(a) > 0).all()
    return axes


def _blob(n, seed, centre=(3.3, 4.1, 3.7), width=4.0):
    """n particles in a cube about one tile (4 voxels) wide inside the 8^3 grid."""
    rng = np.random.default_rng(seed)
    return np.asarray(centre) + rng.uniform(-0.5 * width, 0.5 * width, (n, 3)), rng.standard_normal((n, 3))


def _ref(key, make, axes, k):
    """Oracle outputs of a case, computed once and shared (read-only), after the no-tie check."""
    from oracle import cpu_ref

    key = key + (k,)
    if key not in _REF:
        P, Q = make()
        ax, ay, az = axes
        if len(P) > k:
            d, _ = cpu_ref.knn_kdtree(P, cpu_ref.grid_queries(ax, ay, az), k + 1)
            gap = d[:, k] - d[:, k - 1]
            assert (gap > 0).all(), f"{int((gap <= 0).sum())} voxels with a tie at the k-th distance"
        # k = 1 is the one-slot list of method 'nearest' (the oracle's IDW needs k >= 2)
        ref = cpu_ref.interp_grid(P, Q, ax, ay, az, "nearest" if k == 1 else "idw", k, 2.0)
        for r in ref:
            assert np.isfinite(r).all()  # the reference defines every voxel
            r.setflags(write=False)
        _REF[key] = (P, Q, ref)
    return _REF[key]


def _check(ctx, key, make, axes, k, mask=None, **kw):
    from ptv_interpolation_amd import _lib

    P, Q, ref = _ref(key, make, axes, k)
    if k == 1:
        kw["method"] = _lib.METHOD_NEAREST
    out = ctx.interp_knn(P, Q, axes=tuple(axes), k=k, power=2.0, **kw)
    for c, (a, b) in enumerate(zip(out, ref)):
        if mask is not None:
            assert (a[~mask] == 0).all()
            a, b = a[mask], b[mask]
        bad = int(np.sum(a != b))
        print(f"{key} k={k} {'UVW'[c]}: {bad} of {a.size} voxels differ")
        assert np.array_equal(a, b), f"{bad} voxels differ"


# ---- group-size sweep: with so few particles every one reaches every tile's buffer, so a flush
#      group holds n candidates: both sides of the multiples of 4 (stale-slot clearing), of 32 (the
#      two mask halves) and of 64 (a second group in one flush), and past the buffer's capacity
#      (a flush in the middle of the gather)
@pytest.mark.parametrize("n", [8, 9, 11, 12, 13, 31, 32, 33, 35, 63, 64, 65, 67, 100, 130])
def test_group_sizes_k8(ctx, n):
    _check(ctx, ("blob", n), lambda: _blob(n, 100 + n), _axes((8, 8, 8)), 8)


@pytest.mark.parametrize("k", [1, 4, 5, 8, 12, 20])
def test_every_list_form_n40(ctx, k):
    """One-slot, pair lists with and without front sentinels, and a key list: all share `flush`."""
    _check(ctx, ("blob", 40), lambda: _blob(40, 140), _axes((8, 8, 8)), k)


# ---- ragged and masked: 21 x 18 x 13 has padding lanes in all three axes
def _pack():
    from ptv_interpolation_amd import synth

    return synth.sphere_pack(3000, (21, 18, 13), values="normal")


@pytest.mark.parametrize("k", [8, 4])
@pytest.mark.parametrize("perturbed", [False, True], ids=["uniform", "nonuniform"])
def test_ragged_masked(ctx, k, perturbed):
    """Sphere-pack particles with the fluid mask and nan_to_num.  Non-uniform axes: the tile box
    and the sub-box extents differ from tile to tile."""
    from ptv_interpolation_amd import _lib, synth

    mask = synth.fluid_mask((21, 18, 13))
    assert mask.any() and not mask.all()
    axes = _axes((21, 18, 13), 5 if perturbed else None)
    _check(ctx, ("pack", perturbed), _pack, axes, k, mask=mask, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)


# ---- void tile: far tiles take several passes and rounds (Rp >= 0: the previous-pass branch)
def _octant():
    rng = np.random.default_rng(21)
    return rng.uniform(0.0, 7.0, (300, 3)), rng.standard_normal((300, 3))


def test_void_tiles_several_passes(ctx):
    axes = _axes((16, 16, 16))
    _check(ctx, ("octant",), _octant, axes, 8)
    ctx.debug_stamps(1)
    try:
        _check(ctx, ("octant",), _octant, axes, 8)
        c = ctx.debug_stamps(2)
    finally:
        ctx.debug_stamps(0)
    print(f"octant: waves {c['waves']:.0f}, max per wave {c['max']}")
    assert c["max"]["passes"] > 1 and c["max"]["rounds"] > 1


# ---- lattice mode: 64^3 is large enough for lattice levels (more than 50000 points), so the
#      k-distance instantiation and its tightening path run the same group masks
def _pack64():
    from ptv_interpolation_amd import synth

    return synth.sphere_pack(20000, 64, values="normal")


def test_lattice_levels_64(ctx):
    ax = np.linspace(0, 63, 64)
    _check(ctx, ("pack64",), _pack64, (ax, ax, ax), 8)
    assert ctx.stats["ms_lattice"] > 0.0
