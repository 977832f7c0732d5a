"""The once-per-tile phases of the k <= 8 search kernel: the IDW epilogue and what feeds it.

A full eight-slot list with p = 2 or 1 takes one range test for its eight square roots and
in-range reciprocals instead of the full division sequence, without the j < k selects; any lane out
of range leaves the wave on the general form.  The pass-end and first-radius wave reductions decide
which lists reach the epilogue.  None of this may change an output bit.

IDW with p = 2 and p = 1 uses IEEE-exact operations only and is held bit for bit against
``oracle.cpu_ref``, U, V and W by ``array_equal``.  p = 3 and Sibson go through ``pow`` / ``exp``,
which neither numpy nor the device rounds correctly, so bit equality with the oracle does not hold
for them before this change either: on the MI355X the commit before it differs from the oracle in
176, 186 and 190 of 512 voxels (U, V, W) at p = 3 and in 70, 67 and 67 for Sibson, and this build in the
same numbers, with byte-identical outputs (profiles/r11_tile_phases/epilogue_cases_sha256.txt).
Those two cases are held to the project's normwise bar for them (1e-10,
``tests/test_gpu_keylist_epilogue.py``) and must be finite.  Particle coordinates come from seeded
continuous distributions, and each case first asserts on the CPU that the oracle's k-th and
(k+1)-th distances differ at every voxel: no ties, so one answer exists and no voxel is left out.
Runs only on an MI355X (``-m gpu``).
"""
import numpy as np
import pytest

from tests._util import normwise

pytestmark = pytest.mark.gpu

TOL_LIBM = 1e-10  # p = 3 and Sibson (pow, exp), as tests/test_gpu_keylist_epilogue.py
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _axes(shape, perturb_seed=None, scale=1.0):
    """Unit-spaced axes of an (nx, ny, nz) grid times `scale`, or a seeded monotone perturbation
    of them (each value moved by less than 0.3 of the spacing, the end points kept)."""
    axes = [np.arange(float(n)) for n in shape]
    if perturb_seed is not None:
        rng = np.random.default_rng(perturb_seed)
        for a in axes:
            a[1:-1] += rng.uniform(-0.3, 0.3, len(a) - 2)
            assert (np.diff(a) > 0).all()
    return [a * scale for a in axes]


def _ref(key, make, axes, k, method="idw", power=2.0):
    """Oracle outputs of a case, computed once and shared (read-only), after the no-tie check."""
    from oracle import cpu_ref

    key = key + (k, method, power)
    if key not in _REF:
        P, Q = make()
        ax, ay, az = axes
        assert len(P) > k
        d, _ = cpu_ref.knn_kdtree(P, cpu_ref.grid_queries(ax, ay, az), k + 1)
        gap = d[:, k] - d[:, k - 1]
        assert (gap > 0).all(), f"{int((gap <= 0).sum())} voxels with a tie at the k-th distance"
        ref = cpu_ref.interp_grid(P, Q, ax, ay, az, method, k, power)
        for r in ref:
            assert np.isfinite(r).all()  # the reference defines every voxel
            r.setflags(write=False)
        _REF[key] = (P, Q, ref)
    return _REF[key]


def _check(ctx, key, make, axes, k, method="idw", power=2.0, mask=None, f32=False, bits=True, **kw):
    from ptv_interpolation_amd import _lib

    P, Q, ref = _ref(key, make, axes, k, method, power)
    m = _lib.METHOD_SIBSON if method == "sibson" else _lib.METHOD_IDW
    out = ctx.interp_knn(P, Q, axes=tuple(axes), k=k, power=power, method=m, **kw)
    for c, (a, b) in enumerate(zip(out, ref)):
        if f32:
            assert a.dtype == np.float32
            b = b.astype(np.float32)  # numpy astype: round to nearest even
        if mask is not None:
            assert (a[~mask] == 0).all()
            a, b = a[mask], b[mask]
        assert np.isfinite(a).all()
        bad = int(np.sum(a != b))
        print(f"{key} k={k} {method} p={power} {'UVW'[c]}: {bad} of {a.size} voxels differ, normwise {normwise(a, b):.2e}")
        if bits:
            assert np.array_equal(a, b), f"{bad} voxels differ"
        else:
            assert normwise(a, b) <= TOL_LIBM


# ---- lattice levels (more than 50 000 grid points): the first radius is the wave's largest
#      lattice bound
def _uniform(shape, n=20000, seed=3):
    def make():
        rng = np.random.default_rng(seed)
        return rng.uniform(0.0, 1.0, (n, 3)) * (np.asarray(shape) - 1.0), rng.standard_normal((n, 3))

    return make


@pytest.mark.parametrize("k", [8, 4, 5])
@pytest.mark.parametrize("shape", [(40, 40, 40), (38, 37, 41)], ids=["40", "ragged"])
def test_lattice_grids(ctx, shape, k):
    """k = 8 fills the list (the k == KMAX epilogue); 4 has its own kernel; 5 has front sentinels."""
    _check(ctx, ("uniform", shape), _uniform(shape), _axes(shape), k)
    assert ctx.stats["ms_lattice"] > 0.0


def test_lattice_grid_nonuniform_axes(ctx):
    shape = (40, 40, 40)
    _check(ctx, ("uniform-perturbed", shape), _uniform(shape), _axes(shape, perturb_seed=9), 8)
    assert ctx.stats["ms_lattice"] > 0.0


# ---- the reduction's deciding lane: a blob in one corner of the 8^3 grid, so that the largest k-th
#      distance of a tile sits at its far corner; mirrored into all eight corners, the deciding lane
#      is in every DPP row and at lanes 0 and 63
def _corner_blob(corner, n=40):
    def make():
        rng = np.random.default_rng(50)
        P = rng.uniform(0.2, 2.2, (n, 3))
        for a in range(3):
            if (corner >> a) & 1:
                P[:, a] = 7.0 - P[:, a]
        return P, rng.standard_normal((n, 3))

    return make


@pytest.mark.parametrize("corner", range(8))
def test_deciding_lane_every_corner(ctx, corner):
    _check(ctx, ("corner", corner), _corner_blob(corner), _axes((8, 8, 8)), 8)


# ---- void tiles whose lists are not full after a pass (an infinite k-th distance) and take
#      several passes
def _corner_cube():
    rng = np.random.default_rng(23)
    return rng.uniform(0.0, 5.0, (300, 3)), rng.standard_normal((300, 3))


def test_void_tiles_several_passes(ctx):
    axes = _axes((12, 12, 12))
    _check(ctx, ("cube",), _corner_cube, axes, 8)
    ctx.debug_stamps(1)
    try:
        _check(ctx, ("cube",), _corner_cube, axes, 8)
        c = ctx.debug_stamps(2)
    finally:
        ctx.debug_stamps(0)
    print(f"corner cube: waves {c['waves']:.0f}, max per wave {c['max']}")
    assert c["max"]["passes"] > 1


# ---- epilogue guards
def _blob(n=60, seed=77, on_voxel=False, scale=1.0):
    def make():
        rng = np.random.default_rng(seed)
        P = np.asarray((3.3, 4.1, 3.7)) + rng.uniform(-3.0, 3.0, (n, 3))
        if on_voxel:
            P[0] = (3.0, 4.0, 3.0)  # d2 = 0 there: the square root's fallback, weight 1 / eps
        return P * scale, rng.standard_normal((n, 3))

    return make


def test_particle_on_a_voxel(ctx):
    _check(ctx, ("blob-on-voxel",), _blob(on_voxel=True), _axes((8, 8, 8)), 8)


@pytest.mark.parametrize("scale", [1e-150, 1e149], ids=["1e-150", "1e149"])
def test_scaled_grid_leaves_the_division_range(ctx, scale):
    """d2 of about 1e-300 (below the square root's range) and 1e298 (above the epilogue's 2^490).
    The large scale is 1e149, not 1e150: the grid reaches 7 units, and prepare() refuses
    coordinates beyond 2^500 = 3.3e150.  At 1e149 the tile-relative coordinates leave fp32, so the
    case also holds the search's fp32 filters to switching themselves off there (`wide` tiles)."""
    _check(ctx, ("blob-scaled", scale), _blob(scale=scale), _axes((8, 8, 8), scale=scale), 8)


def test_power_one(ctx):
    _check(ctx, ("blob",), _blob(), _axes((8, 8, 8)), 8, power=1.0)


def test_power_three(ctx):
    _check(ctx, ("blob",), _blob(), _axes((8, 8, 8)), 8, power=3.0, bits=False)


def test_sibson_k8(ctx):
    _check(ctx, ("blob",), _blob(), _axes((8, 8, 8)), 8, method="sibson", bits=False)


def test_masked_f32_outputs(ctx):
    from ptv_interpolation_amd import _lib, synth

    shape = (21, 18, 13)
    mask = synth.fluid_mask(shape)
    assert mask.any() and not mask.all()
    make = lambda: synth.sphere_pack(3000, shape, values="normal")  # noqa: E731
    _check(ctx, ("pack",), make, _axes(shape), 8, mask=mask, f32=True, fluid_mask=mask,
           flags=_lib.FLAG_NAN_TO_NUM | _lib.FLAG_OUT_F32)
