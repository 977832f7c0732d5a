"""The k <= 8 search kernel's lattice-corner seeds on the block shapes where they can
go wrong: blocks with 1, 2 or 3 live x-tiles (3, 2 or 1 waves without work), partial tiles on
every axis, clamped last lattice corners, all-solid tiles and blocks, z-slabs, every list length,
fewer distinct seeds than list slots (the sentinel-padded, store-then-sort seed network then keeps
+inf entries and the lattice bound takes over), exact ties, and a point list.  Each case is held
to the oracle with the bars of tests/test_gpu_parity.py: bit-exact for IDW p = 2 and for nearest.

The cases were written for block-staged seed records (one block barrier in a kernel with
wave-level exits: a wave that skips it hangs the kernel).  Staging measured slower and is not in
the library; the cases stay, since every one of them runs the seed network.

A grid gets a lattice (and with it seed records) only above 50000 points with every side >= 9
(csrc/ptv_search.cpp, lattice_level_above).  The small grids below (nx = 4, 8, 12 and 18 x 6 x 6)
therefore run the kernel without seeds; the `LATTICE` grids repeat their block shapes at the
smallest sizes that have seeds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nx, ny, nz) just above the lattice threshold: 17 -> 5 x-tiles (last block: 1 live tile, 3 waves
# without work), 21 -> 6 (2 live), 26 -> 7 (3 live); ny and nz are no multiples of 4 either, and
# the last lattice plane of each axis is the clamped one (n - 1 is no multiple of 4 in y and z)
LATTICE = [(17, 58, 54), (21, 50, 50), (26, 46, 42)]
SMALL = [(4, 10, 10), (8, 10, 10), (12, 10, 10), (18, 6, 6)]


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _axes(shape):
    nx, ny, nz = shape
    return np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64) * 1.25, np.arange(nz, dtype=np.float64) * 0.75


def _cloud(shape, n, seed=3):
    ax, ay, az = _axes(shape)
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.0, 1.0, (n, 3)) + rng.uniform(0, 1, (n, 3)) * [ax[-1], ay[-1], az[-1]]
    return P, rng.standard_normal((n, 3))


def _check(ctx, P, Q, axes, k, method="idw", z_range=None):
    from oracle import cpu_ref
    from ptv_interpolation_amd import _lib

    m = _lib.METHOD_NEAREST if method == "nearest" else _lib.METHOD_IDW
    got = ctx.interp_knn(P, Q, axes=axes, method=m, k=k, power=2.0, z_range=z_range)
    z0, z1 = (0, len(axes[2])) if z_range is None else z_range
    ref = cpu_ref.interp_grid(P, Q, *axes, method, k, 2.0, z0, z1)
    for name, a, b in zip("UVW", got, ref):
        assert a.shape == b.shape
        assert np.array_equal(a, b, equal_nan=True), f"{name}: {np.sum(a != b)} voxels differ"


@pytest.mark.parametrize("shape", SMALL + LATTICE, ids=lambda s: "x".join(map(str, s)))
def test_live_tiles_per_block(ctx, shape):
    """1, 2, 3 or 4 live x-tiles in a block, partial tiles, clamped last corners: IDW k = 8 and nearest."""
    P, Q = _cloud(shape, 4000)
    _check(ctx, P, Q, _axes(shape), 8)
    _check(ctx, P, Q, _axes(shape), 1, "nearest")


@pytest.mark.parametrize("k", [1, 3, 4, 8])
def test_list_lengths(ctx, k):
    """k = 1 (the one-slot list, as 'nearest': IDW needs k >= 2), 3 (a front sentinel in a 4-slot
    list), 4 and 8 on a grid with seeds."""
    shape = LATTICE[1]
    P, Q = _cloud(shape, 6000, seed=k)
    _check(ctx, P, Q, _axes(shape), k, "nearest" if k == 1 else "idw")


@pytest.mark.parametrize("n,k", [(5, 4), (5, 5), (20, 8)])
def test_fewer_seeds_than_slots(ctx, n, k):
    """Fewer particles than list slots around the corners: the 8 corners' lists are the same few
    particles, fewer than 8 distinct seeds survive, and lanes without a seed bound take the lattice's."""
    shape = LATTICE[0]
    P, Q = _cloud(shape, n, seed=n)
    _check(ctx, P, Q, _axes(shape), k)


def test_solid_tile_and_solid_block(ctx):
    """A fluid mask with exactly one wave's tile all solid, and one with a whole block all solid:
    waves without an active voxel run no seed network and write zeros."""
    from oracle import cpu_ref
    from ptv_interpolation_amd import _lib

    shape = (33, 42, 38)  # 9 x-tiles: 3 blocks in x
    nx, ny, nz = shape
    axes = _axes(shape)
    P, Q = _cloud(shape, 5000)
    ref = cpu_ref.interp_grid(P, Q, *axes, "idw", 8, 2.0)
    tile = np.ones((nz, ny, nx), bool)
    tile[12:16, 8:12, 4:8] = False      # tile (1, 2, 3): wave 1 of block (0, 2, 3)
    block = np.ones((nz, ny, nx), bool)
    block[16:20, 20:24, 16:32] = False  # block (1, 5, 4): all four waves
    for mask in (tile, block):
        got = ctx.interp_knn(P, Q, axes=axes, k=8, power=2.0, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)
        for a, b in zip(got, ref):
            assert np.array_equal(a[mask], b[mask]), f"{np.sum(a[mask] != b[mask])} fluid voxels differ"
            assert (a[~mask] == 0).all()


@pytest.mark.parametrize("z_range", [(4, 40), (12, 48)])
def test_z_slab(ctx, z_range):
    """A slab that starts on a tile boundary (a multiple of 4) that is no boundary of the whole
    grid's second lattice level (a multiple of 16): the slab's lattice starts at its own plane 0."""
    shape = (40, 40, 48)
    P, Q = _cloud(shape, 6000)
    _check(ctx, P, Q, _axes(shape), 8, z_range=z_range)


def test_particle_lattice_on_the_grid(ctx):
    """Particles on the voxels themselves (exact distance ties everywhere), one value per
    component, so every tie order gives the same result."""
    g = np.arange(0.0, 40.0)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)
    Q = np.tile([1.5, -2.0, 0.25], (len(P), 1))
    ax = np.arange(0.0, 38.0)
    _check(ctx, P, Q, (ax, ax, ax), 8)
    _check(ctx, P, Q, (ax, ax, ax), 4)


def test_point_list(ctx):
    """A non-separable call (a 200-point list): no lattice, no seeds."""
    from oracle import cpu_ref

    rng = np.random.default_rng(11)
    P = rng.uniform(-10, 10, (3000, 3)); Q = rng.standard_normal((3000, 3))
    pts = rng.uniform(-9, 9, (200, 3))
    X, Y, Z = (np.ascontiguousarray(pts[:, i]).reshape(1, 1, 200) for i in range(3))
    for k in (8, 4):
        U, V, W = ctx.interp_knn(P, Q, grid_points=(X, Y, Z), shape=X.shape, k=k)
        ref = cpu_ref.interp_points(P, Q, pts, "idw", k, 2.0)
        for a, b in zip((U, V, W), ref.T):
            assert np.array_equal(a.ravel(), b)
