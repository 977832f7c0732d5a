"""The map that deals the blocks of a k-NN launch to the XCDs (csrc/ptv_xcd_map.hpp).

A launch without a dispatch order runs block ``xcd_chunk_block(lb, nb, C)`` in dispatch slot ``lb``:
chunks of C consecutive blocks dealt round-robin to the eight XCDs, one contiguous range per XCD
for what is left after the whole rounds (and for the whole grid when it has fewer than 16 chunks).
A map that is no bijection leaves tiles unwritten and writes others twice over; outputs must not
depend on C at all.  The host test reads the map through ``ptv_xcd_chunk_map`` (the same function
the kernel calls); the GPU tests set C to 1, 3 and 5 blocks (``ptv_debug_xcd_chunk``: the shipped
library reads no environment), so that small grids cross many chunk boundaries, and hold U, V and W
to ``oracle.cpu_ref`` bit for bit for IDW k = 8, k = 4 and ``nearest``.  Particle coordinates come
from seeded continuous distributions, and each reference first asserts that the oracle's k-th and
(k+1)-th distances differ at every voxel, so one answer exists.
"""
import numpy as np
import pytest

_REF = {}
CHUNKS = [1, 3, 5]
METHODS = [("idw", 8), ("idw", 4), ("nearest", 1)]


@pytest.mark.parametrize("C", [1, 3, 8, 64, 5000])
@pytest.mark.parametrize("nb", [1, 7, 8, 9, 63, 64, 65, 1000, 4097])
def test_map_is_a_permutation_with_consecutive_runs(nb, C):
    from ptv_interpolation_amd import _lib

    m = _lib.xcd_chunk_map(nb, C).astype(np.int64)
    assert np.array_equal(np.sort(m), np.arange(nb)), "not a permutation of [0, nb)"
    for x in range(8):
        s = m[x::8]  # XCD x's dispatch slots in order
        for j in range(0, len(s), C):
            run = s[j:j + C]
            assert np.array_equal(run, run[0] + np.arange(len(run))), (x, j, run)
    if nb >= 16 * C:  # interleaved: XCD x's first chunk is chunk x
        for x in range(8):
            assert m[x] == x * C
    else:  # today's contiguous ranges
        q, r = divmod(nb, 8)
        start = 0
        for x in range(8):
            n = q + (x < r)
            assert np.array_equal(m[x::8], start + np.arange(n))
            start += n


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _axes(shape):
    return [np.arange(float(n)) for n in shape]


def _pack():
    from ptv_interpolation_amd import synth

    return synth.sphere_pack(3000, (52, 20, 36), values="normal")


def _half():
    """Every particle in z < 17: the upper tiles are void and take several passes."""
    rng = np.random.default_rng(41)
    return rng.uniform(0.0, 1.0, (3000, 3)) * (51.0, 19.0, 17.0), rng.standard_normal((3000, 3))


def _small():
    rng = np.random.default_rng(43)
    return rng.uniform(0.0, 1.0, (300, 3)) * (11.0, 7.0, 7.0), rng.standard_normal((300, 3))


# grid 52 x 20 x 36: 13 x-tiles in 4 blocks, 5 y-tiles, 9 z-tiles = 180 blocks, no multiple of 8
CASES = {"pack": (_pack, (52, 20, 36)), "half": (_half, (52, 20, 36)), "small": (_small, (12, 8, 8))}


def _ref(name, method, k, z0=0, z1=None):
    """Oracle outputs of a named case, computed once and shared (read-only)."""
    key = (name, method, k, z0, z1)
    if key not in _REF:
        from oracle import cpu_ref

        make, shape = CASES[name]
        P, Q = make()
        ax, ay, az = _axes(shape)
        d, _ = cpu_ref.knn_kdtree(P, cpu_ref.grid_queries(ax, ay, az, z0, z1), k + 1)
        assert (d[:, k] - d[:, k - 1] > 0).all(), "a tie at the k-th distance"
        ref = cpu_ref.interp_grid(P, Q, ax, ay, az, method, k, 2.0, z0, z1)
        for r in ref:
            assert np.isfinite(r).all()
            r.setflags(write=False)
        _REF[key] = (P, Q, (ax, ay, az), ref)
    return _REF[key]


def _compare(out, ref, label, mask=None):
    for c, (a, b) in enumerate(zip(out, ref)):
        if mask is not None:
            assert (a[~mask] == 0).all()
            a, b = a[mask], b[mask]
        bad = int(np.sum(a != b))
        print(f"{label} {'UVW'[c]}: {bad} of {a.size} voxels differ")
        assert np.array_equal(a, b), f"{bad} voxels differ"


def _check(ctx, name, C, z_range=None, mask=None, **kw):
    from ptv_interpolation_amd import _lib

    _lib.debug_xcd_chunk(C)
    try:
        for method, k in METHODS:
            z0, z1 = z_range if z_range else (0, None)
            P, Q, axes, ref = _ref(name, method, k, z0, z1)
            m = _lib.METHOD_NEAREST if method == "nearest" else _lib.METHOD_IDW
            out = ctx.interp_knn(P, Q, axes=axes, method=m, k=k, z_range=z_range, **kw)
            _compare(out, ref, f"{name} C={C} {method} k={k}", mask)
    finally:
        _lib.debug_xcd_chunk(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_ragged_block_count(ctx, C):
    _check(ctx, "pack", C)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_fewer_than_eight_blocks(ctx, C):
    _check(ctx, "small", C)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_z_range_slab(ctx, C):
    _check(ctx, "pack", C, z_range=(6, 29))


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_fluid_mask_nan_to_num(ctx, C):
    from ptv_interpolation_amd import _lib, synth

    mask = synth.fluid_mask((52, 20, 36))
    assert mask.any() and not mask.all()
    _check(ctx, "pack", C, mask=mask, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_empty_half_void_tiles_in_some_chunks(ctx, C):
    _check(ctx, "half", C)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHUNKS)
def test_k24_repair_launch_next_to_the_map(ctx, C):
    """Particles on an integer lattice with one value per component (tests/test_gpu_keys.py): ties
    at the list's boundary send tiles to the repair launch, which takes listed tiles, next to a main
    launch through the map (16 blocks: two rounds at C = 1, contiguous at 3 and 5); then the whole
    launch again with the exact lists (PTV_FLAG_KNN_REPAIR_ALL), through the map as well."""
    from oracle import cpu_ref
    from ptv_interpolation_amd import _lib

    g = np.arange(0.0, 14.0)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)
    Q = np.tile([1.5, -2.0, 0.25], (len(P), 1))
    ax = np.arange(0.5, 13.0, 1.0)
    if "k24" not in _REF:
        _REF["k24"] = cpu_ref.interp_grid(P, Q, ax, ax, ax, "idw", 24, 2.0)
    _lib.debug_xcd_chunk(C)
    try:
        listed = ctx.interp_knn(P, Q, axes=(ax, ax, ax), k=24)
        rep = ctx.stats["n_repair_tiles"]
        whole = ctx.interp_knn(P, Q, axes=(ax, ax, ax), k=24, flags=_lib.FLAG_KNN_REPAIR_ALL)
    finally:
        _lib.debug_xcd_chunk(-1)
    print(f"k=24 C={C}: repaired tiles {rep}")
    assert rep > 0  # the repair launch ran
    _compare(listed, _REF["k24"], f"k=24 C={C} listed")
    _compare(whole, _REF["k24"], f"k=24 C={C} whole")
