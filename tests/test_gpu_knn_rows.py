"""The row phase of the k <= 8 search kernel: cell rows of a gather shell -> x-runs of cells.

Each lane of a wave takes one cell row of the shell, finds its chord of the gather ball, takes off
what the previous pass gathered, and clips the runs to the union of the eight sub-balls' chords of
that row.  The row index comes from a reciprocal multiply, the sub-ball chords from one fma each and
one interval per x-half.  A run that loses a needed cell loses a neighbour; a cell gathered twice
puts a particle into a list twice.  Either changes an output, so every case holds U, V and W to
``oracle.cpu_ref`` bit for bit (``array_equal``) on every voxel: IDW with p = 2 uses IEEE-exact
operations only.  Particle coordinates come from seeded continuous distributions, and each case
first asserts on the CPU that the oracle's k-th and (k+1)-th distances differ at every voxel: no
ties, so one answer exists and no voxel is left out.  Runs only on an MI355X (``-m gpu``).
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


def _axes(shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    return [o + h * np.arange(float(n)) for n, h, o in zip(shape, spacing, origin)]


def _reference(P, Q, axes, k):
    """Oracle outputs after the no-tie check (CPU only)."""
    from oracle import cpu_ref

    ax, ay, az = axes
    assert len(P) > k
    d, _ = cpu_ref.knn_kdtree(P, cpu_ref.grid_queries(ax, ay, az), k + 1)
    gap = d[:, k] - d[:, k - 1]
    assert (gap > 0).all(), f"{int((gap <= 0).sum())} voxels with a tie at the k-th distance"
    ref = cpu_ref.interp_grid(P, Q, ax, ay, az, "idw", k, 2.0)
    for r in ref:
        assert np.isfinite(r).all()  # the reference defines every voxel
        r.setflags(write=False)
    return ref


def _ref(name, k):
    """Reference of a named case, computed once and shared (read-only)."""
    if (name, k) not in _REF:
        make, axes = CASES[name]
        P, Q = make()
        _REF[(name, k)] = (P, Q, axes, _reference(P, Q, axes, k))
    return _REF[(name, k)]


def _compare(out, ref, label, mask=None):
    for c, (a, b) in enumerate(zip(out, ref)):
        if mask is not None:
            assert (a[~mask] == 0).all()
            a, b = a[mask], b[mask]
        assert np.isfinite(a).all()
        bad = int(np.sum(a != b))
        print(f"{label} {'UVW'[c]}: {bad} of {a.size} voxels differ")
        assert np.array_equal(a, b), f"{bad} voxels differ"


def _check(ctx, name, k, mask=None, **kw):
    P, Q, axes, ref = _ref(name, k)
    out = ctx.interp_knn(P, Q, axes=tuple(axes), k=k, **kw)
    _compare(out, ref, f"{name} k={k}", mask)


def _box(lo, hi, n, seed):
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)

    def make():
        rng = np.random.default_rng(seed)
        return lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo), rng.standard_normal((n, 3))

    return make


def _slab():
    """20 000 particles in a slab 0.2 thick: thousands of small cells in x and y, so a tile a few
    voxels off the slab sees more than 64 cell rows in its shell."""
    rng = np.random.default_rng(61)
    P = rng.uniform(0.0, 1.0, (20000, 3)) * (11.0, 11.0, 0.2) + (0.0, 0.0, 5.4)
    return P, rng.standard_normal((20000, 3))


_SP = (0.7, 1.3, 2.1)   # non-unit, unequal spacings
_OR = (1e6, -1e6, 1e6)  # far from 0: the cell edges relative to a tile are small differences of large numbers
CASES = {
    "uniform": (_box((0, 0, 0), (11, 11, 11), 300, 5), _axes((12, 12, 12))),
    "far-origin": (_box(_OR, np.add(_OR, np.multiply(_SP, 11.0)), 300, 6), _axes((12, 12, 12), _SP, _OR)),
    # particles well inside a ragged grid: the shells of the outer tiles overhang the cell grid on
    # every side, so the runs' ends clamp at cell 0 and at the last cell
    "overhang": (_box((3.2, 3.9, 2.7), (6.6, 7.3, 5.8), 300, 7), _axes((10, 11, 9))),
    # all particles in one corner: the far tiles' lists are not full after a pass, and the next pass
    # takes off the chord already gathered before it clips to the sub-balls
    "corner": (_box((0, 0, 0), (5, 5, 5), 300, 23), _axes((12, 12, 12))),
    "slab": (_slab, _axes((12, 12, 12))),
    "wide": (lambda: tuple(a * s for a, s in zip(_box((0.3, 1.1, 0.7), (6.3, 7.1, 6.7), 60, 77)(), (1e149, 1.0))),
             [a * 1e149 for a in _axes((8, 8, 8))]),
}


@pytest.mark.parametrize("k", [8, 4])
@pytest.mark.parametrize("name", ["uniform", "far-origin", "overhang"])
def test_rows_small_grids(ctx, name, k):
    _check(ctx, name, k)


def _stamped(ctx, name):
    """The case again through the stamped k = 8 kernel: its outputs and the per-wave counts."""
    ctx.debug_stamps(1)
    try:
        _check(ctx, name, 8)
        c = ctx.debug_stamps(2)
    finally:
        ctx.debug_stamps(0)
    print(f"{name}: waves {c['waves']:.0f}, max per wave {c['max']}")
    return c


def test_void_tiles_previous_pass_chord(ctx):
    _check(ctx, "corner", 8)
    _check(ctx, "corner", 4)
    assert _stamped(ctx, "corner")["max"]["passes"] >= 2


def test_more_than_64_rows_second_round(ctx):
    _check(ctx, "slab", 8)
    _check(ctx, "slab", 4)
    c = _stamped(ctx, "slab")
    # a wave runs one round per pass unless a pass has more than 64 rows
    assert c["max"]["rounds"] > c["max"]["passes"]


def test_particle_on_cell_edge_and_sub_box_plane(ctx):
    """One particle exactly on a cell edge in x and z and on the plane between the two y-halves of
    its tile (y = 5.5: the sub-balls of both halves see it at the same distance).  The cell grid is
    read from a first call; moving an interior particle keeps the particle count and the bounding
    box, and with them the cell grid."""
    make, axes = CASES["uniform"]
    P, Q = make()
    P = P.copy()
    ctx.interp_knn(P, Q, axes=tuple(axes), k=8)
    nc, cs = ctx.stats["cells"], ctx.stats["cell_size"]
    cx, cz = max(1, nc[0] // 2), max(1, nc[2] // 3)
    P[17] = (0.0 + cx * cs[0], 5.5, 0.0 + cz * cs[2])  # o + c * cs as the kernel forms a cell's edge
    assert 0.0 < P[17, 0] < 11.0 and 0.0 < P[17, 2] < 11.0
    for k in (8, 4):
        ref = _reference(P, Q, axes, k)
        out = ctx.interp_knn(P, Q, axes=tuple(axes), k=k)
        assert list(ctx.stats["cells"]) == list(nc) and list(ctx.stats["cell_size"]) == list(cs)
        _compare(out, ref, f"edge particle k={k}")


def test_masked_grid(ctx):
    from ptv_interpolation_amd import _lib, synth

    mask = synth.fluid_mask((12, 12, 12))
    assert mask.any() and not mask.all()
    for k in (8, 4):
        _check(ctx, "uniform", k, mask=mask, fluid_mask=mask, flags=_lib.FLAG_NAN_TO_NUM)


@pytest.mark.parametrize("k", [8, 4])
def test_overflowed_gaps_and_radii_stay_unclipped(ctx, k):
    """tests/_geometry's cloud scaled by 2^80: not a `wide` tile (coordinates below 2^100), but the
    squared sub-ball radii overflow fp32 and so does the squared gap of every row that does not
    pass through a sub-ball's centre.  inf <= inf accepts such a row, and its chord must then be
    the whole row (inf - inf is NaN, of which a square root's guard would make a chord of no
    width).  k = 4 has no `wide` guard at all."""
    from tests import _geometry as geo

    P, Q, ax, ay, az = geo.case("scale_2^80")
    if ("2^80", k) not in _REF:
        _REF[("2^80", k)] = _reference(P, Q, (ax, ay, az), k)
    out = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k)
    _compare(out, _REF[("2^80", k)], f"scale_2^80 k={k}")


def test_wide_tiles_come_out_unclipped(ctx):
    """The grid of tests/test_gpu_knn_tile_phases.py scaled by 1e149: tile-relative coordinates leave
    fp32, the sub-ball radii are infinite and the clip must keep every run whole."""
    _check(ctx, "wide", 8)
