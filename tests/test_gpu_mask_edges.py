"""The pore-mask path (csrc/ptv_mask.hip) held to the oracle at its edges, bit for bit.

``sample_mask_on_grid``: exact half-way points (the ``t <= 0.5`` rule), descending raw axes, both
in-bounds end points, length-1 raw axes, every row-store alignment of ``k_mask_sample_sep``, and
z-slab launches against the whole grid.  ``extract_boundary_particles``: the 16-voxel (SWAR) kernels
and the per-voxel ones on the same pictures at one lane per row, several waves and several blocks,
every thickness 1..4 (the dilation ping-pong) and sampling steps 1, 2, 7; integer masks whose low
byte hides the value; more than 1024 count blocks (the carry loop of ``k_boundary_scan``).

Cases: tests/_rows_edges.py.  tests/test_rows_edge_cases.py holds the oracle to scipy on them.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _rows_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


# ----------------------------------------------------------------------------- sample_mask_on_grid
@pytest.mark.parametrize("case", E.mask_sample_cases(), ids=lambda c: c[0])
def test_sample_mask_edges(ctx, case):
    from ptv_interpolation_amd import interpolator as ip

    _, raw, bounds, (ax, ay, az) = case
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    with np.errstate(invalid="ignore"):
        exp = cpu_ref.sample_mask_nearest(raw, bounds, X, Y, Z)
        got = ip.sample_mask_on_grid(raw, (X, Y, Z), bounds)
        flat = ip.sample_mask_on_grid(raw, (X.ravel(), Y.ravel(), Z.ravel()), bounds)
    assert got.dtype == np.bool_ and got.shape == exp.shape and np.array_equal(got, exp)
    assert flat.dtype == np.bool_ and flat.shape == (X.size,) and np.array_equal(flat, exp.ravel())


def _raw_axes(raw, bounds):
    nz, ny, nx = raw.shape
    return [np.linspace(lo, hi - 1, n) for (lo, hi), n in zip(bounds, (nx, ny, nz))]


@pytest.mark.parametrize("point_list", [False, True], ids=["axes", "grid_points"])
def test_sample_mask_zslabs_equal_whole(ctx, point_list):
    raw, bounds, (ax, ay, az) = E.slab_case()
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    exp = cpu_ref.sample_mask_nearest(raw, bounds, X, Y, Z)
    raw_bytes = (raw.astype(float) > 0.5).view(np.uint8)
    kw = dict(grid_points=(X, Y, Z), shape=X.shape) if point_list else dict(axes=(ax, ay, az))
    whole = ctx.sample_mask(raw_bytes, _raw_axes(raw, bounds), **kw)
    assert whole.dtype == np.uint8 and np.array_equal(whole.view(bool), exp)
    parts = []
    for a, b in E.SLABS:
        b = len(az) if b is None else b
        part = ctx.sample_mask(raw_bytes, _raw_axes(raw, bounds), z_range=(a, b), **kw)
        assert part.shape == (b - a,) + exp.shape[1:]
        assert np.array_equal(part.view(bool), exp[a:b]), (a, b)
        parts.append(part)
    assert np.array_equal(np.concatenate(parts), whole)


# ----------------------------------------------------------------------------- extract_boundary_particles
def _check_boundary(m, bounds, thicknesses=E.THICKNESSES, steps=E.STEPS, nonempty=False):
    from ptv_interpolation_amd import interpolator as ip

    for t in thicknesses:
        for step in steps:
            got = ip.extract_boundary_particles(m, bounds, sampling_step=step, thickness=t)
            exp = cpu_ref.boundary_particles(m, bounds, step, t)
            assert len(got) == 3
            assert not nonempty or len(exp[0]) > 0
            for a, e in zip(got, exp):
                assert a.dtype == e.dtype and a.shape == e.shape and np.array_equal(a, e), (t, step)


@pytest.mark.parametrize("shape", E.SWAR_SHAPES + E.GENERIC_SHAPES, ids=str)
@pytest.mark.parametrize("kind", E.MASK_KINDS)
def test_boundary_particles_pictures(ctx, kind, shape):
    """(.., 16), (.., 48), (.., 64): the 16-voxel kernels at one lane per row, with both carry bytes,
    and over 3 blocks; (.., 47), (.., 63): the same pictures on the per-voxel kernels."""
    _check_boundary(E.bool_mask(kind, shape), E.shape_bounds(shape), nonempty=True)


@pytest.mark.parametrize("dtype", E.WIDE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(6, 9, 48), (6, 9, 47)], ids=str)
def test_boundary_particles_wide_integer_masks(ctx, shape, dtype):
    """numpy's `bool & ~int` keeps the value's low bit; 256, 65536 and 2**40 are fluid with a zero low
    byte, -1 and 257 are odd with high bits set."""
    _check_boundary(E.wide_mask(shape, dtype), E.shape_bounds(shape), thicknesses=(1, 3), nonempty=True)


@pytest.mark.parametrize("shape", E.SCAN_SHAPES, ids=str)
def test_boundary_particles_scan_carry(ctx, shape):
    """1040 count blocks: the single-block scan loops twice and carries the first 1024 blocks' total."""
    _check_boundary(E.scan_mask(shape), E.shape_bounds(shape), thicknesses=(2,), steps=(1, 5), nonempty=True)


@pytest.mark.parametrize("shape", E.DEGENERATE_SHAPES, ids=str)
def test_boundary_particles_degenerate_axes(ctx, shape):
    _check_boundary(E.degenerate_mask(shape), E.shape_bounds(shape))


@pytest.mark.parametrize("shape", [(6, 9, 48), (6, 9, 47)], ids=str)
def test_boundary_particles_step_beyond_count(ctx, shape):
    """A sampling step larger than the number of boundary voxels keeps the first one only."""
    from ptv_interpolation_amd import interpolator as ip

    m = E.bool_mask("blob", shape)
    b = E.shape_bounds(shape)
    n = len(cpu_ref.boundary_particles(m, b, 1, 2)[0])
    assert n > 1
    for step in (n - 1, n, n + 1, 10 * n):
        got = ip.extract_boundary_particles(m, b, sampling_step=step, thickness=2)
        exp = cpu_ref.boundary_particles(m, b, step, 2)
        assert len(exp[0]) == (2 if step == n - 1 else 1)
        for a, e in zip(got, exp):
            assert a.dtype == e.dtype and np.array_equal(a, e)


@pytest.mark.parametrize("shape", [(9, 17, 64), (9, 17, 63)], ids=str)
def test_boundary_particles_device_entry_count(ctx, shape):
    import torch

    m = E.bool_mask("blob", shape)
    b = E.shape_bounds(shape)
    dm = torch.from_numpy(m.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    for t, step in ((1, 1), (3, 2), (4, 7)):
        n = ctx.boundary_particles_dev(dm.data_ptr(), shape, t, step, [0.0] * 3, [1.0] * 3, [1.0] * 3)
        assert n == len(cpu_ref.boundary_particles(m, b, step, t)[0]), (t, step)
