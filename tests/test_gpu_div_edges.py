"""The consistent divergence (csrc/ptv_div.hip) held to the oracle at its edges, bit for bit and
NaN for NaN: non-finite inputs (an un-filled interpolation hands it NaN in every solid cell; only
the face rules decide whether a masked-off neighbour leaks), the extremes of both formats
(``(c + n) * 0.5`` against numpy's ``/ 2.0`` at subnormals and at overflow), every extent at which
the launch changes shape (16-byte lanes or one element per lane, one or two tile columns, chunks of
32 planes in batches of 4), degenerate masks, z-slabs with halos, integer fields, and device
pointers off the 16-byte boundary.

Cases: tests/_rows_edges.py.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _rows_edges as E

pytestmark = pytest.mark.gpu

PY = (0.7, 1.3, 0.9)                 # Python floats: float32 fields stay float32
NP64 = tuple(np.float64(h) for h in (0.25, 1.1, 3.0))  # numpy scalars: float32 fields give float64


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _same(got, exp, what=None):
    """Same dtype and shape, the same NaN pattern, and equal values (sign of zero included) elsewhere."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    assert np.array_equal(got, exp, equal_nan=True), what
    ok = ~np.isnan(exp)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(exp[ok])), what


def _check(u, v, w, m, h, what=None):
    from ptv_interpolation_amd import physics

    with np.errstate(over="ignore", invalid="ignore"):
        exp = cpu_ref.consistent_divergence(u, v, w, m, *h)
    got = physics.compute_consistent_divergence(u, v, w, m, *h)
    _same(got, exp, what)
    return exp


SPACINGS = [(np.float64, PY), (np.float32, PY), (np.float32, NP64)]
SPACING_IDS = ["f64", "f32", "f32_np64_spacing"]


# ----------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("shape", [(6, 7, 16), (6, 7, 13)], ids=["vector", "scalar"])
def test_divergence_nan_in_solid_cells(ctx, shape, dt, h):
    """NaN in every solid cell of u, v and w.  A face towards a solid neighbour is 0, so that
    neighbour's NaN must not show; the cell's own NaN does (the reference does not zero it)."""
    u, v, w, m = E.div_fields(shape, dt, 101)
    u, v, w = E.nan_in_solid(u, v, w, m)
    exp = _check(u, v, w, m, h)
    assert np.isnan(exp).any() and np.isfinite(exp[m]).any()


@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("shape", [(6, 7, 16), (6, 7, 13)], ids=["vector", "scalar"])
def test_divergence_nonfinite_in_fluid_cells(ctx, shape, dt, h):
    u, v, w, m = E.div_fields(shape, dt, 102)
    u, v, w = E.nan_in_solid(u, v, w, m)
    u, v, w = E.nonfinite_in_fluid(u, v, w, m, 103)
    exp = _check(u, v, w, m, h)
    assert np.isinf(exp).any() and np.isnan(exp).any() and np.isfinite(exp).any()


# ----------------------------------------------------------------------------- field extremes
@pytest.mark.parametrize("dt,h", SPACINGS + [(np.float32, (1.0, 1.0, 1.0)), (np.float64, (1.0, 1.0, 1.0))],
                         ids=SPACING_IDS + ["f32_unit", "f64_unit"])
@pytest.mark.parametrize("shape", [(5, 6, 16), (5, 6, 13)], ids=["vector", "scalar"])
def test_divergence_field_extremes(ctx, shape, dt, h):
    """Smallest normals, subnormals, 0.75 max and signed zeros: halving is exact or rounds as numpy's
    division by 2.0 does, and the sums overflow where numpy's do."""
    u, v, w, m = E.extreme_fields(shape, dt, 104)
    exp = _check(u, v, w, m, h)
    assert np.isinf(exp).any()
    if h[0] == 1.0:  # unit spacing keeps the subnormal differences subnormal
        assert ((exp != 0) & (np.abs(exp) < np.finfo(exp.dtype).tiny)).any()


# ----------------------------------------------------------------------------- extents and paths
@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("nx", E.DIV_NX)
def test_divergence_row_extents(ctx, nx, dt, h):
    u, v, w, m = E.div_fields((2, 3, nx), dt, 200 + nx)
    _check(u, v, w, m, h)


@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("nz", E.DIV_NZ)
def test_divergence_plane_extents(ctx, nz, dt, h):
    u, v, w, m = E.div_fields((nz, 2, 8), dt, 300 + nz)
    _check(u, v, w, m, h)


@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("shape", E.DIV_TINY, ids=str)
def test_divergence_singleton_axes(ctx, shape, dt, h):
    for fluid in (0.6, 1.1):
        u, v, w, m = E.div_fields(shape, dt, 400 + sum(shape), fluid=fluid)
        _check(u, v, w, m, h, fluid)


# ----------------------------------------------------------------------------- masks
@pytest.mark.parametrize("dt,h", SPACINGS, ids=SPACING_IDS)
@pytest.mark.parametrize("shape", [(4, 5, 16), (4, 5, 7)], ids=["vector", "scalar"])
def test_divergence_degenerate_masks(ctx, shape, dt, h):
    u, v, w, _ = E.div_fields(shape, dt, 500)
    one = np.zeros(shape, dtype=bool)
    one[2, 3, 5] = True
    labels = np.random.default_rng(501).choice(np.array([0, 2, 255], dtype=np.uint8), size=shape)
    for name, m in (("all fluid", np.ones(shape, bool)), ("all solid", np.zeros(shape, bool)), ("one cell", one),
                    ("labels 0/2/255", labels), ("labels int32", labels.astype(np.int32) * 256)):
        _check(u, v, w, m, h, name)


# ----------------------------------------------------------------------------- slabs with halos
@pytest.mark.parametrize("shape,h,rt", [((70, 6, 13), (0.5, 0.25, 2.0), np.float32),
                                        ((70, 6, 16), tuple(np.float64(s) for s in (0.5, 0.25, 2.0)), np.float64)],
                         ids=["scalar_f32", "vector_f32_to_f64"])
def test_divergence_zslabs_with_halos_equal_whole_f32(ctx, shape, h, rt):
    """test_divergence_zslabs_with_halos_equal_whole on float32 fields: a one-plane slab, slabs of 33
    planes (more than one 32-plane chunk, not a multiple of the 4-plane batch) and one of 3."""
    u, v, w, m = E.div_fields(shape, np.float32, 600, fluid=0.7)
    whole = cpu_ref.consistent_divergence(u, v, w, m, *h)
    assert whole.dtype == rt
    cuts = E.DIV_SLAB_CUTS
    for s, e in zip(cuts[:-1], cuts[1:]):
        lo, hi = max(s - 1, 0), min(e + 1, shape[0])
        sl = slice(lo, hi)
        out = ctx.divergence(u[sl], v[sl], w[sl], m[sl], *[float(x) for x in h], result_dtype=rt,
                             z_range=(s - lo, e - lo), edges=(lo == 0 and s == 0, hi == shape[0] and e == shape[0]))
        _same(out, whole[s:e], (s, e))


# ----------------------------------------------------------------------------- integer fields
@pytest.mark.parametrize("dtype", [np.int16, np.int64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(4, 5, 16), (4, 5, 7)], ids=["vector", "scalar"])
def test_divergence_integer_fields(ctx, shape, dtype):
    """Integer fields are widened: (int + int) / 2.0 is float64 in the reference."""
    rng = np.random.default_rng(700)
    u, v, w = (rng.integers(-99, 100, shape).astype(dtype) for _ in range(3))
    m = rng.uniform(size=shape) < 0.6
    exp = _check(u, v, w, m, PY)
    assert exp.dtype == np.float64


# ----------------------------------------------------------------------------- device pointers
def test_divergence_device_pointers_off_alignment(ctx):
    """Field, mask and output pointers one element past a 16-byte boundary with nx % 4 == 0: the launch
    must give up its 16-byte lanes and still equal the oracle."""
    import torch

    from ptv_interpolation_amd import _lib

    shape = (5, 6, 16)
    n = int(np.prod(shape))
    u, v, w, m = E.div_fields(shape, np.float32, 800)
    u, v, w = E.nan_in_solid(u, v, w, m)

    def shifted(a):
        buf = torch.zeros(n + 8, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
        t = buf[1:n + 1]
        t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        return buf, t

    bufs = [shifted(a) for a in (u, v, w)]
    mbuf, dm = shifted(m.view(np.uint8))
    obuf, out = shifted(np.zeros(shape, dtype=np.float32))
    for _, t in bufs:
        assert t.data_ptr() % 16 == 4
    assert dm.data_ptr() % 4 == 1 and out.data_ptr() % 16 == 4
    torch.cuda.synchronize()
    ctx.divergence_dev(shape[2], shape[1], shape[0], [t.data_ptr() for _, t in bufs], dm.data_ptr(), out.data_ptr(),
                       *PY, field_dtype=_lib.F32, result_dtype=_lib.F32,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        exp = cpu_ref.consistent_divergence(u, v, w, m, *PY)
    _same(out.cpu().numpy().reshape(shape), exp)
    assert float(obuf[0]) == 0.0 and float(obuf[n + 1]) == 0.0  # nothing written outside the slice
