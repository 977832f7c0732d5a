"""The host entry points of the grid-field families stage through one pool of the context
(csrc/ptv_stage.hpp) and run what their ``_dev`` entry points run.

1. Host and ``_dev`` entry point give the same bytes and the same stats (timings aside), on the
   two-wide (even nx) and the one-wide (odd nx) path.
2. Families interleaved on one context, so that the pool's slots grow, shrink and change element
   type, give what each call gives alone on a fresh context.
3. A rejected call between two good ones leaves the second one's bytes as they are."""
import ctypes as C

import numpy as np
import pytest

import _host_staging as hs

pytestmark = pytest.mark.gpu

PAIRS = [(name, shape, dt) for name, (dts, _) in hs.CASES.items() for shape in hs.SHAPES for dt in dts]
_inputs = {}


def inputs(shape, dtype=np.float64):
    key = (shape, np.dtype(dtype))
    if key not in _inputs:
        _inputs[key] = hs.Inputs(shape, dtype)
    return _inputs[key]


_alone = {}


def alone(name, shape, dtype=np.float64):
    """The host call on a fresh context of its own (made once per case)."""
    from ptv_interpolation_amd import _lib

    key = (name, shape, np.dtype(dtype))
    if key not in _alone:
        ctx = _lib.Context(0)
        try:
            _alone[key] = hs.CASES[name][1](ctx, inputs(shape, dtype), False)
        finally:
            ctx.close()
    return _alone[key]


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name,shape,dtype", PAIRS, ids=[f"{n}-{s}-{np.dtype(d).name}" for n, s, d in PAIRS])
def test_host_and_dev_entry_points_agree(ctx, name, shape, dtype):
    fn = hs.CASES[name][1]
    host = fn(ctx, inputs(shape, dtype), False)
    dev = fn(ctx, inputs(shape, dtype), True)
    assert len(host[0]) > 0
    assert hs.same(host, dev), (hs.untimed(host[1]), hs.untimed(dev[1]))


# (7, 9, 13) float64 clean -> (5, 4, 2) float32 flow -> (7, 9, 13) pressure -> drag -> edt -> (5, 4, 2) variational
SEQUENCE = [("clean", (7, 9, 13), np.float64), ("flow analysis", (5, 4, 2), np.float32),
            ("pressure", (7, 9, 13), np.float64), ("interface drag", (7, 9, 13), np.float32),
            ("edt", (7, 9, 13), np.float64), ("variational", (5, 4, 2), np.float64)]


def test_interleaved_families_share_the_pool():
    from ptv_interpolation_amd import _lib

    c = _lib.Context(0)
    try:
        got = [hs.CASES[name][1](c, inputs(shape, dt), False) for name, shape, dt in SEQUENCE]
    finally:
        c.close()
    for (name, shape, dt), res in zip(SEQUENCE, got):
        assert hs.same(res, alone(name, shape, dt)), (name, shape)


def _rejected_clean(c, d, nx=None, with_mask=True):
    """ptv_clean_divergence with a bad argument, through the host entry point itself."""
    from ptv_interpolation_amd import _lib

    mk = np.ascontiguousarray(d.mask).view(np.uint8)
    prm = _lib.CleanParams(d.nx if nx is None else nx, d.ny, d.nz, *hs.H,
                           mk.ctypes.data_as(C.POINTER(C.c_uint8)) if with_mask else None, 2, 1e-8, 1e-10, 1e-10, 10)
    out = [np.empty_like(a) for a in d.f[:3]]
    st = _lib.CleanStats()
    _lib.check(_lib.lib().ptv_clean_divergence(c.h, C.byref(prm), *[_lib.as_dp(a) for a in d.f[:3]],
                                               *[_lib.as_dp(a) for a in out], C.byref(st)))


@pytest.mark.parametrize("bad", [dict(nx=-3), dict(with_mask=False)], ids=["negative dimension", "missing mask"])
def test_a_rejected_call_leaves_the_next_one_alone(bad):
    from ptv_interpolation_amd import _lib

    shape = (7, 9, 13)
    c = _lib.Context(0)
    try:
        first = hs.CASES["clean"][1](c, inputs(shape), False)
        with pytest.raises(ValueError):
            _rejected_clean(c, inputs((5, 4, 2)), **bad)
        second = hs.CASES["clean"][1](c, inputs(shape), False)
        third = hs.CASES["flow analysis"][1](c, inputs((5, 4, 2), np.float32), False)
    finally:
        c.close()
    assert hs.same(first, second)
    assert hs.same(second, alone("clean", shape))
    assert hs.same(third, alone("flow analysis", (5, 4, 2), np.float32))
