"""GPU checks of the staircase interface drag (csrc/ptv_drag.hip behind ``ptv_interface_drag``) and
of the pressure-based permeability (``ptv_gradient_sums``), against the reference's fixtures
(tests/golden/drag_*.npz) and, off their dtypes, against the numpy restatement that
test_drag_oracle.py holds to those fixtures.

Shapes are the smallest that reach every path: (2, 2, 2); a length-1 axis ((1, 5, 9), (5, 1, 9));
nothing a multiple of anything ((5, 7, 9)); 70 labels, more than one LDS chunk of 32 ((12, 20, 33));
many blocks of 4096 voxels and every wave of a block ((40, 48, 130)).  One label takes the register
path, several the LDS path.

Tolerances, derived and not measured (tests/_drag_ref.py).  The device's per-face terms are float64
and, for float64 fields, the reference's bit for bit.  Any order of summing n float64 terms lies
within gamma(n) S of their exact sum E; the host combines at most 12 partial sums per key, so
|gpu - E| <= gamma(n + 12) S, and |gpu - ref| <= 2 gamma(n + 12) S.  For float32 fields E is taken
of the float64 terms of the float32 inputs (the device widens on load) and the fixture is allowed
its own float32 bound (n + 4) 2^-24 S (1 + 2^-10) on top.  Counts and ``Area`` are compared with ==.
"""
import math
import os

import numpy as np
import pytest

import _drag_ref as dref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# shape, labels in the mask, coarse cell of the blobs
SHAPES = [((2, 2, 2), 2, (1, 1, 1)), ((1, 5, 9), 3, (1, 1, 2)), ((5, 1, 9), 3, (1, 1, 2)), ((5, 7, 9), 4, (1, 2, 2)),
          ((12, 20, 33), 70, (2, 2, 3)), ((40, 48, 130), 8, (6, 7, 9))]


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


@pytest.fixture(scope="module")
def va():
    from ptv_interpolation_amd import velocity_analysis

    return velocity_analysis


def _args(c):
    return (c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"], c["mask"])


_TERMS = {}


def _terms(key, c, labels):
    """The restatement's per-face terms, computed once per case and left unchanged."""
    if key not in _TERMS:
        _TERMS[key] = dref.face_terms(*_args(c), labels)
    return _TERMS[key]


def _check_against_terms(res, terms):
    assert list(res) == list(terms)
    for k, r in res.items():
        assert r["Area"] == terms[k]["Area"], (k, r["Area"], terms[k]["Area"])
        for q in dref.FORCE_KEYS:
            e, _, _ = dref.exact(terms[k][q])
            assert abs(r[q] - e) <= dref.bound64(terms[k][q]), (k, q, r[q], e, dref.bound64(terms[k][q]))
        for ax in "xyz":
            assert r[f"F{ax}"] == r[f"F{ax}_v"] + r[f"F{ax}_p"]


@pytest.mark.parametrize("name", sorted(dref.CASES))
def test_reference_fixtures(va, name):
    g = np.load(os.path.join(GOLDEN, f"drag_{name}.npz"), allow_pickle=False)
    c = dref.make_case(name)
    assert dref.checksum(c) == float(g["checksum"]), "the seeded inputs are not the fixture's"
    keys = [k.item() for k in g["keys"]]
    labels = c["labels"] if c["labels"] is not None else keys
    res = va.compute_interface_drag(*_args(c), labels=c["labels"])
    terms = _terms(name, c, labels)
    _check_against_terms(res, terms)
    f32 = c["u"].dtype == np.float32
    for i, k in enumerate(keys):
        for j, q in enumerate(dref.KEYS):
            ref, got = g["values"][i, j], res[k][q]
            if q == "Area":
                assert got == ref, (k, got, ref)
                continue
            b64 = dref.bound64(terms[k][q])
            bound = b64 + dref.bound32(terms[k][q]) if f32 else 2 * b64
            assert abs(got - ref) <= bound, (k, q, got, ref, bound)
        if c["pressure"] is None:
            assert res[k]["Fx_p"] == 0.0 and res[k]["Fy_p"] == 0.0 and res[k]["Fz_p"] == 0.0
    if c["labels"] is None:
        assert list(res) == [np.True_] and isinstance(list(res)[0], np.bool_)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,nlab,cell", SHAPES)
def test_shapes_against_the_restatement(ctx, va, shape, nlab, cell, dtype):
    c = dref.make_inputs(shape, dtype, nlab, cell, None, seed=31 * sum(shape) + np.dtype(dtype).itemsize)
    labels = c["labels"]
    res = va.compute_interface_drag(*_args(c), labels=labels, volume=2.0)
    _check_against_terms(res, dref.face_terms(*_args(c), labels))
    for r in res.values():
        assert r["Mx"] == r["Fx"] / 2.0
    # every face count, and the one-label register path against the same label's LDS-path result
    rec, _ = ctx.interface_drag(c["mask"], c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"],
                                labels)
    want = dref.records(*_args(c), labels)
    assert np.array_equal(rec["count"], want["count"])
    one, _ = ctx.interface_drag(c["mask"], c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"], [1])
    assert np.array_equal(one["count"], want["count"][:1])
    terms = dref.face_terms(*_args(c), [1])[1]
    single = va.compute_interface_drag(*_args(c), labels=[1])[1]
    for q in dref.FORCE_KEYS:
        assert abs(single[q] - dref.exact(terms[q])[0]) <= dref.bound64(terms[q]), q


@pytest.mark.parametrize("fill", [0, 3])
def test_all_fluid_and_all_solid(va, fill):
    c = dref.make_inputs((5, 7, 9), np.float64, 4, (1, 2, 2), None, seed=5)
    mask = np.full((5, 7, 9), fill, dtype=np.int16)
    res = va.compute_interface_drag(*_args(c)[:-1], mask, labels=[1, 3], volume=1.0)
    assert list(res) == [1, 3]
    for r in res.values():
        assert all(r[q] == 0.0 for q in r), r
        assert r["Area"] == 0.0
    if fill == 0:
        assert va.compute_interface_drag(*_args(c)[:-1], mask) == {}


def test_label_order_and_repeat_calls_do_not_change_a_bit(va):
    c = dref.make_case("f64_70")
    labels = c["labels"]
    first = va.compute_interface_drag(*_args(c), labels=labels)
    again = va.compute_interface_drag(*_args(c), labels=labels)
    backward = va.compute_interface_drag(*_args(c), labels=labels[::-1])
    some = va.compute_interface_drag(*_args(c), labels=[40, 3, 69])  # other neighbours in the table, other chunks
    assert list(backward) == labels[::-1]
    for k in labels:
        for q in first[k]:
            a = np.float64(first[k][q])
            assert a.tobytes() == np.float64(again[k][q]).tobytes(), (k, q)
            assert a.tobytes() == np.float64(backward[k][q]).tobytes(), (k, q)
            if k in some:
                assert a.tobytes() == np.float64(some[k][q]).tobytes(), (k, q)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_permeability_from_pressure(ctx, va, dtype):
    g = np.load(os.path.join(GOLDEN, f"drag_perm_{np.dtype(dtype).name}.npz"), allow_pickle=False)
    c = dref.make_perm_case(dtype)
    assert dref.checksum(c) == float(g["checksum"])
    dx, dy, dz = c["spacing"]
    sums, cond, k_exact = dref.permeability_from_pressure(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"],
                                                          dx, dy, dz)
    n = c["u"].size
    # the six sums: np.gradient's values bit for bit, summed in float64 in some fixed order
    _, st = ctx.flow_analysis(c["u"], c["v"], c["w"], dx, dy, dz, outputs=())
    gz, gy, gx = ctx.gradient_sums(c["pressure"], dx, dy, dz)
    comps = np.gradient(c["pressure"], dz, dy, dx)
    fields = (c["u"], c["v"], c["w"], comps[2], comps[1], comps[0])
    for got, e, a in zip((st["sum_u"], st["sum_v"], st["sum_w"], gx, gy, gz), sums, fields):
        s = math.fsum(np.abs(np.asarray(a, dtype=np.float64)).ravel())
        print("sum", got, e, abs(got - e), dref.gamma(n) * s)
        assert abs(got - e) <= dref.gamma(n) * s, (got, e)
    assert ctx.gradient_sums(c["pressure"], dx, dy, dz) == [gz, gy, gx]  # the same bits on every call
    k = va.compute_permeability_from_pressure(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], dx, dy, dz)
    assert max(cond) <= 10.0
    print("k", k, k_exact, float(g["permeability"]))
    assert abs(k - k_exact) <= 8 * n * dref.U64 * max(cond) * abs(k_exact)
    u_ref = dref.U64 if dtype == np.float64 else dref.U32  # what the reference sums in
    assert abs(k - float(g["permeability"])) <= 8 * n * (dref.U64 + u_ref) * max(cond) * abs(k_exact)


def test_permeability_of_a_constant_pressure_is_zero(va):
    c = dref.make_perm_case(np.float64, shape=(5, 7, 9))
    p = np.full((5, 7, 9), 3.25)
    k = va.compute_permeability_from_pressure(c["u"], c["v"], c["w"], p, c["viscosity"], *c["spacing"])
    assert k == 0.0 and type(k) is float
