"""GPU checks of the mask alignment (csrc/ptv_edt.hip): the exact distance transform against
scipy, the score against the numpy restatement (tests/_align_ref.py, held to the reference's
fixtures by test_align_oracle.py), and ``find_best_offset`` against the reference's recorded search.

Transform: ``d2 == rint(scipy ** 2)`` as integers and the float64 field ``== scipy``, both exact.
Shapes are the smallest that reach every path: single voxels and length-1 axes; a row longer than a
wave ((3, 4, 70)); long columns with few lanes; more than one block on every axis ((33, 65, 130));
and the axis lengths at which an envelope pass changes kernel: 300 (an LDS tile past 64 KB, 1024
threads) and 700 (past kEdtStagedMax = 640: no tile), on the y and on the z axis.

Score: counts with ``==``; the sum within ``2 gamma(n + c) S`` of numpy's, c = 1024 the most
per-block partial sums the closing kernel combines (kAlignMaxBlocks), derived in _align_ref.py; on
the layered fixture every distance is an integer, every sum exact, and everything compares with
``==``, Powell's whole path included.
"""
import os
import sys

import numpy as np
import pytest

import _align_ref as aref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1, 1), (1, 1, 7), (2, 2, 2), (1, 5, 9), (5, 1, 9), (5, 7, 9), (3, 4, 70), (70, 3, 4), (3, 70, 4),
          (33, 65, 130), (300, 3, 4), (3, 300, 4), (700, 3, 4), (3, 700, 4)]
SIZES = [0, 1, 63, 64, 65, 4097, 100003]


@pytest.fixture(scope="module")
def al():
    from ptv_interpolation_amd import _lib, alignment

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return alignment


def _masks(shape):
    """name -> mask (nonzero = foreground), each with at least one zero."""
    rng = np.random.default_rng(sum(shape) * 7 + shape[0])
    nz, ny, nx = shape
    out = {"all zero": np.zeros(shape, dtype=bool)}
    m = np.ones(shape, dtype=bool)
    m[-1, -1, -1] = False
    out["corner zero"] = m
    m = np.ones(shape, dtype=bool)
    m[nz // 2, ny // 2, :] = rng.random(nx) < 0.5
    m[nz // 2, ny // 2, rng.integers(nx)] = False
    out["one row"] = m  # every other row carries the sentinel into the y pass
    m = np.ones(shape, dtype=bool)
    m[nz // 3] = rng.random((ny, nx)) < 0.7
    m[nz // 3, rng.integers(ny), rng.integers(nx)] = False
    out["one plane"] = m
    z, y, x = np.indices(shape)
    out["checkerboard"] = ((z + y + x) % 2).astype(bool)  # voxel (0, 0, 0) is a zero
    for fill in (0.5, 0.99, 0.999):
        m = rng.random(shape) < fill
        if m.all():
            m.flat[rng.integers(m.size)] = False
        out[f"fill {fill}"] = m
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_equals_scipy(al, shape):
    for name, mask in _masks(shape).items():
        want = aref.edt(mask)
        want2 = aref.edt2(mask)
        got = al.distance_transform_edt(mask)
        got2 = al.distance_transform_edt(mask, return_squared=True)
        assert got.dtype == np.float64 and got2.dtype == np.int32 and got.shape == shape, name
        assert np.array_equal(got2, want2), (name, int((got2 != want2).sum()))
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_transform_equals_the_definition(al):
    rng = np.random.default_rng(3)
    mask = rng.random((9, 10, 11)) < 0.8
    assert np.array_equal(al.distance_transform_edt(mask, return_squared=True), aref.edt2_brute(mask))


def test_transform_dtypes_and_repeats(al):
    rng = np.random.default_rng(4)
    mask = rng.random((5, 7, 70)) < 0.9
    ref = al.distance_transform_edt(mask)
    assert np.array_equal(ref, aref.edt(mask))
    for m in (mask.view(np.uint8), mask.astype(np.int32) * -5, mask.astype(np.uint8) * 200, mask.astype(np.int64) << 40):
        assert np.array_equal(al.distance_transform_edt(m), ref), m.dtype
    assert np.array_equal(al.distance_transform_edt(mask), ref)
    assert np.array_equal(al.distance_transform_edt(np.asfortranarray(mask)), ref)
    d2 = al.distance_transform_edt(mask, return_squared=True)
    assert d2.dtype == np.int32 and np.array_equal(np.sqrt(d2.astype(np.float64)), ref)


def test_transform_without_a_zero_raises(al):
    for shape in ((3, 4, 5), (1, 1, 1), (2, 70, 3)):
        with pytest.raises(ValueError):
            al.distance_transform_edt(np.ones(shape, dtype=bool))
    # and the context is usable afterwards
    assert al.distance_transform_edt(np.zeros((2, 2, 2), dtype=bool)).sum() == 0.0


def test_transform_empty(al):
    assert al.distance_transform_edt(np.ones((0, 3, 4), dtype=bool)).shape == (0, 3, 4)


# ---- the score ----
@pytest.fixture(scope="module")
def blob():
    """A blob solid mask, its scipy distance field, and 100003 points scattered over and around it."""
    rng = np.random.default_rng(12)
    coarse = rng.random((4, 5, 6)) < 0.55
    solid = np.repeat(np.repeat(np.repeat(coarse, 5, 0), 5, 1), 5, 2)[:19, :23, :29].copy()
    solid[0, 0, 0] = False
    dt = aref.edt(solid)
    nz, ny, nx = solid.shape
    pts = rng.uniform(-3.0, 3.0, (max(SIZES), 3)) + rng.uniform(0, 1, (max(SIZES), 3)) * np.array([nx, ny, nz])
    return solid, dt, pts


def _check(al, pts, dt, offsets, exact=False):
    vals, rec = al.alignment_objective(pts, dt, offsets)
    assert vals.dtype == np.float64 and len(vals) == len(offsets) == len(rec)
    for o, v, r in zip(offsets, vals, rec):
        n_in, n_out, s, e = aref.record(pts, dt, o)
        assert (int(r["n_inside"]), int(r["n_outside"])) == (n_in, n_out), o
        want = aref.objective(pts, dt, o)
        if exact:
            assert r["sum"] == s and v == want, (o, v, want)
        else:
            bound = 2 * aref.sum_bound(n_in, e)
            assert abs(r["sum"] - s) <= bound, (o, r["sum"], s, bound)
            if n_in == 0:
                assert v == aref.OUTSIDE_SCORE
            else:
                assert v == r["sum"] + np.int64(n_out) * dt.max()
                assert abs(v - want) <= bound * (1 + 2.0**-50) + 2.0**-52 * abs(want), (o, v, want)
    return vals, rec


@pytest.mark.parametrize("n", SIZES)
def test_score_against_the_restatement(al, blob, n):
    _, dt, pts = blob
    _check(al, pts[:n], dt, aref.PROBE_OFFSETS[[0, 2, 3, 4]])


def test_score_from_a_mask_equals_score_from_its_field(al, blob):
    solid, dt, pts = blob
    v1, r1 = al.alignment_objective(pts[:4097], dt, aref.PROBE_OFFSETS)
    for m in (solid, solid.astype(np.int32) * 3):
        v2, r2 = al.alignment_objective(pts[:4097], m, aref.PROBE_OFFSETS)
        assert np.array_equal(v1, v2) and np.array_equal(r1, r2)


def test_score_halves_and_faces(al, blob):
    _, dt, _ = blob
    nz, ny, nx = dt.shape
    halves = [0.5, 1.5, 2.5, -0.5]
    rows = [(h, 1.0, 1.0) for h in halves + [nx - 0.5, nx - 1.5]]
    rows += [(1.0, h, 1.0) for h in halves + [ny - 0.5, ny - 1.5]]
    rows += [(1.0, 1.0, h) for h in halves + [nz - 0.5, nz - 1.5]]
    # beyond each of the six faces, and just inside them
    rows += [(-0.51, 1, 1), (nx - 0.49, 1, 1), (1, -0.51, 1), (1, ny - 0.49, 1), (1, 1, -0.51), (1, 1, nz - 0.49),
             (-0.49, 1, 1), (nx - 0.51, 1, 1), (1, -0.49, 1), (1, ny - 0.51, 1), (1, 1, -0.49), (1, 1, nz - 0.51),
             (-1e300, 1, 1), (1, 1e300, 1), (1, 1, 3e9), (-3e9, 1, 1)]
    pts = np.array(rows, dtype=np.float64)
    # one point at a time: each lands where np.round puts it
    for p in pts:
        _check(al, p[None, :], dt, np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.5, 0.0]]))
    _check(al, pts, dt, aref.PROBE_OFFSETS)
    # -0.5 rounds to index 0 (inside), nx - 0.5 to nx or nx - 1 by parity
    _, rec = al.alignment_objective(np.array([[-0.5, -0.5, -0.5]]), dt, [(0, 0, 0)])
    assert rec["n_inside"][0] == 1
    _, rec = al.alignment_objective(np.array([[nx - 0.5, 0.0, 0.0]]), dt, [(0, 0, 0)])
    assert rec["n_inside"][0] == (1 if nx % 2 == 1 else 0)


def test_all_points_outside_and_no_points(al, blob):
    _, dt, pts = blob
    vals, rec = al.alignment_objective(pts[:1000], dt, [(1e4, 0, 0), (0, -1e4, 0)])
    assert list(vals) == [1e9, 1e9] and list(rec["n_inside"]) == [0, 0] and list(rec["n_outside"]) == [1000, 1000]
    vals, rec = al.alignment_objective(np.zeros((0, 3)), dt, [(0, 0, 0)])
    assert vals[0] == 1e9 and rec["n_inside"][0] == 0 and rec["n_outside"][0] == 0


def test_a_batch_equals_single_calls_and_repeats(al, blob):
    _, dt, pts = blob
    v, r = al.alignment_objective(pts, dt, aref.PROBE_OFFSETS)
    assert len(v) == 7
    for i, o in enumerate(aref.PROBE_OFFSETS):
        v1, r1 = al.alignment_objective(pts, dt, o[None, :])
        assert v1[0] == v[i] and r1[0] == r[i], i
    v2, r2 = al.alignment_objective(pts, dt, aref.PROBE_OFFSETS)
    assert np.array_equal(v, v2) and np.array_equal(r, r2)


def test_session_scores_without_a_second_upload(al, blob):
    from ptv_interpolation_amd import _lib

    solid, dt, pts = blob
    ctx = _lib.Context.get(0)
    s = _lib.AlignSession(ctx, pts[:4097], dt.shape, dt)
    a = s.score(aref.PROBE_OFFSETS)
    assert ctx._align_owner is s
    b = s.score(aref.PROBE_OFFSETS)  # resident: NULL points and field
    assert np.array_equal(a, b)
    other = _lib.AlignSession(ctx, pts[:63], dt.shape, dt)
    other.score(aref.PROBE_OFFSETS[:1])
    assert np.array_equal(s.score(aref.PROBE_OFFSETS), a)  # uploads again after the other session
    with pytest.raises(ValueError):  # the context holds 4097 points, not 5
        ctx.align_score(dt.shape, 5, aref.PROBE_OFFSETS[:1])


def test_layered_fixture_everything_exact(al):
    g = np.load(os.path.join(GOLDEN, "align_layered.npz"), allow_pickle=False)
    dt = aref.edt(~g["mask"])
    assert np.array_equal(al.distance_transform_edt(~g["mask"]), dt)
    vals, _ = _check(al, g["points"], dt, g["probe_offsets"], exact=True)
    assert np.array_equal(vals, g["probe_values"])
    vals, _ = al.alignment_objective(g["points"], ~g["mask"], g["probe_offsets"])
    assert np.array_equal(vals, g["probe_values"])


# ---- find_best_offset ----
def test_find_best_offset_layered_equals_the_reference(al, capsys):
    g = np.load(os.path.join(GOLDEN, "align_layered.npz"), allow_pickle=False)
    x, fun = al.find_best_offset(aref.Frame(g["points"]), g["mask"], initial_offset=tuple(g["initial"]))
    assert np.array_equal(x, g["res_x"]) and fun == g["res_fun"]
    out = capsys.readouterr().out
    assert "Computing Distance Transform..." in out and "Starting optimization from initial offset" in out
    # invert: the same search over the complement given as the solid
    x2, fun2 = al.find_best_offset(aref.Frame(g["points"]), ~g["mask"], initial_offset=tuple(g["initial"]), invert=True)
    assert np.array_equal(x2, x) and fun2 == fun


def test_find_best_offset_layered_through_the_root_shim(al):
    sys.modules.pop("auto_align", None)
    import auto_align

    assert auto_align.find_best_offset is al.find_best_offset or auto_align.find_best_offset.__module__ == al.__name__
    g = np.load(os.path.join(GOLDEN, "align_layered.npz"), allow_pickle=False)
    x, fun = auto_align.find_best_offset(aref.Frame(g["points"]), g["mask"], initial_offset=tuple(g["initial"]))
    assert np.array_equal(x, g["res_x"]) and fun == g["res_fun"]


def test_find_best_offset_blob(al):
    g = np.load(os.path.join(GOLDEN, "align_blob.npz"), allow_pickle=False)
    pts, mask = g["points"], g["mask"]
    dt = aref.edt(~mask)
    x, fun = al.find_best_offset(aref.Frame(pts), mask, initial_offset=tuple(g["initial"]))
    n_in, _, _, e = aref.record(pts, dt, x)
    want = aref.objective(pts, dt, x)
    assert abs(fun - want) <= 2 * aref.sum_bound(n_in, e) * (1 + 2.0**-50) + 2.0**-52 * abs(want), (fun, want)
    assert fun <= aref.objective(pts, dt, g["initial"])
