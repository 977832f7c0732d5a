"""The numpy restatement of the staircase interface drag (tests/_drag_ref.py) against the
reference's fixtures (tests/golden/drag_*.npz, made by tests/golden/make_drag_golden.py).

Bounds, derived and not measured.  The restatement's per-face terms are, for float64 fields, the
reference's terms bit for bit, so the reference's key (numpy's pairwise sums, then its own
left-to-right combination of at most 12 of them) lies within gamma(n + 12) S of the exact sum E of
the n terms; the test allows twice that.  For float32 fields the reference rounds each term at most
4 times in float32 and sums in float32: |ref - E64| <= (n + 4) 2^-24 S (1 + 2^-10).  ``Area`` is a
sum of integer counts times a spacing product in a fixed order: compared with ==.
"""
import glob
import os

import numpy as np
import pytest

import _drag_ref as dref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "drag_*.npz"))
               if "perm_" not in os.path.basename(p))


def test_every_case_has_its_fixture():
    assert CASES == sorted(dref.CASES)


@pytest.fixture(scope="module", params=sorted(dref.CASES))
def case(request):
    g = np.load(os.path.join(GOLDEN, f"drag_{request.param}.npz"), allow_pickle=False)
    c = dref.make_case(request.param)
    assert dref.checksum(c) == float(g["checksum"]), "the seeded inputs are not the fixture's"
    assert np.array_equal(np.asarray(c["mask"]), g["mask"])
    return c, g


def test_restatement_matches_the_reference(case):
    c, g = case
    keys = [k.item() for k in g["keys"]]
    labels = c["labels"] if c["labels"] is not None else keys
    terms = dref.face_terms(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"], c["mask"], labels)
    assert list(terms) == keys
    f32 = c["u"].dtype == np.float32
    for i, k in enumerate(keys):
        for j, q in enumerate(dref.KEYS):
            ref = g["values"][i, j]
            if q == "Area":
                assert terms[k][q] == ref, (k, q)
                continue
            e, _, _ = dref.exact(terms[k][q])
            bound = dref.bound32(terms[k][q]) if f32 else 2 * dref.bound64(terms[k][q])
            assert abs(ref - e) <= bound, (k, q, ref, e, bound)


def test_records_reduce_the_same_faces(case):
    c, g = case
    keys = [k.item() for k in g["keys"]]
    labels = c["labels"] if c["labels"] is not None else keys
    rec = dref.records(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"], c["mask"], labels)
    dx, dy, dz = c["spacing"]
    for i, k in enumerate(labels):
        if list(labels).count(k) > 1:
            continue  # the reference sums a repeated label twice; the host assembly test covers it
        area = 0.0
        for axis, a in enumerate((dy * dx, dz * dx, dz * dy)):
            for d in range(2):
                if rec[i, axis, d]["count"]:
                    area += rec[i, axis, d]["count"] * a
        assert area == g["values"][keys.index(k), dref.KEYS.index("Area")], k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_permeability_bound_holds_for_the_reference(dtype):
    """The ramp keeps every sum's condition at or below 10, and the reference's own value stays
    inside the bound the GPU test uses: a relative error of 8 n u max(kappa), with u the unit
    roundoff of the dtype the reference sums in."""
    g = np.load(os.path.join(GOLDEN, f"drag_perm_{np.dtype(dtype).name}.npz"), allow_pickle=False)
    c = dref.make_perm_case(dtype)
    assert dref.checksum(c) == float(g["checksum"])
    _, cond, k = dref.permeability_from_pressure(c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"])
    assert max(cond) <= 10.0, cond
    n = c["u"].size
    u = dref.U64 if dtype == np.float64 else dref.U32
    assert abs(float(g["permeability"]) - k) <= 8 * n * u * max(cond) * abs(k)
