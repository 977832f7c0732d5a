"""The numpy restatement of the flow analysis (tests/_flow_ref.py) against the fixtures the reference
wrote (tests/golden/flow_*.npz, make_flow_golden.py): every field and the permeability, bit for bit.
The GPU tests use the restatement as their oracle off the fixtures' shapes."""
import glob
import os
import warnings

import numpy as np
import pytest

import _flow_ref as fref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "flow_*.npz")))


def test_the_fixtures_cover_the_cases():
    for name in ("f64_py", "f64_np64", "f32_py", "f32_np64", "small_222", "small_253", "all_solid", "naninf", "int"):
        assert name in CASES, name


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    c = fref.load_case(os.path.join(GOLDEN, f"flow_{name}.npz"))
    args = (c["u"], c["v"], c["w"], c["dx"], c["dy"], c["dz"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the NaN / inf case
        got = fref.analyze(*args, c["viscosity"], c["mask"])
        k = fref.compute_permeability(c["u"], c["v"], c["w"], got["dissipation"], c["viscosity"], c["dx"], c["dy"],
                                      c["dz"], c["mask"])
    for out in fref.OUTPUTS:
        assert fref.same(got[out], c[out]), (name, out)
    assert fref.same(k, c["permeability"]), (name, k, c["permeability"])


def test_fixture_kinds():
    """What the names promise: dtypes, spacing kinds, masks, the special values."""
    load = lambda n: fref.load_case(os.path.join(GOLDEN, f"flow_{n}.npz"))
    assert load("f64_py")["u"].dtype == np.float64 and type(load("f64_py")["dx"]) is float
    assert type(load("f64_np64")["dx"]) is np.float64 and load("f64_np64")["mask"] is None
    assert load("f32_py")["strain_rate"].dtype == np.float32 and type(load("f32_py")["dx"]) is float
    assert load("f32_np64")["strain_rate"].dtype == np.float32 and type(load("f32_np64")["dx"]) is np.float64
    # the two float32 division rules differ somewhere, or the fixtures could not tell them apart
    a, b = load("f32_py"), load("f32_np64")
    weak = fref.compute_strain_rate(b["u"], b["v"], b["w"], float(b["dx"]), float(b["dy"]), float(b["dz"]), b["mask"])
    assert not np.array_equal(weak, b["strain_rate"])
    assert a["dx"] != a["dy"] != a["dz"]
    assert not load("all_solid")["mask"].any() and not load("all_solid")["strain_rate"].any()
    n = load("naninf")
    assert np.isnan(n["u"]).sum() == 1 and np.isinf(n["w"]).sum() == 1 and np.isnan(n["strain_rate"]).any()
    assert load("int")["u"].dtype.kind == "i" and load("int")["strain_rate"].dtype == np.float64
    assert load("small_222")["u"].shape == (2, 2, 2) and load("small_253")["u"].shape == (2, 5, 3)


def test_short_axis_raises_numpys_error():
    u = np.zeros((3, 1, 4))
    with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
        fref.compute_strain_rate(u, u, u, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
        np.gradient(u, 1.0, 1.0, 1.0)
