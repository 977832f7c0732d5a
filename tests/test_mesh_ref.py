"""The numpy restatement of the mesh interface drag (tests/_mesh_ref.py) against the reference's
fixtures (tests/golden/mesh_*.npz, spline_*.npz): no device needed.

The float64 chain repeats the reference's operations, so here it reproduces every fixture bit for
bit; the assertion allows the fixture's own ``gap`` (its distance from the long-double chain), so a
numpy with another pairwise split still passes.  The long-double chain is held to the stored
``exact`` values, which is what the GPU tests measure against.
"""
import os

import numpy as np
import pytest

import _mesh_ref as mref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MESH_CASES = ["two", "odd", "nop", "vol", "edge", "single", "big", "zero", "f32"]
SPLINE_CASES = ["a", "line", "ties"]


def load_mesh(name):
    g = np.load(os.path.join(GOLDEN, f"mesh_{name}.npz"), allow_pickle=False)
    labels = [x.item() for x in g["labels"]]
    meshes = {lab: (g[f"verts_{i}"], g[f"faces_{i}"]) for i, lab in enumerate(labels)}
    fields = [g["u"], g["v"], g["w"], g["pressure"] if "pressure" in g.files else None]
    bg = g["background"] if "background" in g.files else None
    return g, meshes, fields, bg


@pytest.mark.parametrize("name", MESH_CASES)
def test_float64_restatement_reproduces_the_reference(name):
    g, meshes, fields, bg = load_mesh(name)
    res = mref.integrate(meshes, *fields, float(g["viscosity"]), *g["spacing"], background=bg)
    assert list(res) == [x.item() for x in g["out_labels"]]
    assert tuple(g["keys"][:21]) == mref.KEYS
    for i, lab in enumerate(res):
        sums, scale = res[lab]
        ref = g["values"][i, :21]
        assert np.array_equal(np.isnan(sums), np.isnan(ref)), (lab, sums, ref)
        ok = ~np.isnan(ref)
        assert np.all(np.abs(sums[ok] - ref[ok]) <= g["gap"][i][ok]), (lab, sums - ref, g["gap"][i])
        # the fixture's scale is the long-double chain's (float32 fields: the reference's samples are float32)
        assert np.allclose(scale, g["scale"][i], rtol=1e-6 if fields[0].dtype == np.float32 else 1e-12, atol=0)
        r = dict(zip(g["keys"], g["values"][i]))
        for c in "xyz":  # the combined keys are the reference's
            if not np.isnan(r[f"F{c}"]):
                assert r[f"F{c}"] == r[f"F{c}_v"] + r[f"F{c}_p"]
        if float(g["volume"]):
            assert r["Mx"] == r["Fx"] / float(g["volume"])
        else:
            assert "Mx" not in r


def test_the_cases_reach_their_edges():
    g, meshes, _, _ = load_mesh("big")
    assert len(meshes[1][1]) == 1300 and 1300 % 256 and 1300 % 64
    g, meshes, _, _ = load_mesh("single")
    assert [len(f) for _, f in meshes.values()] == [1, 0, 40] and g["out_labels"].tolist() == [1, 4]
    g, meshes, _, _ = load_mesh("edge")
    v = meshes[1][0]
    assert v.dtype == np.float32 and np.array_equal(v.min(0), [0, 0, 0]) and np.array_equal(v.max(0), [8, 10, 12])
    g, _, _, _ = load_mesh("zero")
    nan = np.isnan(g["values"][0, :21])
    assert nan.any() and not nan[12] and not nan[9:12].any() and np.isfinite(g["values"][0, 19:21]).all()
    g, _, _, _ = load_mesh("two")  # the background mask splits both labels' triangles
    assert np.all(g["values"][:, 19] > 0) and np.all(g["values"][:, 20] > 0)
    g, _, fields, _ = load_mesh("f32")
    assert fields[0].dtype == np.float32
    assert "pressure" not in np.load(os.path.join(GOLDEN, "mesh_nop.npz")).files


@pytest.mark.parametrize("name", MESH_CASES)
def test_long_double_chain_is_the_stored_exact(name):
    g, meshes, fields, bg = load_mesh(name)
    res = mref.integrate(meshes, *fields, float(g["viscosity"]), *g["spacing"], background=bg, ft=mref.LD)
    for i, lab in enumerate(res):
        exact = g["exact_hi"][i].astype(mref.LD) + g["exact_lo"][i].astype(mref.LD)
        ok = ~np.isnan(g["exact_hi"][i])
        assert np.array_equal(np.isnan(res[lab][0]), ~ok)
        assert np.all(np.abs(res[lab][0][ok] - exact[ok]) <= 2.0 ** -60 * g["scale"][i][ok])


@pytest.mark.parametrize("name", SPLINE_CASES)
def test_spline_fixtures(name):
    """The long-double prefilter and samplers stand within rounding of scipy's: the reflect start, the
    padded sampling and the order-0 rule are the right restatement (a mirror start would stand 1e-6
    off, a clamped coordinate 0.2)."""
    g = np.load(os.path.join(GOLDEN, f"spline_{name}.npz"), allow_pickle=False)
    c = np.load(os.path.join(GOLDEN, f"spline_{name}_coef.npz"), allow_pickle=False)
    field, pts = g["field"], g["points"]
    coef = mref.prefilter(field)
    assert coef.shape == tuple(n + 24 for n in field.shape) == c["coef"].shape
    cmax = np.abs(c["coef"]).max()
    assert np.abs(coef - c["coef"].astype(mref.LD)).max() <= 64 * mref.EPS * cmax
    assert np.abs((coef - c["coef"].astype(mref.LD)).astype(np.float64) - c["coef_diff"]).max() <= 1e-20
    assert np.abs(mref.sample3(coef, pts) - g["s3"]).max() <= 64 * mref.EPS * cmax
    assert np.abs(mref.sample1(field, pts) - g["s1"]).max() <= 16 * mref.EPS * np.abs(field).max()
    assert np.array_equal(field[mref.index0(field.shape, pts)], g["s0"])
    assert pts.min() >= -0.25 and np.all(pts.max(1) <= np.array(field.shape) - 0.75)
