"""GPU checks of the cubic B-spline prefilter, the order 0 / 1 / 3 sampling and the mesh interface
drag (csrc/ptv_mesh.hip behind ``ptv_spline_prefilter``, ``ptv_map_coordinates`` and
``ptv_mesh_drag``) against the reference's fixtures (tests/golden/mesh_*.npz, spline_*.npz).

The bar.  A GPU value g passes when |g - exact| <= 8 * max(gap, eps * scale), eps = 2^-52: ``exact`` is
the long-double chain of tests/_mesh_ref.py, ``gap`` the reference's (or scipy's) own distance from
it and ``scale`` the sum of |term| (for a sample: max |field| at order 1, max |coefficient| at order
3, times the weight sum 1).  The bar comes from the reference's error and the number format, not
from the code under test; the factor 8 allows a 64-term tensor sum and a block reduction in another
order.  What it exists to catch sits at 1e-7 relative or above (a mirror start 1.3e-6, a clamped
coordinate 0.2, a float64 centroid of float32 vertices 1e-7).  The measured ratios
|g - exact| / max(gap, eps * scale) are printed before each assertion and, with PTV_MESH_PARITY_OUT set
to a path, appended to that file (profiles/mesh_parity.txt is such a run).

Measured on an MI355X (profiles/mesh_parity.txt): every check lies within the bar, the largest
ratios being 2.2 for the coefficients, 1.0 for the order-3 samples and 1.8 for a mesh key.  Plain
float64 recursion and sampling (scipy's own arithmetic) does not get there: it left two keys at 11
times max(gap, eps * scale), where the reference's gap happens to lie under eps * scale, because the
viscous terms amplify the samples' accumulated rounding through u_interface - u_inner.  The device
therefore carries the recursion, the weights, the tensor sums and that difference in
double-double arithmetic and rounds each stored value once (csrc/ptv_mesh.hip).

Shapes are the smallest that reach each edge: 1,300 triangles (six blocks, the last of 20), one
triangle, a label without any, vertices on 0 and n - 1, a zero-area triangle, a singleton axis, a
line of 94 padded samples (two chunks of the x pass), float32 fields.
"""
import os

import numpy as np
import pytest

import _mesh_ref as mref
from test_mesh_ref import MESH_CASES, SPLINE_CASES, load_mesh

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _run(va, name, **kw):
    g, meshes, fields, bg = load_mesh(name)
    volume = float(g["volume"]) or None
    res = va.integrate_mesh_drag(meshes, *fields, float(g["viscosity"]), *g["spacing"], background_mask=bg,
                                 volume=volume, **kw)
    return g, res


def note(line):
    print(line)
    path = os.environ.get("PTV_MESH_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def ratios(got, exact, gap, scale):
    """|g - exact| / max(gap, eps * scale) per entry (0 where both are NaN or the bar and the error are 0)."""
    err = np.abs(np.asarray(got).astype(mref.LD) - exact).astype(np.float64)
    den = np.maximum(gap, mref.EPS * scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / den)


@pytest.mark.parametrize("name", MESH_CASES)
def test_mesh_fixtures_within_the_bar(va, name):
    g, res = _run(va, name)
    assert list(res) == [x.item() for x in g["out_labels"]]
    for i, (lab, r) in enumerate(res.items()):
        assert list(r) == [k.item() for k in g["keys"]]
        got = np.array([r[k] for k in mref.KEYS])
        exact = g["exact_hi"][i].astype(mref.LD) + g["exact_lo"][i].astype(mref.LD)
        nan = np.isnan(g["values"][i, :21])
        assert np.array_equal(np.isnan(got), nan), (lab, got)  # NaN in exactly the reference's keys
        q = ratios(got[~nan], exact[~nan], g["gap"][i][~nan], g["scale"][i][~nan])
        for cls, sel in (("viscous", slice(0, 9)), ("pressure", slice(9, 12)), ("area", [12, 19, 20]),
                         ("phase", slice(13, 19))):
            qq = ratios(got[sel], exact[sel], g["gap"][i][sel], g["scale"][i][sel])
            qq = qq[~np.isnan(qq)]
            note(f"mesh {name} label {lab} {cls}: max |g - exact| / max(gap, eps scale) = "
                 f"{(qq.max() if qq.size else 0.0):.3f}")
        assert np.all(q <= 8.0), (lab, dict(zip(np.array(mref.KEYS)[~nan], q)))
        # Area_water + Area_solid = Area within the bar of Area
        assert abs((r["Area_water"] + r["Area_solid"]) - r["Area"]) <= mref.bar(g["gap"][i][12], g["scale"][i][12])
        for c in "xyz":
            if not np.isnan(r[f"F{c}"]):
                assert r[f"F{c}"] == r[f"F{c}_v"] + r[f"F{c}_p"]
                if g["volume"]:
                    assert r[f"M{c}"] == r[f"F{c}"] / float(g["volume"])
        assert ("Mx" in r) == bool(g["volume"])


def test_triangle_counts_and_the_label_without_triangles(ctx):
    g, meshes, fields, _ = load_mesh("single")
    keep = {lab: m for lab, m in meshes.items() if len(m[1])}
    vt = np.concatenate([m[0] for m in keep.values()])
    base = np.cumsum([0] + [len(m[0]) for m in keep.values()])
    fc = np.concatenate([m[1] + b for m, b in zip(keep.values(), base)])
    off = np.cumsum([0] + [len(m[1]) for m in keep.values()])
    rec, times = ctx.mesh_drag(fields[:3], fields[3], None, vt, fc, off, float(g["viscosity"]), *g["spacing"])
    assert rec["n_tris"].tolist() == [1, 40]
    assert times["ms_prefilter"] > 0 and times["ms_traction"] > 0
    # an empty label in the middle of the table gives zeros and moves nothing else
    off3 = np.array([0, 1, 1, 41])
    rec3, _ = ctx.mesh_drag(None, None, None, vt, fc, off3, float(g["viscosity"]), *g["spacing"], shape=fields[0].shape)
    assert rec3["n_tris"].tolist() == [1, 0, 40] and np.all(rec3["sums"][1] == 0)
    assert np.array_equal(rec3["sums"][[0, 2]], rec["sums"])


def test_zero_area_triangle(va):
    g, res = _run(va, "zero")
    r = res[1]
    nan = {k for k in r if np.isnan(r[k])}
    assert nan == {k.item() for k, v in zip(g["keys"], g["values"][0]) if np.isnan(v)}
    assert {"Fx_v", "Fy_v_tan", "Fz_v_nor", "Fx"} <= nan and not nan & {"Fx_p", "Area", "Area_water", "Area_solid"}
    assert np.isfinite(r["Area"])


def test_two_runs_are_bit_identical(va):
    _, a = _run(va, "big")
    _, b = _run(va, "big")
    assert a.keys() == b.keys()
    for lab in a:
        assert all(np.array_equal(a[lab][k], b[lab][k], equal_nan=True) for k in a[lab])


@pytest.mark.parametrize("name", SPLINE_CASES)
def test_prefilter_and_samples_within_the_bar(ctx, name):
    from ptv_interpolation_amd import sampling

    g = np.load(os.path.join(GOLDEN, f"spline_{name}.npz"), allow_pickle=False)
    c = np.load(os.path.join(GOLDEN, f"spline_{name}_coef.npz"), allow_pickle=False)
    field, pts = g["field"], g["points"]
    cmax, fmax = np.abs(c["coef"]).max(), np.abs(field).max()
    coef = sampling.spline_filter_nearest(field)
    assert coef.shape == c["coef"].shape and coef.dtype == np.float64
    exact = c["coef"].astype(mref.LD) + c["coef_diff"].astype(mref.LD)
    q = ratios(coef, exact, np.abs(c["coef_diff"]).astype(np.float64), cmax)
    note(f"spline {name} coefficients: max |g - exact| / max(gap, eps scale) = {q.max():.3f}")
    assert np.all(q <= 8.0)
    for order, scale in ((3, cmax), (1, fmax)):
        s = sampling.map_coordinates(field, pts, order=order)
        exact = g[f"s{order}"].astype(mref.LD) + g[f"s{order}_diff"].astype(mref.LD)
        q = ratios(s, exact, np.abs(g[f"s{order}_diff"]).astype(np.float64), scale)
        note(f"spline {name} order {order}: max |g - exact| / max(gap, eps scale) = {q.max():.3f}")
        assert np.all(q <= 8.0), order
    assert np.array_equal(sampling.map_coordinates(field, pts, order=0), g["s0"])  # bit for bit
    # the resident coefficients give the same samples without another filter
    again = sampling.map_coordinates(None, pts, order=3, shape=field.shape)
    assert np.array_equal(again, sampling.map_coordinates(field, pts, order=3))
    # float32 input is widened exactly; the trailing shape of the coordinates is kept
    f32 = field.astype(np.float32)
    a = sampling.map_coordinates(f32, pts.reshape(3, 2, -1), order=3)
    assert a.shape == (2, pts.shape[1] // 2) and np.array_equal(a.ravel(), sampling.map_coordinates(f32.astype(np.float64), pts, order=3))


def test_residency_and_the_pieces_agree(ctx, va):
    """The drag's samples are the sampling module's on the same points, and a second call on the
    resident fields and coefficients filters nothing and gives the same bits."""
    from ptv_interpolation_amd import sampling

    g, meshes, fields, bg = load_mesh("two")
    visc, h = float(g["viscosity"]), g["spacing"]
    first = va.integrate_mesh_drag(meshes, *fields, visc, *h, background_mask=bg)
    assert va.integrate_mesh_drag.last_times["ms_prefilter"] > 0
    second = va.integrate_mesh_drag(meshes, *fields, visc, *h, background_mask=bg, resident=True)
    assert va.integrate_mesh_drag.last_times["ms_prefilter"] == 0
    for lab in first:
        assert all(first[lab][k] == second[lab][k] for k in first[lab])
    # per-piece: the device's samples through the restatement's own arithmetic
    class Pieces(mref.ScipySampler):
        def inner(self, k, coords):
            return sampling.map_coordinates(self.f[k], coords, order=3)

        def interface(self, k, coords):
            return sampling.map_coordinates(self.f[k], coords, order=1)

        def pressure(self, coords):
            return sampling.map_coordinates(self.p, coords, order=1)

        def water(self, coords):
            return sampling.map_coordinates(self.bg, coords, order=0) > 0.5

    for i, (lab, (verts, faces)) in enumerate(meshes.items()):
        t, _ = mref.terms(verts, faces, Pieces(*fields, bg), visc, *h)
        sums = t.sum(axis=1)
        got = np.array([first[lab][k] for k in mref.KEYS])
        # the same per-triangle values summed in two orders: 2 gamma(n) of the scale
        assert np.all(np.abs(got - sums) <= 2 * len(faces) * mref.EPS * g["scale"][i]), lab
    with pytest.raises(ValueError):  # reuse must name the resident shape
        ctx.mesh_drag(None, None, None, *meshes[1], [0, len(meshes[1][1])], visc, *h, shape=(3, 3, 3))
