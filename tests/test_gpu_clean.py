"""GPU parity of the projection-method divergence cleaning (csrc/ptv_clean.hip) against the
reference fixtures of tests/golden/make_clean_golden.py.

* ``apply_consistent_correction``: bit-identical (elementwise IEEE arithmetic in numpy's order).
* the masked Laplacian: componentwise ``|y_gpu - y_ref| <= 16 * 2**-53 * (|A| |x|)`` (a row of A
  has at most 7 distinct entries, scipy's CSR product sums 13 stored terms in another order).
* the whole cleaning (``iterations`` 1 and 3): LSQR cannot be bit-exact, its norms are long
  reductions and thousands of Lanczos steps amplify the last bit.  Each fixture stores the gap
  between two CPU orderings of the same run (``order_gap_fields``, ``order_gap_div``); the GPU
  result must lie within 10 x that gap, and stop every solve for the same reason (``istop``).
  The measured ratios are printed (profiles/clean_parity.txt keeps a run's output).
"""
import numpy as np
import pytest

from tests._util import clean_fixture as fixture, clean_spacings as spacings

pytestmark = pytest.mark.gpu

CASES = ["g12", "g20", "g32", "thin", "iso"]
FACTOR = 10.0


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


_runs = {}


def cleaned(ctx, name, its):
    """One GPU cleaning per (case, iterations), shared by the tests below."""
    if (name, its) not in _runs:
        g = fixture(name)
        _runs[name, its] = ctx.clean_divergence(g["u"], g["v"], g["w"], g["mask"], *spacings(g), iterations=its)
    return _runs[name, its]


@pytest.mark.parametrize("name", CASES)
def test_correction_bit_identical(ctx, name):
    g = fixture(name)
    phi_grid = np.zeros_like(g["u"])
    phi_grid[g["mask"]] = g["phi"]
    out = ctx.apply_correction(g["u"], g["v"], g["w"], phi_grid, g["mask"], *spacings(g))
    for a, c in zip(out, "uvw"):
        assert np.array_equal(a, g["corr_" + c]), c
        assert not np.signbit(a[~g["mask"]]).any() and (a[~g["mask"]] == 0).all()


def test_correction_python_entry_point(ctx):
    from ptv_interpolation_amd import physics

    g = fixture("thin")
    out = physics.apply_consistent_correction(g["u"], g["v"], g["w"], g["phi"], g["mask"], *spacings(g))
    for a, c in zip(out, "uvw"):
        assert np.array_equal(a, g["corr_" + c])


@pytest.mark.parametrize("name", CASES)
def test_laplacian_componentwise_bound(ctx, name):
    g = fixture(name)
    y = ctx.laplacian_apply(g["lap_x"], g["mask"], *spacings(g))
    bound = 16.0 * 2.0 ** -53 * g["lap_abs"]
    err = np.abs(y - g["lap_y"])
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    print(f"clean laplacian {name}: max |err| / bound = {worst:.3f}")
    assert (err <= bound).all()
    assert (y[~g["mask"]] == 0).all()


@pytest.mark.parametrize("its", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_full_cleaning_within_the_order_gap(ctx, name, its):
    g = fixture(name)
    (u, v, w), st = cleaned(ctx, name, its)
    ref = np.stack([g[f"{c}_it{its}"] for c in "uvw"])
    got = np.stack([u, v, w])
    k = 0 if its == 1 else 1
    gap_f, gap_d = float(g["order_gap_fields"][k]), float(g["order_gap_div"][k])
    diff_f = float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))
    mdiv_ref = float(g[f"mean_abs_div_it{its}"])
    diff_d = abs(st["mean_abs_div_final"] - mdiv_ref) / mdiv_ref
    print(f"clean parity {name} iterations={its}: fields {diff_f:.3e} / gap {gap_f:.3e} = {diff_f / gap_f:.3f}; "
          f"mean|div| {diff_d:.3e} / gap {gap_d:.3e} = {diff_d / gap_d:.3f}; "
          f"istop {st['istop']} itn {st['itn']} (reference itn {g[f'itn_it{its}'].tolist()})")
    assert st["n_outer"] == its and not st["nan_stop"]
    assert st["istop"] == g[f"istop_it{its}"].tolist()
    assert all(0 < n <= 3000 for n in st["itn"])
    assert st["n_fluid"] == int(g["mask"].sum())
    for a in (u, v, w):
        assert (a[~g["mask"]] == 0).all()
    assert diff_f <= FACTOR * gap_f
    assert diff_d <= FACTOR * gap_d


@pytest.mark.parametrize("name", ["g12", "thin"])
def test_two_calls_give_identical_bits(ctx, name):
    g = fixture(name)
    (u, v, w), st = cleaned(ctx, name, 3)
    (u2, v2, w2), st2 = ctx.clean_divergence(g["u"], g["v"], g["w"], g["mask"], *spacings(g), iterations=3)
    for a, b in ((u, u2), (v, v2), (w, w2)):
        assert a.tobytes() == b.tobytes()
    for key in ("istop", "itn", "rnorm", "mean_abs_div", "mean_abs_div_final", "flux_initial", "flux_final"):
        assert st[key] == st2[key], key


def test_device_pointer_call_matches_host_call(ctx):
    import torch

    g = fixture("g12")
    (u, v, w), st = cleaned(ctx, "g12", 3)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.array(g[c])).to(dev) for c in "uvw"]
    m = torch.from_numpy(g["mask"].view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    nz, ny, nx = g["u"].shape
    ptrs = [a.data_ptr() for a in t]
    st2 = ctx.clean_divergence_dev(nx, ny, nz, ptrs, m.data_ptr(), ptrs, *spacings(g), iterations=3)  # in place
    for a, b in zip(t, (u, v, w)):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    assert st2["itn"] == st["itn"] and st2["istop"] == st["istop"]


def test_iterations_zero_and_all_solid(ctx):
    g = fixture("thin")
    (u, v, w), st = ctx.clean_divergence(g["u"], g["v"], g["w"], g["mask"], *spacings(g), iterations=0)
    assert st["n_outer"] == 0 and st["istop"] == []
    for a, c in zip((u, v, w), "uvw"):
        assert np.array_equal(a, g[c])  # u.copy() (physics.py:154): nothing is zeroed without a correction
    assert st["mean_abs_div"][0] == st["mean_abs_div_final"]
    with pytest.raises(ValueError):
        ctx.clean_divergence(g["u"], g["v"], g["w"], np.zeros_like(g["mask"]), *spacings(g))


def test_report_has_the_references_line_structure(ctx, capsys):
    from ptv_interpolation_amd import physics

    g = fixture("thin")
    n = int(g["mask"].sum())
    out = physics.clean_divergence(g["u"], g["v"], g["w"], g["mask"], *spacings(g), iterations=3)
    text = capsys.readouterr().out
    (u, v, w), _ = cleaned(ctx, "thin", 3)
    for a, b in zip(out, (u, v, w)):
        assert a.tobytes() == b.tobytes()
    expect = ["Starting Iterative Divergence Cleaning (3 iterations)...", "  [Initial] Net X-Flux (mid-plane): "]
    for i in range(3):
        expect += ["", f"--- Iteration {i+1}/3 ---", "  Current Mean Abs Div: ", f"  Solving Poisson (A: {n}x{n})..."]
    expect += ["", "=" * 40, "DIVERGENCE CLEANING COMPLETE", "Initial Mean Abs Div: ", "Final Mean Abs Div:   ",
               "Total Reduction:      ", "  [Final] Net X-Flux (mid-plane): ", "=" * 40, ""]
    lines = text.split("\n")
    assert lines[-1] == ""  # the last print's newline
    lines = lines[:-1]
    assert len(lines) == len(expect), text
    for got, want in zip(lines, expect):
        if want == "" or want.startswith(("=", "---", "DIVERGENCE", "Starting", "  Solving")):
            assert got == want, (got, want)
        else:
            assert got.startswith(want), (got, want)
            float(got[len(want):].rstrip("x"))  # a number follows the prefix
    # the reported numbers are the reference's to the printed digits' worth of the order gap
    flux0 = float(np.sum(g["u"][:, :, g["u"].shape[2] // 2]) * float(g["dy"]) * float(g["dz"]))
    assert lines[1] == f"  [Initial] Net X-Flux (mid-plane): {flux0:.4e}"
