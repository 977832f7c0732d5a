"""The CPU oracle of the variational cleaning (tests/_variational_ref.py) against the fixtures that
tests/golden/make_variational_golden.py recorded from the reference (no device needed).

The CSR form repeats the reference's scipy operations, so it must reproduce the reference's outputs
and iteration count bit for bit; the stencil form is the ordering the fixtures' ``order_gap`` was
measured with.
"""
import glob
import os

import numpy as np
import pytest

import _variational_ref as vref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "var_*.npz")))


def load(case):
    g = np.load(os.path.join(GOLDEN, f"var_{case}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def test_the_fixtures_are_there():
    assert CASES == ["g12", "g12_l200", "g20", "iso", "thin"]


@pytest.mark.parametrize("case", CASES)
def test_csr_form_is_the_reference_bit_for_bit(case):
    g = load(case)
    sp = (float(g["dx"]), float(g["dy"]), float(g["dz"]))
    out, itn, info = vref.solve(g["u"], g["v"], g["w"], g["mask"], *sp, lambda_reg=float(g["lambda_reg"]))
    assert (itn, info) == (int(g["itn"]), int(g["info"]))
    for name, a in zip("uvw", out):
        assert np.array_equal(a, g[f"{name}_c"]), name


@pytest.mark.parametrize("case", CASES)
def test_stencil_form_stops_with_the_reference_within_the_recorded_gap(case):
    g = load(case)
    sp = (float(g["dx"]), float(g["dy"]), float(g["dz"]))
    out, itn, info = vref.solve(g["u"], g["v"], g["w"], g["mask"], *sp, lambda_reg=float(g["lambda_reg"]),
                                form="stencil")
    assert (itn, info) == (int(g["itn"]), int(g["info"]))
    gap = vref.order_gap([g["u_c"], g["v_c"], g["w_c"]], out)
    # the same computation as the generator's; only the two norms (BLAS, threaded for vectors
    # this long) may round differently
    assert abs(gap - float(g["order_gap"])) <= 1e-12 * float(g["order_gap"])


@pytest.mark.parametrize("case", CASES)
def test_operator_forms_against_the_recorded_product(case):
    g = load(case)
    mask = g["mask"]
    sp = (float(g["dx"]), float(g["dy"]), float(g["dz"]))
    lam = float(g["lambda_reg"])
    x = [g["ax_xu"], g["ax_xv"], g["ax_xw"]]
    y = [g["ax_yu"], g["ax_yv"], g["ax_yw"]]
    A = vref.csr_system(mask, *sp, lam)
    got = A @ np.concatenate([a[mask] for a in x])
    assert np.array_equal(got, np.concatenate([a[mask] for a in y]))
    # both forms within 16 roundings of the extended-precision product, componentwise
    _, ye, _, ymag = vref.exact_products(x, mask, *sp, lam)
    st = vref.Stencil(mask, *sp).apply(x, lam)
    for k in range(3):
        bound = 16 * 2.0 ** -53 * ymag[k]
        for form, val in (("csr", y[k]), ("stencil", st[k])):
            err = np.abs(val.astype(np.longdouble) - ye[k])
            assert np.all(err[mask] <= bound[mask]), (form, float(np.max(err[mask] / bound[mask])))
        assert np.all(st[k][~mask] == 0.0)


def test_identity_row_of_the_enclosed_voxel():
    g = load("iso")
    mask = g["mask"]
    nz, ny, nx = mask.shape
    c = (nz // 2, ny // 2, nx // 2)
    assert mask[c] and not mask[c[0] - 1, c[1], c[2]] and not mask[c[0], c[1], c[2] + 1]
    A = vref.csr_system(mask, 1.0, 1.25, 0.8, 1e3)
    n = int(mask.sum())
    row = int(np.cumsum(mask.ravel())[np.ravel_multi_index(c, mask.shape)] - 1)
    for k in range(3):
        r = A.getrow(k * n + row).toarray().ravel()
        e = np.zeros(3 * n)
        e[k * n + row] = 1.0
        assert np.array_equal(r, e)


@pytest.mark.parametrize("maxiter", [1, 2, 5, 17])
def test_truncated_forms_agree(maxiter):
    g = load("g12")
    sp = (float(g["dx"]), float(g["dy"]), float(g["dz"]))
    a, itn_a, info_a = vref.solve(g["u"], g["v"], g["w"], g["mask"], *sp, maxiter=maxiter)
    b, itn_b, info_b = vref.solve(g["u"], g["v"], g["w"], g["mask"], *sp, maxiter=maxiter, form="stencil")
    assert (itn_a, info_a) == (itn_b, info_b) == (maxiter, maxiter)
    assert vref.order_gap(a, b) <= 64 * 2.0 ** -52
