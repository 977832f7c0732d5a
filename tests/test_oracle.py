"""The oracle (oracle/cpu_ref.py) pinned against the reference's own outputs.

Golden vectors come from importing the reference interpolator.py
(tests/golden/make_golden.py).  IDW/Sibson with p=2 are required bit-exact;
pow/exp paths and tied inputs are normwise (<= 1e-10).
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests._util import clean_fixture, clean_spacings, load, names, normwise


def _bit_exact_expected(g):
    return int(g.get("tied", 0)) == 0 and str(g["method"]) == "idw" and float(g["power"]) in (2.0, 1.0, 0.5, -1.0)


@pytest.mark.parametrize("name", names(("idw", "sibson", "edge")))
def test_oracle_matches_reference(name):
    g = load(name)
    U, V, W = cpu_ref.interp_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"],
                                  method=str(g["method"]), k=int(g["k"]), power=float(g["power"]))
    for a, b in ((U, g["U"]), (V, g["V"]), (W, g["W"])):
        if _bit_exact_expected(g) or str(g["method"]) == "sibson" and not int(g.get("tied", 0)):
            # Sibson uses np.exp on the same machine class; exact here, normwise elsewhere.
            assert normwise(a, b) <= 1e-13
        if _bit_exact_expected(g):
            assert np.array_equal(a, b, equal_nan=True)
        assert normwise(a, b) <= 1e-10


def test_oracle_masked_pipeline():
    g = load("masked_spherepack_idw")
    U, V, W = cpu_ref.interp_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"], "idw", 8, 2.0)
    assert normwise(U, g["U_raw"]) <= 1e-12
    U, V, W = cpu_ref.nan_fill_and_mask(U, V, W, g["mask"])
    for a, b in ((U, g["U"]), (V, g["V"]), (W, g["W"])):
        assert normwise(a, b) <= 1e-12


@pytest.mark.parametrize("k", [1, 3, 7, 8, 9, 16, 30, 50, 64, 127, 128, 129, 300])
def test_pairwise_sum_matches_numpy(k):
    rng = np.random.default_rng(k)
    A = rng.standard_normal((300, k)) * np.exp(rng.uniform(-30, 30, (300, k)))
    ref = A.sum(axis=1)
    mine = np.array([cpu_ref.pairwise_sum(r) for r in A])
    assert np.array_equal(ref, mine)


def test_bruteforce_matches_kdtree():
    rng = np.random.default_rng(3)
    P = rng.uniform(0, 20, (3000, 3)); Qp = rng.uniform(-2, 22, (2000, 3))
    d1, i1 = cpu_ref.knn_kdtree(P, Qp, 17)
    d2, i2 = cpu_ref.knn_bruteforce(P, Qp, 17)
    assert np.array_equal(d1, d2)
    assert np.array_equal(i1, i2)


def test_parallel_driver_equals_whole_grid():
    g = load("idw_k8_p2")
    U0, V0, W0 = cpu_ref.interp_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"], "idw", 8, 2.0)
    U1, V1, W1 = cpu_ref.interp_grid_parallel(g["points"], g["values"], g["ax"], g["ay"], g["az"], "idw", 8, 2.0, n_jobs=2)
    assert np.array_equal(U0, U1) and np.array_equal(V0, V1) and np.array_equal(W0, W1)


def _rbf_args(g):
    eps = float(g["epsilon"]) if "epsilon" in g else None
    deg = int(g["degree"]) if "degree" in g else None
    return int(g["k"]), str(g["kernel"]), eps, deg, float(g["smoothing"])


@pytest.mark.parametrize("name", names(("rbf",)))
def test_rbf_oracle_matches_reference(name):
    """The local-RBF restatement (scipy RBFInterpolator(neighbors=k) via numpy's LAPACK gesv)
    against the reference's own outputs.  The Gaussian eps=0.3 systems reach cond 6e8: two
    LAPACK builds differ there by 1.6e-9, so those fixtures get 1e-8 (tests/test_gpu_rbf.py)."""
    g = load(name)
    k, kern, eps, deg, s = _rbf_args(g)
    U, V, W = cpu_ref.rbf_local_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"], k, kern, eps, deg, s)
    tol = 1e-8 if kern == "gaussian" else 1e-11
    for a, b in ((U, g["U"]), (V, g["V"]), (W, g["W"])):
        assert normwise(a, b) <= tol


def test_rbf_monomial_powers_match_scipy():
    from scipy.interpolate._rbfinterp import _monomial_powers

    for deg in range(-1, 4):
        assert np.array_equal(cpu_ref.monomial_powers(deg), _monomial_powers(3, deg))


@pytest.mark.parametrize("kernel", sorted(cpu_ref.RBF_PHI))
def test_rbf_kernel_formulas_match_scipy(kernel):
    """phi(r) against scipy's compiled kernel matrix builder on one small point set."""
    from scipy.interpolate._rbfinterp_pythran import _kernel_matrix

    rng = np.random.default_rng(1)
    y = rng.uniform(0, 3, (20, 3))
    ref = _kernel_matrix(y, kernel)
    r = np.sqrt(((y[:, None, :] - y[None, :, :]) ** 2).sum(-1))
    assert np.allclose(cpu_ref.RBF_PHI[kernel](r), ref, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("name", names(("div_",)))
def test_divergence_oracle_matches_reference(name):
    """physics.compute_consistent_divergence golden vectors: bit-exact, same dtype."""
    g = load(name)
    sp = [g[k] if int(g["spacing_np64"]) else float(g[k]) for k in ("dx", "dy", "dz")]
    d = cpu_ref.consistent_divergence(g["u"], g["v"], g["w"], g["mask"], *sp)
    assert d.dtype == g["div"].dtype
    assert np.array_equal(d, g["div"])


def test_nearest_oracle_matches_reference():
    g = load("nearest_small")
    U, V, W = cpu_ref.interp_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"], "nearest")
    for a, b in ((U, g["U"]), (V, g["V"]), (W, g["W"])):
        assert np.array_equal(a, b)


# ------------------------------------------------ pore-mask path + outlier filter (§8(f) rows 2-3)
def _bounds(g, key):
    b = g[key]
    if int(g[key + "_int"]):
        b = b.astype(int)
    return tuple(tuple(v.tolist()) for v in b)


@pytest.mark.parametrize("name", names(("mask_sample_",)))
def test_oracle_sample_mask_matches_reference(name):
    g = load(name)
    Z, Y, X = np.meshgrid(g["az"], g["ay"], g["ax"], indexing="ij")
    assert np.array_equal(cpu_ref.sample_mask_nearest(g["raw"], _bounds(g, "raw_bounds"), X, Y, Z), g["mask"])


@pytest.mark.parametrize("name", names(("boundary_",)))
def test_oracle_boundary_particles_match_reference(name):
    g = load(name)
    got = cpu_ref.boundary_particles(g["mask"], _bounds(g, "bounds"), int(g["step"]), int(g["thickness"]))
    for a, e in zip(got, (g["bx"], g["by"], g["bz"])):
        assert a.dtype == e.dtype and np.array_equal(a, e)


@pytest.mark.parametrize("name", names(("filter_",)))
def test_oracle_outlier_filter_matches_reference(name):
    g = load(name)
    keep, radius = cpu_ref.outlier_filter(g["points"], g["values"], int(g["k"]), float(g["threshold"]))
    assert np.array_equal(keep, g["keep"])
    assert f"= {radius:.4f}\n" in str(g["stdout"])


def test_oracle_rgi_nearest_tie_and_bounds():
    g = np.array([0.0, 1.0, 2.0, 3.0])
    x = np.array([-0.1, 0.0, 0.5, 0.5000001, 1.5, 2.9, 3.0, 3.1])
    assert cpu_ref.rgi_nearest_index(g, x).tolist() == [-1, 0, 0, 1, 1, 3, 3, -1]
    assert cpu_ref.rgi_nearest_index(g[::-1], x).tolist() == [-1, 3, 3, 2, 2, 0, 0, -1]
    assert cpu_ref.rgi_nearest_index(np.array([2.0]), np.array([2.0, 2.5])).tolist() == [0, -1]


def test_idw_radius_oracle_matches_bruteforce():
    """The fixed-radius IDW restatement (an extension; parity unpinned) against a brute-force
    evaluation of its definition: d2 <= r*r, w = 1/(d**p + 1e-10), sum(w v)/sum(w), NaN if empty."""
    rng = np.random.default_rng(5)
    P = rng.uniform(0, 10, (500, 3))
    Q = rng.standard_normal((500, 3))
    q = rng.uniform(0, 10, (300, 3))
    for r, p in ((1.0, 2.0), (2.5, 1.5), (0.3, 2.0)):
        got = cpu_ref.idw_radius_points(P, Q, q, r, power=p)
        for i in range(len(q)):
            dd = q[i] - P
            d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            sel = d2 <= r * r
            if not sel.any():
                assert np.isnan(got[i]).all()
                continue
            w = 1.0 / (np.sqrt(d2[sel]) ** p + 1e-10)
            np.testing.assert_allclose(got[i], (w[:, None] * Q[sel]).sum(0) / w.sum(), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name", names(("linear_",)))
def test_linear_oracle_matches_reference(name):
    """method='linear' restatement (Delaunay.find_simplex + interpnd arithmetic) against the
    reference interpolate_field fixtures, bit for bit."""
    from oracle import cpu_ref

    g = load(name)
    out = cpu_ref.linear_grid(g["points"], g["values"], g["ax"], g["ay"], g["az"])
    for a, c in zip(out, "UVW"):
        assert np.array_equal(a, g[c])


# ---- divergence cleaning oracle (cpu_ref.clean_projection) against the clean_* fixtures ----
CLEAN_CASES = ["g12", "g20", "g32", "thin", "iso"]


@pytest.mark.parametrize("name", CLEAN_CASES)
def test_clean_oracle_correction_bit_identical(name):
    g = clean_fixture(name)
    out = cpu_ref.consistent_correction(g["u"], g["v"], g["w"], g["phi"], g["mask"], *clean_spacings(g))
    for a, c in zip(out, "uvw"):
        assert a.tobytes() == g["corr_" + c].tobytes(), c


@pytest.mark.parametrize("name", CLEAN_CASES)
def test_clean_oracle_laplacian_componentwise_bound(name):
    """Both forms of the oracle's Laplacian against the reference's CSR product, under the bound
    the GPU stencil is held to (tests/test_gpu_clean.py): 16 * 2**-53 * (|A| |x|)."""
    g = clean_fixture(name)
    m = g["mask"]
    bound = 16.0 * 2.0 ** -53 * g["lap_abs"][m]
    A = cpu_ref.masked_laplacian(m, *clean_spacings(g))
    op = cpu_ref.masked_laplacian_operator(m, *clean_spacings(g))
    assert A.shape == op.shape == (int(m.sum()),) * 2
    assert abs(A - A.T).max() == 0
    for y in (A @ g["lap_x"][m], op.matvec(g["lap_x"][m])):
        assert (np.abs(y - g["lap_y"][m]) <= bound).all()
    if name == "iso":  # the enclosed fluid voxel is a zero row
        assert (np.diff(A.indptr) == 0).sum() >= 1


@pytest.mark.parametrize("its", [1, 3])
@pytest.mark.parametrize("name", ["g12", "thin", "iso"])
def test_clean_oracle_within_the_fixture_order_gap(name, its):
    """The oracle's CSR run against the reference's: same istop per solve, fields and mean |div|
    within 10 x the fixture's own order gap.  g20 and g32 take tens of seconds on a CPU and are not
    in the suite; run once by hand (ratio to the gap, fields / mean |div|):
      g20 its=1 0.000 / 0.000, its=3 0.000 / 0.000, istop [1, 1, 1], itn [2550, 2606, 2653]
      g32 its=1 0.000 / 0.000, its=3 0.000 / 0.000, istop [7, 7, 7]
    (the oracle's CSR matrix holds the reference's entries in the reference's order, so the runs
    coincide to the bit)."""
    g = clean_fixture(name)
    (u, v, w), info = cpu_ref.clean_projection(g["u"], g["v"], g["w"], g["mask"], *clean_spacings(g), iterations=its)
    ref = np.stack([g[f"{c}_it{its}"] for c in "uvw"])
    k = 0 if its == 1 else 1
    gap_f, gap_d = float(g["order_gap_fields"][k]), float(g["order_gap_div"][k])
    diff_f = float(np.linalg.norm((np.stack([u, v, w]) - ref).ravel()) / np.linalg.norm(ref.ravel()))
    mdiv = float(g[f"mean_abs_div_it{its}"])
    diff_d = abs(info["mean_abs_div_final"] - mdiv) / mdiv
    print(f"clean oracle {name} iterations={its}: fields {diff_f:.3e} / gap {gap_f:.3e}; mean|div| {diff_d:.3e} / "
          f"gap {gap_d:.3e}; istop {info['istop']} itn {info['itn']} (reference {g[f'itn_it{its}'].tolist()})")
    assert info["istop"] == g[f"istop_it{its}"].tolist()
    assert info["n_outer"] == its and not info["nan_stop"] and info["n_fluid"] == int(g["mask"].sum())
    assert diff_f <= 10.0 * gap_f
    assert diff_d <= 10.0 * gap_d


def test_clean_oracle_order_gap_and_edges():
    """clean_order_gap restates the fixture's own gap definition; iterations=0 returns copies."""
    g = clean_fixture("iso")
    args = (g["u"], g["v"], g["w"], g["mask"], *clean_spacings(g))
    gap_f, gap_d, agree, (f_csr, i_csr), (f_free, i_free) = cpu_ref.clean_order_gap(*args, iterations=1)
    assert agree and i_csr["istop"] == g["istop_it1"].tolist()
    # the fixture's gap came from the same two orderings of the reference; same order of magnitude
    assert 0.1 * float(g["order_gap_fields"][0]) <= gap_f <= 10.0 * float(g["order_gap_fields"][0])
    assert gap_d <= 10.0 * float(g["order_gap_div"][0])
    (u, v, w), info = cpu_ref.clean_projection(*args, iterations=0)
    for a, c in zip((u, v, w), "uvw"):
        assert a.tobytes() == g[c].tobytes() and a is not g[c]
    assert info["n_outer"] == 0 and info["istop"] == [] and info["mean_abs_div"] == [info["mean_abs_div_final"]]
    with pytest.raises(ValueError):
        cpu_ref.clean_projection(g["u"], g["v"], g["w"], np.zeros_like(g["mask"]), *clean_spacings(g))
