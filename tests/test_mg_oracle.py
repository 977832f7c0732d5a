"""The multigrid preconditioner's numpy restatement (tests/_mg_ref.py) on the CPU: its coarse
operators are the exact Galerkin products, M is symmetric with A's sign, and scipy's cg with this M
needs fewer iterations than scipy's plain cg on the anchored pressure system."""
import numpy as np
import pytest
from scipy.sparse.linalg import cg

import _mg_ref as mg
import _pressure_ref as pref
from _variational_ref import single_threaded_blas

_h = {}


def hierarchy(name):
    if name not in _h:
        mask, d, sp = mg.case(name)
        _h[name] = mg.Hierarchy(mask, d, *sp)
    return _h[name]


@pytest.mark.parametrize("name", mg.CASES + ["half_unit"])
def test_coarse_operators_are_galerkin_products(name):
    """Level l + 1 equals P^T A_l P built from explicit sparse matrices: exactly where every weight is
    an integer (unit spacings), otherwise to the rounding of sums of at most eight equal-signed terms
    taken in two orders (8 * 2**-53 relative per level, accumulated over the levels)."""
    H = hierarchy(name)
    mask, d, sp = mg.case(name)
    # level 0 is section 21's matrix on the active voxels
    act = (mask & ~d).ravel()
    A0 = mg.level_matrix(H.levels[0])
    ref = pref.laplacian_matrix(mask, *sp, dirichlet=d, symmetric=True)
    fluid_act = (~d[mask])
    if act.any():  # the diagonals are sums of the same at most six terms in two orders
        ref = ref[fluid_act][:, fluid_act]
        assert abs(A0[act][:, act] - ref).max() <= 6 * 2.0 ** -53 * abs(ref).max()
    assert A0[~act].nnz == 0 and A0[:, ~act].nnz == 0
    exact = sp == (1.0, 1.0, 1.0)
    for l in range(len(H.levels) - 1):
        P = mg.aggregation_matrix(H.levels[l].shape)
        G = (P.T @ mg.level_matrix(H.levels[l]) @ P).tocsr()
        C = mg.level_matrix(H.levels[l + 1])
        diff = abs(G - C).max() if G.nnz or C.nnz else 0.0
        scale = abs(C).max() if C.nnz else 1.0
        print(f"{name} level {l + 1}: cells {C.shape[0]} max |P^T A P - stored| / max |stored| = {diff / scale:.2e}")
        assert diff == 0.0 if exact else diff <= 8 * (l + 1) * 2.0 ** -53 * scale
    assert H.cells()[-1] <= 8 or len(H.levels) == mg.MAX_LEVELS


# Operations on one cell's path through a cycle, each rounding once: a sweep is 6 * 3 + 4 = 22, the
# residual 20, the restriction 8, the prolongation 1; a level runs 2 * nu = 4 sweeps (117 in all), the
# coarsest 16 sweeps (352).  Damped Jacobi does not amplify (|I - omega D^-1 A| <= 1 in the D norm), so
# the error of M r is at most that many units of 2**-53 times |M r|.
def _ops(H):
    return 117 * (len(H.levels) - 1) + 352


@pytest.mark.parametrize("name", ["odd", "g20", "half", "pockets", "line5"])
def test_m_is_symmetric_with_the_sign_of_a(name):
    H = hierarchy(name)
    mask, d, _ = mg.case(name)
    act = mask & ~d
    rng = np.random.default_rng(5)
    r1, r2 = (np.where(act, rng.standard_normal(mask.shape), 0.0) for _ in range(2))
    z1, z2 = H.apply(r1), H.apply(r2)
    assert not z1[~act].any()
    lhs, rhs = float(np.vdot(r1, z2)), float(np.vdot(r2, z1))
    norm = np.linalg.norm
    bound = _ops(H) * 2.0 ** -53 * (norm(r1) * norm(z2) + norm(r2) * norm(z1))
    print(f"{name}: |r1.Mr2 - r2.Mr1| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert np.vdot(r1, z1) < 0 and np.vdot(r2, z2) < 0  # A is negative definite and so is M


def test_zero_diagonal_cells_stay_out():
    H = hierarchy("pockets")
    mask, d, _ = mg.case("pockets")
    r = np.random.default_rng(2).standard_normal(mask.shape)
    z = H.apply(r)
    assert z[1, 1, 1] == 0.0 and not H.levels[0].inside[1, 1, 1]  # the isolated voxel
    assert z[1:3, 4:7, 5:9].any()  # the pocket is smoothed like any other part
    assert not hierarchy("plane").apply(np.ones(mg.case("plane")[0].shape)).any()
    assert hierarchy("plane").active() == [0] * len(hierarchy("plane").levels)


@pytest.mark.parametrize("name", ["g12", "g20", "odd"])
def test_fewer_iterations_than_plain_cg(name):
    mask, d, sp, rhs = mg._golden(name)
    A = pref.laplacian_matrix(mask, *sp, dirichlet=d, symmetric=True)
    b = rhs[mask].copy()
    b[d[mask]] = 0.0
    count = [0]

    def callback(_x):
        count[0] += 1

    with single_threaded_blas():
        x, info = cg(A, b, rtol=1e-10, atol=0.0, maxiter=3000, callback=callback)
    p, itn, pinfo = mg.pcg(rhs, mask, d, *sp)
    res = np.linalg.norm(b - A @ p[mask]) / np.linalg.norm(b)
    print(f"{name}: plain cg {count[0]} iterations (info {info}), multigrid pcg {itn} (info {pinfo}), "
          f"true relative residual {res:.2e}")
    assert info == 0 and pinfo == 0
    assert itn < count[0]
    assert res < 1e-9
