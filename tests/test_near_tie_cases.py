"""CPU preconditions of tests/test_gpu_near_ties.py: the properties of the near-tie cases
(tests/_near_ties.py) that the GPU comparisons rely on, for every (case, k) they run.

(a) exact ties: the voxels with an exact d2 tie on differing values among the first k + 1, the only
    ones a GPU comparison leaves out, are at most 5 % (``NT.EXCLUDED_CAP``);
(b) near ties present: at least 90 % of the voxels have two distinct d2 of one key truncation next to
    each other inside the list, and for odd k at least 50 % have them as k-th and (k+1)-th, so a
    search that trusts the keys' order or set is wrong almost everywhere;
(c) oracle agreement: cKDTree's neighbour indices equal the brute-force ones outside (a).

d2 is ``(dx*dx + dy*dy) + dz*dz`` by brute force, ascending, ties by lower index; the truncation is
to 52 - B mantissa bits with B as launch_knn computes it (12 for these 3000 particles).
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _near_ties as NT
from tests._util import d2_ties_points, normwise

TOL_RBF = 1e-10  # tests/test_gpu_rbf.py


def test_key_bits():
    assert [NT.key_bits(n) for n in (1, 2, 3, 2048, 2049, 3000, 4096, 4097)] == [1, 1, 2, 11, 12, 12, 12, 13]
    a = np.array([1.0, 1.0 + 2.0 ** -41, 1.0 + 2.0 ** -40])
    assert NT.trunc(a, NT.N)[0] == NT.trunc(a, NT.N)[1] != NT.trunc(a, NT.N)[2]


def test_bruteforce_selection_equals_the_full_stable_sort():
    """knn_bruteforce selects before it sorts; on an integer lattice (ties at almost every rank, the
    k-th included) it returns the first k of the full stable argsort, and d2 with ``squared``."""
    g = np.arange(6.0)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([P[::7] + 0.5, P[::11]])
    dd = q[:, None, :] - P[None, :, :]
    d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
    full = np.argsort(d2, axis=1, kind="stable")
    for k in (1, 6, 7, 27, len(P)):
        d, i = cpu_ref.knn_bruteforce(P, q, k, squared=True)
        assert np.array_equal(i, full[:, :k])
        assert np.array_equal(d, np.take_along_axis(d2, full[:, :k], axis=1))
        assert np.array_equal(cpu_ref.knn_bruteforce(P, q, k)[0], np.sqrt(d))


def test_d2_ties_points_by_hand():
    """Particles on the x axis seen from the origin; d2 = 1, 1, 4, 4, 9, 16, 16, 16, 25 ..."""
    x = np.array([1.0, -1.0, 2.0, -2.0, 3.0, 4.0, -4.0, 4.0] + [5.0 + j for j in range(12)])
    P = np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)
    V = np.arange(len(x), dtype=np.float64)[:, None] * np.ones((1, 3))
    V[1] = V[0]  # the d2 = 1 pair carries one value
    q = np.zeros((1, 3))
    got = {k: tuple(bool(a[0]) for a in d2_ties_points(P, V, q, k)) for k in (1, 2, 3, 4, 5, 6, 7)}
    assert got[1] == (True, False)   # boundary tie 1 | 1, one value
    assert got[2] == (True, False)   # in-list tie on one value
    assert got[3] == (True, True)    # boundary tie 4 | 4 on differing values
    assert got[4] == (True, True)    # that tie inside the list
    assert got[5] == (True, True)
    assert got[6] == (True, True)    # 16 | 16 at the boundary
    Vh = V.copy()
    Vh[2:8] = 7.0
    assert d2_ties_points(P, Vh, q, 6)[1][0] == False  # noqa: E712  every tied run carries one value
    Vh[7] = 8.0
    assert d2_ties_points(P, Vh, q, 6)[1][0] == True  # noqa: E712  the run reaches a third value past k + 1
    # sqrt merges what d2 tells apart: 1 + 2^-52 and 1 + 2^-51 have one square root
    P2 = np.array([[np.sqrt(1.0 + 2.0 ** -52), 0, 0], [0, np.sqrt(1.0 + 2.0 ** -51), 0]] + [[9.0 + j, 0, 0] for j in range(12)])
    d2, _ = cpu_ref.knn_bruteforce(P2, q, 2, squared=True)
    if d2[0, 0] != d2[0, 1] and np.sqrt(d2[0, 0]) == np.sqrt(d2[0, 1]):
        assert not d2_ties_points(P2, np.arange(42.0).reshape(14, 3), q, 1)[0][0]


@pytest.mark.parametrize("name,k", NT.runs())
def test_exact_tie_cap_and_finite_oracle(name, k):
    """(a)"""
    tie, het = NT.ties(name, k)
    print(f"{name} k={k} (2^-{NT.exponent(name, k)}): exact d2 ties {tie.mean():.2%}, on differing values "
          f"{het.mean():.2%} (cap {NT.EXCLUDED_CAP:.0%})")
    for method in ("idw",) + (("sibson",) if k in NT.K_SIBSON else ()):
        for a in NT.oracle_knn(name, k, method):
            assert np.isfinite(a).all()
    assert het.mean() <= NT.EXCLUDED_CAP


@pytest.mark.parametrize("name,k", NT.runs())
def test_near_ties_present(name, k):
    """(b).  The control twins_gap_36 is the exception the other way round: its twins are 2^-36 apart,
    16 truncation steps at unit distance, so a pair shares a truncation only when the displacement is
    within about d 2^-5 rad of perpendicular to the line of sight (probability about d / 32 per pair):
    at most a quarter of the voxels have one in the list and at most 5 % at the boundary.
    twins_gap_40 sits on the truncation step and lies between the control and twins_gap_43."""
    inl, bnd = NT.near_tie_shares(name, k)
    print(f"{name} k={k}: near tie in the list {inl:.2%}, at the k-th/(k+1)-th {bnd:.2%}")
    if name == "twins_gap_36":
        assert inl <= 0.25 and bnd <= 0.05
    elif name == "twins_gap_40":
        lo, hi = NT.near_tie_shares("twins_gap_36", k), NT.near_tie_shares("twins_gap_43", k)
        assert lo[0] < inl <= hi[0] and lo[1] <= bnd <= hi[1]
    else:
        assert k == 1 or inl >= 0.90
        assert k % 2 == 0 or bnd >= 0.50
    if k % 2 == 0 and not name.startswith("twins_gap_4"):
        assert bnd == 0.0  # an even k ends between two pairs of twins


@pytest.mark.parametrize("name,k", NT.runs())
def test_kdtree_agrees_with_bruteforce(name, k):
    """(c)"""
    P = NT.case(name, k)[0]
    _, it = cpu_ref.knn_kdtree(P, NT.queries(name), k)
    ib = NT.lists(name, k)[1][:, :k]
    keep = NT.keep(name, k).ravel()
    assert np.array_equal(np.asarray(it).reshape(len(ib), -1)[keep], ib[keep])


def test_scaled_variants_keep_every_comparison():
    for e in NT.SCALES:
        d2, idx = NT.lists(f"twins@scale_2^{e}")
        d2b, idxb = NT.lists("twins")
        assert np.array_equal(idx, idxb) and np.array_equal(d2, d2b * 4.0 ** e)


def test_gap_cases_share_one_cloud():
    """Every particle's nearest particle is its twin, 2^-e away up to the rounding of the twin's
    coordinates (half an ulp of a coordinate below 16 per axis: under 2^-49 in all)."""
    Q = NT.case("twins")[1]
    for e in NT.GAPS:
        P, Qe, *_ = NT.case(f"twins_gap_{e}")
        assert np.array_equal(Qe, Q)
        d = np.sort(np.linalg.norm(P[:, None, :] - P[None, :, :], axis=2), axis=1)[:, 1]
        assert np.all(np.abs(d - 2.0 ** -e) <= 2.0 ** -49)
    assert np.array_equal(NT.case("twins_gap_43")[0], NT.case("twins")[0])


@pytest.mark.parametrize("k", NT.K_FILTER)
def test_filter_case(k):
    """The outlier filter lists k + 1 entries (the particle itself first): for even k the list splits a
    pair of twins.  Particles whose (k+1)-th / (k+2)-th d2 tie exactly are at most 5 %; the tree's and
    the brute-force restatement agree on every other particle."""
    P, Q, *_ = NT.case("twins")
    tie = NT.filter_ties("twins", k)
    d2 = NT.filter_lists("twins")[0]
    t = NT.trunc(d2[:, :k + 2], NT.N)
    split = float(((t[:, k] == t[:, k + 1]) & (d2[:, k] != d2[:, k + 1])).mean())
    print(f"filter k={k}: boundary exact ties {tie.mean():.2%}, boundary near ties {split:.2%}")
    assert tie.mean() <= NT.EXCLUDED_CAP
    assert (d2[:, 0] == 0.0).all() and (d2[:, 1] > 0.0).all()  # column 0 is the particle itself, never its twin
    assert k % 2 == 1 or split >= 0.50
    kt, _ = cpu_ref.outlier_filter(P, Q, k, 3.0)
    kb, _ = cpu_ref.outlier_filter(P, Q, k, 3.0, knn="bruteforce")
    assert np.array_equal(kt[~tie], kb[~tie])


@pytest.mark.parametrize("k", NT.K_RBF)
def test_mirror_case(k):
    """mirror: near ties as in twins ((b)), no exact boundary tie beyond the cap, the tree's neighbour
    sets equal the brute-force ones, and the reference's own LAPACK solve is within 1e-10 normwise of
    the extended-precision solve of the same systems, so the GPU's bar is 1e-10 and nothing wider."""
    P, Q, ax, ay, az = NT.case("mirror")
    assert NT.shape("mirror") == (1, 10, 13) and np.abs(P[:, 2] - NT.MIRROR_Z0).min() >= NT.MIRROR_CLEAR - 1e-9
    dmin = np.sort(np.linalg.norm(P[:, None, :] - P[None, :, :], axis=2), axis=1)[:, 1].min()
    assert dmin > 1e-3  # no near-coincident particles
    inl, bnd = NT.near_tie_shares("mirror", k)
    tie = NT.rbf_ties("mirror", k)
    print(f"mirror k={k}: near tie in the list {inl:.2%}, at the boundary {bnd:.2%}, exact boundary ties {tie.mean():.2%}")
    assert inl >= 0.90 and bnd >= 0.50 and tie.mean() <= NT.EXCLUDED_CAP
    _, it = cpu_ref.knn_kdtree(P, NT.queries("mirror"), k)
    ib = NT.lists("mirror")[1][:, :k]
    assert np.array_equal(np.sort(it, axis=1)[~tie], np.sort(ib, axis=1)[~tie])
    lap, ext = NT.oracle_rbf("mirror", k, "lapack"), NT.oracle_rbf("mirror", k, "extended")
    for c in range(3):
        gap = normwise(lap[~tie, c], ext[~tie, c])
        print(f"mirror TPS k={k} {'UVW'[c]}: lapack-vs-exact {gap:.3e}")
        assert gap <= TOL_RBF
