"""Near-tie cases shared by tests/test_near_tie_cases.py (CPU preconditions) and
tests/test_gpu_near_ties.py (GPU parity): clouds in which two DIFFERENT squared distances from a
voxel share the truncation of the packed keys (ptv_knn_impl.hpp make_key: d2 with its low B mantissa
bits replaced by the slot, B = bit length of the largest slot; n = 3000 gives B = 12), on particles
with independent random values.  There the order of the two, and at the k-th / (k+1)-th boundary the
neighbour set, has one right answer that the keys alone cannot give.

``twins``            1500 particles uniform in [-0.5, 12.5]^3, each with a twin displaced by a random
                     unit vector x 2^-43, shuffled; the 13 x 10 x 9 grid of tests/_geometry.py.  The
                     twins' d2 from a voxel differ by about 2^-42 relative: hundreds of ulps, mostly
                     inside one truncation (2^-40 relative).
``twins@scale_2^e``  the same scaled by 2^e (exact: every comparison is kept), e = 80 and -80.
``twins@dense``      the same cloud on the 45 x 41 x 40 grid, where the coarse lattice builds its
                     bounds from near-tied lists.
``twins_gap_<e>``    the same cloud (same base particles, directions, shuffle and values) with twin
                     displacement 2^-e, e in GAPS: from clearly separable (36, the control) across
                     the truncation boundary down to 2^-47, where the two d2 are some tens of ulps
                     apart.
``mirror``           near ties without near-coincident particles (twins make local-RBF systems
                     singular): a one-plane grid 13 x 10 x 1 at z = MIRROR_Z0, 1500 particles with
                     |z - z0| >= 0.3, each mirrored to (x, y, 2 z0 - z + delta), |delta| = 2^-43.

Exact d2 ties.  The closer the twins, the more often their two d2 round to the same double; a voxel
with such a tie on differing values among its first k + 1 has no unique answer and is left out of
the GPU comparisons, and EXCLUDED_CAP (5 %) bounds what may be left out.  Where the cloud alone
exceeds the cap, the displacement of that (case, k) is widened by one binade (WIDENED), measured
shares before -> after:

    twins          k = 127, 129, 130   2^-43 -> 2^-42   5.21 %, 5.30 %, 5.30 % -> 2.74 %, 2.82 %, 2.82 %
    twins_gap_47   k = 20              2^-47 -> 2^-46   5.98 % -> 4.19 %

There is no case below 2^-47, because none can meet the cap.  Two twins' d2 differ by
2 d delta cos(theta) (theta: the angle between the displacement and the line of sight), an ulp of d2
near 1 is 2^-52, and the two round to one double when |cos(theta)| is below about 2^-53 / delta: at
delta = 2^-49 about 3 % of the pairs seen from a voxel, and a list of 13 holds 6 or 7 pairs.  Measured
at k = 13 and 20: 2^-48 gives 9.8 % and 14.8 % of the voxels, 2^-49 17.4 % and 25.2 %, and 2^-50, the
ulp of a coordinate between 4 and 8 (twins with every coordinate above 8 then coincide), 63.1 % and
74.1 %.  A comparison that leaves that much out proves little, so the series ends at 2^-47.

Every case returns ``(P, Q, ax, ay, az)``, read-only; the same arrays go to the GPU and the oracle.
The oracle is ``oracle.cpu_ref`` on brute-force lists (d2 in the search's order
``(dx*dx + dy*dy) + dz*dz``, ascending, ties by lower index), made once per cloud and shared
read-only.
"""
import functools

import numpy as np

from tests import _geometry as G

N_BASE = 1500
N = 2 * N_BASE
GAP = 43
GAPS = (36, 40, 43, 47)
SCALES = (80, -80)
MIRROR_Z0 = 6.0
MIRROR_CLEAR = 0.3
EXCLUDED_CAP = 0.05  # share of voxels with an exact d2 tie on differing values a test may leave out
WIDENED = {("twins", 127): 42, ("twins", 129): 42, ("twins", 130): 42, ("twins_gap_47", 20): 46}

# IDW k on `twins`: the exact pair lists, every key-list length with an odd and an even k, the large-k path
K_PAIRS = (7, 8, 12)
K_KEYS = (13, 14, 21, 22, 29, 31, 39, 47, 55, 63, 95, 127)
K_BIG = (129, 130)
K_SIBSON = (30, 31)
K_VARIANT = (13, 20)  # twins_gap_<e>, the scaled and the dense variants
K_MODES = 21
K_PERMUTED = (13, 21, 50)
K_FILTER = (12, 13, 24, 25, 63)  # listed entries are k + 1
K_RBF = (13, 21)
COLUMNS = {"": 140, "dense": 30}  # brute-force list length kept per cloud: beyond every k + 1 + 8 used on it


def key_bits(n):
    """B as launch_knn computes it: the smallest B >= 1 with 2^B >= n."""
    B = 1
    while B < 31 and (1 << B) < n:
        B += 1
    return B


def trunc(d2, n):
    """d2 with the low B mantissa bits cleared: what a packed key keeps of it."""
    mask = np.uint64(0xFFFFFFFFFFFFFFFF) ^ np.uint64((1 << key_bits(n)) - 1)
    return (np.ascontiguousarray(d2, dtype=np.float64).view(np.uint64) & mask).view(np.float64)


def exponent(name, k=None):
    """e of the twin displacement 2^-e that (case, k) runs with."""
    base = name.partition("@")[0]
    e = GAP if base in ("twins", "mirror") else int(base[len("twins_gap_"):])
    return WIDENED.get((base, k), e)


@functools.lru_cache(maxsize=None)
def _twin_parts():
    rng = np.random.default_rng(4301)
    A = rng.uniform(-0.5, 12.5, (N_BASE, 3))
    u = rng.standard_normal((N_BASE, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    perm = rng.permutation(N)
    Q = rng.standard_normal((N, 3))
    return A, u, perm, Q


@functools.lru_cache(maxsize=None)
def _cloud(base, variant, e):
    _, _, ax, ay, az, _ = G.base(variant == "dense")
    if base == "mirror":
        rng = np.random.default_rng(4302)
        A = rng.uniform(-0.5, 12.5, (4 * N_BASE, 3))
        A = A[np.abs(A[:, 2] - MIRROR_Z0) >= MIRROR_CLEAR][:N_BASE]
        assert len(A) == N_BASE and not variant
        M = A.copy()
        M[:, 2] = 2.0 * MIRROR_Z0 - A[:, 2] + rng.choice([-1.0, 1.0], N_BASE) * 2.0 ** -e
        P = np.concatenate([A, M])[rng.permutation(N)]
        Q = rng.standard_normal((N, 3))
        az = np.array([MIRROR_Z0])
    elif base == "twins" or base.startswith("twins_gap_"):
        A, u, perm, Q = _twin_parts()
        P = np.concatenate([A, A + u * 2.0 ** -e])[perm]
        if variant.startswith("scale_2^"):
            s = 2.0 ** int(variant.split("^")[1])
            P, ax, ay, az = P * s, ax * s, ay * s, az * s
        elif variant not in ("", "dense"):
            raise KeyError(variant)
    else:
        raise KeyError(base)
    return G._ro(*(np.array(a, dtype=np.float64, order="C") for a in (P, Q, ax, ay, az)))


def case(name, k=None):
    """(P, Q, ax, ay, az) of a named case as run with k neighbours, read-only (k matters to the
    WIDENED pairs only)."""
    base, _, variant = name.partition("@")
    return _cloud(base, variant, exponent(name, k))


def queries(name):
    from oracle import cpu_ref

    _, _, ax, ay, az = case(name)
    return cpu_ref.grid_queries(ax, ay, az)


def shape(name):
    _, _, ax, ay, az = case(name)
    return len(az), len(ay), len(ax)


def runs():
    """Every (case, k) of the grid interpolation tests (k = 1 is method='nearest'; 30 and 31 run Sibson,
    31 IDW as well)."""
    out = [("twins", k) for k in (1,) + K_PAIRS + K_KEYS + K_BIG + K_SIBSON + (K_MODES,) + K_PERMUTED]
    out += [(f"twins_gap_{e}", k) for e in GAPS for k in K_VARIANT]
    out += [(f"twins@scale_2^{e}", k) for e in SCALES for k in K_VARIANT]
    out += [("twins@dense", k) for k in K_VARIANT]
    return sorted(set(out), key=out.index)


@functools.lru_cache(maxsize=None)
def _lists(base, variant, e):
    from oracle import cpu_ref

    P, _, ax, ay, az = _cloud(base, variant, e)
    return G._ro(*cpu_ref.knn_bruteforce(P, cpu_ref.grid_queries(ax, ay, az), COLUMNS.get(variant, 140), squared=True))


def lists(name, k=None):
    """(d2, idx): the brute-force lists of the case's voxels, COLUMNS long, ascending d2 (ties by
    lower index), read-only."""
    base, _, variant = name.partition("@")
    return _lists(base, variant, exponent(name, k))


@functools.lru_cache(maxsize=None)
def ties(name, k):
    """(tie, hetero) of tests/_util.d2_ties_points over the case's voxels, (nz, ny, nx) bool:
    ``hetero`` is what the GPU comparisons exclude."""
    from tests._util import d2_ties_lists

    d2, idx = lists(name, k)
    assert d2.shape[1] >= k + 1 + 8
    t, h = d2_ties_lists(d2, idx, case(name, k)[1], k)
    return G._ro(t.reshape(shape(name)), h.reshape(shape(name)))


def keep(name, k):
    return ~ties(name, k)[1]


@functools.lru_cache(maxsize=None)
def oracle_knn(name, k, method="idw"):
    """(U, V, W), read-only: cpu_ref's epilogue of the method ('nearest' for k = 1) on the first k of the
    brute-force lists (what cpu_ref.interp_grid(..., knn="bruteforce") computes, without searching again)."""
    from oracle import cpu_ref

    d2, idx = lists(name, k)
    out = cpu_ref.interp_from_lists(np.sqrt(d2[:, :k]), idx[:, :k], case(name, k)[1], "nearest" if k == 1 else method, 2.0)
    return G._ro(*(np.ascontiguousarray(out[:, c].reshape(shape(name))) for c in range(3)))


def near_tie_shares(name, k):
    """(in_list, boundary): the share of voxels with two distinct d2 of one truncation next to each
    other among the first k of the brute-force order (k = 1: none), and the share whose k-th and
    (k+1)-th are such a pair."""
    d2 = lists(name, k)[0][:, :k + 1]
    t = trunc(d2, N)
    near = (t[:, :-1] == t[:, 1:]) & (d2[:, :-1] != d2[:, 1:])
    return float(near[:, :k - 1].any(axis=1).mean()), float(near[:, k - 1].mean())


@functools.lru_cache(maxsize=None)
def filter_lists(name):
    """(d2, idx) of every particle's 72 nearest particles (itself first), brute force, read-only."""
    from oracle import cpu_ref

    P = case(name)[0]
    return G._ro(*cpu_ref.knn_bruteforce(P, P, max(K_FILTER) + 9, squared=True))


def filter_ties(name, k):
    """(n,) bool: particles whose (k+1)-th and (k+2)-th d2 (the particle itself is the first) tie
    exactly, so that the outlier filter's neighbour set is the search's choice."""
    d2 = filter_lists(name)[0]
    return d2[:, k] == d2[:, k + 1]


def rbf_ties(name, k):
    """(voxels,) bool: the k-th and (k+1)-th d2 tie exactly (the local-RBF neighbour set is the
    search's choice there; inside the set the order does not matter, it is sorted by index)."""
    d2 = lists(name, k)[0]
    return d2[:, k - 1] == d2[:, k]


@functools.lru_cache(maxsize=None)
def oracle_rbf(name, k, solver):
    """cpu_ref.rbf_local_points, thin-plate spline, neighbour sets from the brute-force order."""
    from oracle import cpu_ref

    P, Q, *_ = case(name)
    out = cpu_ref.rbf_local_points(P, Q, queries(name), k, "thin_plate_spline", solver=solver, knn="bruteforce")
    out.setflags(write=False)
    return out
