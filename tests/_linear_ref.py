"""scipy's Delaunay point location, restated in numpy from the arrays of a ``Delaunay`` object
(``simplices``, ``neighbors``, ``transform``, ``min_bound``, ``max_bound``), and the condition the
linear kernels are held to, voxel by voxel.

What scipy does per query (spatial/_qhull.pyx ``_find_simplex``, ``_find_simplex_directed``,
``_find_simplex_bruteforce``; interpolate/interpnd.pyx ``LinearNDInterpolator._do_evaluate``):

* a point strictly outside ``[min_bound - eps, max_bound + eps]`` on some axis has no simplex;
* a directed walk moves from simplex to simplex through the first face with ``c_k < -eps`` and stops
  at a simplex whose four coordinates all lie in ``[-eps, 1 + eps]`` (an *accepting* simplex), or at a
  hull face (no simplex), or, when it meets a degenerate simplex (NaN transform) or runs too long,
  hands over to the brute-force scan;
* the scan returns the first simplex in index order that accepts the point.  A degenerate simplex
  cannot be tested itself: in its place its valid neighbours are tested in slot order, with
  ``-eps_broad`` in place of ``-eps`` on the coordinate that faces the degenerate simplex.

Where the walk stops depends on where it started, so two correct locators may differ wherever more
than one simplex accepts.  The scan's answer does not depend on a start.  Hence the condition
(``admissible`` / ``unexplained``): an output must equal, to the bit, the interpolant of some accepting
simplex or of the scan's answer, and may be the fill value only where scipy's rule can end without a
simplex.

Arithmetic is scipy's, in its order: ``c_i = ((0 + T_i0 d_0) + T_i1 d_1) + T_i2 d_2`` for i < 3,
``c_3 = ((1 - c_0) - c_1) - c_2``, ``out = (((0 + c_0 v_0) + c_1 v_1) + c_2 v_2) + c_3 v_3``.
The keyword arguments ``c3``, ``eps`` and ``nth`` exist for the mutation tests only.
"""
import functools

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
EPS = 100.0 * DBL_EPSILON
# Delaunay.find_simplex: eps_broad = sqrt(eps) with eps = 100 * DBL_EPSILON
EPS_BROAD_FIND_SIMPLEX = float(np.sqrt(100.0 * DBL_EPSILON))
# LinearNDInterpolator (what griddata calls) and k_linear_brute: sqrt(DBL_EPSILON); settled by
# tests/test_linear_ref.py::test_eps_broad_of_the_interpolator
EPS_BROAD = float(np.sqrt(DBL_EPSILON))

PAIRS_PER_CHUNK = 1 << 19  # (query, simplex) pairs held at once


def _chunks(nq, nsimplex):
    step = max(1, PAIRS_PER_CHUNK // max(1, nsimplex))
    for lo in range(0, nq, step):
        yield lo, min(nq, lo + step)


def valid_simplices(tri):
    """(nsimplex,) bool: the transform is not NaN (scipy tests transform[s, 0, 0] only)."""
    T = tri.transform
    return T[:, 0, 0] == T[:, 0, 0]


def barycentric(T, q, c3="chain"):
    """(4, m, ns) coordinates of queries q (m, 3) in the simplices with transforms T (ns, 4, 3)."""
    d = [q[:, j, None] - T[None, :, 3, j] for j in range(3)]  # 3 x (m, ns)
    Tc = np.ascontiguousarray(T[:, :3, :].transpose(1, 2, 0))  # (3, 3, ns)
    c = np.empty((4,) + d[0].shape)
    for i in range(3):
        ci = 0.0 + Tc[i, 0][None, :] * d[0]
        ci += Tc[i, 1][None, :] * d[1]
        ci += Tc[i, 2][None, :] * d[2]
        c[i] = ci
    if c3 == "chain":
        c[3] = ((1.0 - c[0]) - c[1]) - c[2]
    else:  # the mutation: 1 - (c_0 + c_1 + c_2)
        c[3] = 1.0 - ((c[0] + c[1]) + c[2])
    return c


def barycentric_in(tri, q, s, c3="chain"):
    """(m, 4) coordinates of query i in simplex s[i]."""
    T = tri.transform[s]
    d = q - T[:, 3, :]
    c = []
    for i in range(3):
        ci = np.zeros(len(q))
        for j in range(3):
            ci = ci + T[:, i, j] * d[:, j]
        c.append(ci)
    if c3 == "chain":
        c.append(((1.0 - c[0]) - c[1]) - c[2])
    else:
        c.append(1.0 - ((c[0] + c[1]) + c[2]))
    return np.stack(c, -1)


def interpolate_in(tri, values, q, s, c3="chain"):
    """(m, 3): the interpolant of simplex s[i] at query i, interpnd's sum order."""
    c = barycentric_in(tri, q, s, c3)
    vv = values[tri.simplices[s]]  # (m, 4, 3)
    out = np.zeros((len(q), values.shape[1]))
    for j in range(4):
        out = out + c[:, j, None] * vv[:, j]
    return out


def fully_outside(tri, q, eps=EPS):
    """_is_point_fully_outside: strict comparisons against the box widened by eps."""
    return ((q < tri.min_bound - eps) | (q > tri.max_bound + eps)).any(axis=1)


def _inside(c, eps):
    """c (4, ...) -> (...) bool; NaN coordinates are not inside."""
    with np.errstate(invalid="ignore"):
        return ((c >= -eps) & (c <= 1.0 + eps)).all(axis=0)


def accepting(tri, q, eps=EPS, c3="chain"):
    """(m, nsimplex) bool: valid simplices with all four coordinates in [-eps, 1 + eps]."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    ok = valid_simplices(tri)
    out = np.zeros((len(q), len(ok)), bool)
    for lo, hi in _chunks(len(q), len(ok)):
        out[lo:hi] = _inside(barycentric(tri.transform, q[lo:hi], c3), eps) & ok[None, :]
    return out


def _scan_results(tri, c, eps, eps_broad, acc=None):
    """(m, nsimplex) int: what the scan returns if it stops at simplex i (-1: it goes on)."""
    ok = valid_simplices(tri)
    nb = tri.neighbors
    if acc is None:
        acc = _inside(c, eps) & ok[None, :]
    res = np.where(acc, np.arange(len(ok), dtype=np.int32)[None, :], np.int32(-1))
    for i in np.nonzero(~ok)[0]:
        r = np.full(c.shape[1], -1)
        for k in range(4):
            n = nb[i, k]
            if n == -1 or not ok[n]:
                continue
            lo = np.where(nb[n] == i, -eps_broad, -eps)  # leeway towards the degenerate simplex
            cn = c[:, :, n]  # (4, m)
            with np.errstate(invalid="ignore"):
                inn = ((cn >= lo[:, None]) & (cn <= 1.0 + eps)).all(axis=0)
            r = np.where((r < 0) & inn, n, r)
        res[:, i] = r
    return res


def brute_force(tri, q, eps_broad, eps=EPS, c3="chain", nth=0, with_step=False):
    """_find_simplex_bruteforce: (m,) simplex per query, -1 for none.  ``nth`` = 1 is the mutation
    that stops at the second index that accepts.  ``with_step`` also returns the index at which the
    scan stopped (a degenerate simplex where the answer came through the neighbour rule)."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    ns = len(tri.simplices)
    out = np.full(len(q), -1)
    step = np.full(len(q), -1)
    for lo, hi in _chunks(len(q), ns):
        res = _scan_results(tri, barycentric(tri.transform, q[lo:hi], c3), eps, eps_broad)
        hit = res >= 0
        sel = hit if nth == 0 else hit & (np.cumsum(hit, axis=1) == nth + 1)
        found = sel.any(axis=1)
        at = sel.argmax(axis=1)
        out[lo:hi] = np.where(found, res[np.arange(hi - lo), at], -1)
        step[lo:hi] = np.where(found, at, -1)
    outside = fully_outside(tri, q, eps)
    out[outside] = -1
    step[outside] = -1
    return (out, step) if with_step else out


def scan_table(tri, q, eps_broad, eps=EPS):
    """(m, nsimplex) int32: the scan's answer if it stopped at index i, -1 where index i does not
    accept (small inputs only: not chunked).  The scan returns the first entry >= 0 of a row."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    return _scan_results(tri, barycentric(tri.transform, q), eps, eps_broad)


def brute_values(tri, values, q, fill, eps_broad, **kw):
    """(m, 3): what a locator that always scans writes (fill where the scan finds nothing)."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    s = brute_force(tri, q, eps_broad, **kw)
    out = interpolate_in(tri, values, q, np.maximum(s, 0), kw.get("c3", "chain"))
    out[s < 0] = fill
    return out


class Admissible:
    """The allowed (u, v, w) per query: ``triples[ptr[i]:ptr[i + 1]]`` (interpolants of the accepting
    simplices, then of the scan's answer) and ``fill_ok[i]``."""

    def __init__(self, ptr, triples, simplex, fill_ok, fill, scan, outside, n_accepting):
        self.ptr, self.triples, self.simplex = ptr, triples, simplex
        self.fill_ok, self.fill, self.scan, self.outside, self.n_accepting = fill_ok, fill, scan, outside, n_accepting

    def has_value(self):
        return np.diff(self.ptr) > 0

    def n_distinct(self):
        """(m,) distinct admissible triples per query, the fill value included where allowed."""
        owner = np.repeat(np.arange(len(self.fill_ok)), np.diff(self.ptr))
        owner = np.concatenate([owner, np.nonzero(self.fill_ok)[0]])
        t = np.concatenate([self.triples, np.full((int(self.fill_ok.sum()), 3), self.fill)])
        rows = np.unique(np.column_stack([owner.astype(np.uint64), _bits(t)]), axis=0)
        return np.bincount(rows[:, 0].astype(np.int64), minlength=len(self.fill_ok))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def admissible(tri, values, q, fill, eps_broad, eps=EPS):
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    values = np.asarray(values, dtype=np.float64)
    ok = valid_simplices(tri)
    hull = (tri.neighbors == -1) & ok[:, None]  # (ns, 4): faces of valid simplices on the hull
    hs = np.nonzero(hull.any(axis=1))[0]
    ns = len(ok)
    owner, simplex = [], []
    exits = np.zeros(len(q), bool)
    scan = np.full(len(q), -1)
    n_acc = np.zeros(len(q), np.int64)
    for lo, hi in _chunks(len(q), ns):
        c = barycentric(tri.transform, q[lo:hi])
        acc = _inside(c, eps) & ok[None, :]
        n_acc[lo:hi] = acc.sum(axis=1)
        i, s = np.nonzero(acc)
        owner.append(i + lo)
        simplex.append(s)
        with np.errstate(invalid="ignore"):
            exits[lo:hi] = ((c[:, :, hs] < -eps) & hull[hs].T[:, None, :]).any(axis=(0, 2))
        res = _scan_results(tri, c, eps, eps_broad, acc)
        hit = res >= 0
        scan[lo:hi] = np.where(hit.any(axis=1), res[np.arange(hi - lo), hit.argmax(axis=1)], -1)
    outside = fully_outside(tri, q, eps)
    scan[outside] = -1
    owner = np.concatenate(owner + [np.nonzero(scan >= 0)[0]])
    simplex = np.concatenate(simplex + [scan[scan >= 0]])
    order = np.argsort(owner, kind="stable")
    owner, simplex = owner[order], simplex[order]
    triples = interpolate_in(tri, values, q[owner], simplex)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(q)))])
    fill_ok = outside | (scan < 0) | exits
    return Admissible(ptr, triples, simplex, fill_ok, float(fill), scan, outside, n_acc)


def unexplained(got, adm):
    """Indices of the queries whose (u, v, w) bytes match none of their admissible triples.
    ``got``: (m, 3), or three arrays of m values each."""
    if isinstance(got, (tuple, list)):
        got = np.stack([np.asarray(g, dtype=np.float64).ravel() for g in got], -1)
    got = np.ascontiguousarray(got, dtype=np.float64).reshape(-1, 3)
    m = len(adm.fill_ok)
    assert len(got) == m
    gb = _bits(got)
    owner = np.repeat(np.arange(m), np.diff(adm.ptr))
    same = (gb[owner] == _bits(adm.triples)).all(axis=1)
    explained = np.bincount(owner[same], minlength=m) > 0
    explained |= adm.fill_ok & (gb == _bits(np.array([adm.fill]))[0]).all(axis=1)
    return np.nonzero(~explained)[0]


# -------------------------------------------------------------------------------------------------
# the cases shared by tests/test_linear_ref.py (CPU) and tests/test_gpu_linear_location.py (GPU)
# -------------------------------------------------------------------------------------------------
FILL = -7.5
# name -> built for more than one admissible triple at some voxel.  one_simplex is built for the hull
# exit and the bounding box alone (one simplex cannot tie with another); walk_from_0 for long walks
# in general position.
CASES = {"lattice_off": True, "lattice_on": True, "bounds": True, "one_simplex": False, "two_simplices": True,
         "walk_from_0": False}
VERTEX_PICKS = (0, 300, 900, 1800, 2700)


def lattice():
    g = np.arange(6.0)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    Q = np.random.default_rng(9).standard_normal((len(P), 3))
    return P, Q


def grid_queries(ax, ay, az):
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(P, Q, (ax, ay, az), Delaunay) of a named case, arrays read-only."""
    from scipy.spatial import Delaunay

    from tests import _geometry as G

    if name in ("lattice_off", "lattice_on"):
        P, Q = lattice()
        a = np.linspace(-0.37, 5.41, 23) if name == "lattice_off" else np.arange(-0.5, 6.0, 0.5)
        axes = (a, a, a)
    elif name in ("bounds", "walk_from_0"):
        P, Q, *_ = G.case("base")
    elif name in ("one_simplex", "two_simplices"):
        # vertices on nodes of the integer grid -1 .. 6: voxels on vertices, edges, faces, the hull
        # planes and (two_simplices: the fifth particle lies outside the first four's circumsphere, so
        # Qhull adds one simplex) the shared face x + y + z = 4
        P = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [5, 5, 5]])[:4 if name == "one_simplex" else 5]
        Q = np.random.default_rng(12).standard_normal((len(P), 3))
        a = np.arange(-1.0, 7.0)
        axes = (a, a, a)
    else:
        raise KeyError(name)
    d = Delaunay(P)
    if name == "bounds":
        pick = np.argsort(np.linalg.norm(P - P.mean(axis=0), axis=1))[list(VERTEX_PICKS)]
        t = np.array([EPS / 2, EPS, 2 * EPS])
        axes = tuple(np.sort(np.concatenate([[d.min_bound[c]], P[pick, c], [d.max_bound[c]], d.min_bound[c] - t,
                                             d.max_bound[c] + t])) for c in range(3))
    elif name == "walk_from_0":
        axes = (np.linspace(0.0, 12.0, 16), np.linspace(0.25, 11.5, 16), np.linspace(1.0, 11.0, 16))
    for a in axes:
        a.setflags(write=False)
    return P, Q, axes, d


@functools.lru_cache(maxsize=None)
def case_admissible(name, eps_broad=EPS_BROAD):
    P, Q, axes, d = case(name)
    return admissible(d, Q, grid_queries(*axes), FILL, eps_broad)


def flat_face_probes(tri, points, deltas):
    """Probes across every face that a valid simplex n shares with a degenerate simplex i: three points
    of the face, each moved out of n towards i until n's coordinate facing i is -delta.  Returns
    (queries (m, 3), delta per query).  A walk that arrives in n leaves through that face into i and
    hands over to the scan, whose answer at index i is n if and only if delta <= eps_broad."""
    ok = valid_simplices(tri)
    T = tri.transform
    q, dl = [], []
    for i in np.nonzero(~ok)[0]:
        for k in range(4):
            n = tri.neighbors[i, k]
            if n == -1 or not ok[n]:
                continue
            m = int(np.nonzero(tri.neighbors[n] == i)[0][0])
            face = points[tri.simplices[n][np.arange(4) != m]]
            g = T[n, m] if m < 3 else -(T[n, 0] + T[n, 1] + T[n, 2])  # gradient of c_m
            for w in ((1 / 3, 1 / 3, 1 / 3), (0.5, 0.3, 0.2), (0.2, 0.2, 0.6)):
                x = np.asarray(w) @ face
                for d in deltas:
                    q.append(x - d * g / (g @ g))
                    dl.append(d)
    return np.array(q), np.array(dl)


def share_line(name, eps_broad=EPS_BROAD):
    """One line of profiles/linear_location_parity.txt: the voxel counts of a case."""
    P, Q, axes, d = case(name)
    adm = case_admissible(name, eps_broad)
    m = len(adm.fill_ok)
    q = grid_queries(*axes)
    multi = adm.n_accepting > 1
    distinct = adm.n_distinct() > 1
    both = adm.fill_ok & adm.has_value()
    # a walk that starts in a degenerate simplex hands every in-box voxel to the scan
    ok = valid_simplices(d)
    return (f"{name}: voxels {m}, simplices {len(ok)} ({int((~ok).sum())} degenerate), outside the box "
            f"{int(adm.outside.sum())}, no simplex (fill only) {int((adm.fill_ok & ~adm.has_value()).sum())} "
            f"({np.mean(adm.fill_ok & ~adm.has_value()):.1%}), more than one accepting simplex {int(multi.sum())} "
            f"({multi.mean():.1%}), more than one distinct triple {int(distinct.sum())} ({distinct.mean():.1%}), "
            f"fill and a value both admissible {int(both.sum())} ({both.mean():.1%}), "
            f"in the box (flagged when forced to scan) {int((~fully_outside(d, q)).sum())}")
