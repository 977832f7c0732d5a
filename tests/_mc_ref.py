"""A numpy oracle of the device marching cubes' triangulation rule, written
from the rule: face segments, cycles, orientation, fans, then the volume in cube order with shared
vertices.  It does not read the generated table (ptv_mc_table.hpp); test_mc_table.py holds the two
against each other.

Coordinates are (z, y, x).  Corner c of a cube has the offset ((c >> 2) & 1, (c >> 1) & 1, c & 1);
edges are numbered axis z, y, x and within an axis by the lower corner's index.
"""
import itertools

import numpy as np

CORNERS = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)])
# edge id -> (lower corner, axis)
EDGE_LOW = [(c, ax) for ax in range(3) for c in range(8) if CORNERS[c][ax] == 0]
EDGE_AXIS = np.array([ax for _, ax in EDGE_LOW])
EDGE_OFF = np.array([CORNERS[c] for c, _ in EDGE_LOW])  # the owner lattice point, relative to the cube


def _edge_between(a, b):
    lo, hi = min(a, b), max(a, b)
    ax = {4: 0, 2: 1, 1: 2}[hi - lo]
    return EDGE_LOW.index((lo, ax))


def _midpoint(e):
    m = EDGE_OFF[e].astype(float)
    m[EDGE_AXIS[e]] += 0.5
    return m


def _face_loops():
    """Each face as its four corners in cyclic order."""
    loops = []
    for ax, side in itertools.product(range(3), (0, 1)):
        on = [c for c in range(8) if CORNERS[c][ax] == side]
        a = on[0]
        nbrs = [c for c in on if np.abs(CORNERS[c] - CORNERS[a]).sum() == 1]
        far = [c for c in on if np.abs(CORNERS[c] - CORNERS[a]).sum() == 2][0]
        loops.append([a, nbrs[0], far, nbrs[1]])
    return loops


FACE_LOOPS = _face_loops()


def _shares_a_face(e, f):
    a, b = _midpoint(e), _midpoint(f)
    return any(a[k] == b[k] and a[k] in (0.0, 1.0) for k in range(3))


def case_cycles(case):
    """The oriented vertex cycles (lists of edge ids) of one case."""
    inside = [bool((case >> c) & 1) for c in range(8)]
    links = {}  # edge -> set of edges joined to it by a face segment
    for loop in FACE_LOOPS:
        sides = [(loop[i], loop[(i + 1) % 4]) for i in range(4)]
        cut = [_edge_between(a, b) for a, b in sides if inside[a] != inside[b]]
        pairs = []
        if len(cut) == 2:
            pairs.append(tuple(cut))
        elif len(cut) == 4:  # the ambiguous face: each inside corner is cut off on its own
            for i in range(4):
                if inside[loop[i]]:
                    pairs.append((_edge_between(loop[i - 1], loop[i]), _edge_between(loop[i], loop[(i + 1) % 4])))
        for e, f in pairs:
            links.setdefault(e, []).append(f)
            links.setdefault(f, []).append(e)
    cycles, left = [], set(links)
    while left:
        start = min(left)
        cyc = [start]
        left.discard(start)
        while True:
            step = [f for f in links[cyc[-1]] if f in left]
            if not step:
                break
            cyc.append(min(step) if len(cyc) == 1 else step[0])
            left.discard(cyc[-1])
        # orientation: the polygon's normal must look at the inside ends of its edges
        p = np.array([_midpoint(e) for e in cyc])
        normal = sum(np.cross(p[i] - p[0], p[i + 1] - p[0]) for i in range(1, len(p) - 1))
        towards = np.zeros(3)
        for e in cyc:
            lo, ax = EDGE_LOW[e]
            d = np.zeros(3)
            d[ax] = -1.0 if inside[lo] else 1.0  # from the outside end to the inside end
            towards += d
        if normal @ towards < 0:
            cyc = cyc[:1] + cyc[:0:-1]
        cycles.append(cyc)
    return cycles


def case_triangles(case):
    """The triangles (edge id triples) of one case, in the rule's order."""
    tris = []
    for cyc in case_cycles(case):
        n = len(cyc)
        for r in range(n):
            c = cyc[r:] + cyc[:r]
            if not any(_shares_a_face(c[0], c[k]) for k in range(2, n - 1)):
                break
        else:
            raise AssertionError(f"case {case}: no apex without an in-face diagonal")
        tris += [(c[0], c[k], c[k + 1]) for k in range(1, n - 1)]
    return tris


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = [case_triangles(c) for c in range(256)]
    return _TABLE


def marching_cubes(mask, label, step_size=1):
    """``(verts float32 (n, 3), faces int32 (m, 3))`` of one label, or None without a triangle."""
    s = int(step_size)
    ind = (np.asarray(mask) == label)[::s, ::s, ::s]
    if min(ind.shape) < 2:
        return None
    L = np.array(ind.shape)
    # vertices: one per lattice edge whose ends differ, numbered by (owner point, axis)
    has = np.zeros(tuple(L) + (3,), dtype=bool)
    has[:-1, :, :, 0] = ind[:-1] != ind[1:]
    has[:, :-1, :, 1] = ind[:, :-1] != ind[:, 1:]
    has[:, :, :-1, 2] = ind[:, :, :-1] != ind[:, :, 1:]
    vid = np.full(has.shape, -1, dtype=np.int64)
    vid[has] = np.arange(int(has.sum()))
    z, y, x, ax = np.nonzero(has)
    verts = (np.stack([z, y, x], axis=1) * s).astype(np.float32)
    verts[np.arange(len(ax)), ax] += np.float32(s) / np.float32(2)
    # cases per cube
    C = L - 1
    case = np.zeros(tuple(C), dtype=np.int64)
    for c in range(8):
        dz, dy, dx = CORNERS[c]
        case |= ind[dz:dz + C[0], dy:dy + C[1], dx:dx + C[2]].astype(np.int64) << c
    flat = case.reshape(-1)
    keys, rows = [], []
    for c in np.unique(flat):
        tris = table()[c]
        if not tris:
            continue
        cubes = np.nonzero(flat == c)[0]
        cz, cy, cx = np.unravel_index(cubes, tuple(C))
        for k, tri in enumerate(tris):
            cols = [vid[cz + EDGE_OFF[e][0], cy + EDGE_OFF[e][1], cx + EDGE_OFF[e][2], EDGE_AXIS[e]] for e in tri]
            rows.append(np.stack(cols, axis=1))
            keys.append(cubes * 8 + k)
    if not rows:
        return None
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    faces = rows[np.argsort(keys, kind="stable")]
    assert faces.min() >= 0
    return verts, faces.astype(np.int32)


def marching_cubes_labels(mask, labels, step_size=1):
    """``{label: (verts, faces)}`` for the labels that have triangles."""
    out = {}
    for label in labels:
        m = marching_cubes(mask, label, step_size)
        if m is not None:
            out[label] = m
    return out


def closed_and_oriented(faces):
    """Every directed edge occurs once and its reverse occurs once."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    fwd = e[:, 0] * n + e[:, 1]
    rev = e[:, 1] * n + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), v.mean(axis=1)).sum() / 6.0)
