"""The case table of the device marching cubes (ptv_mc_table.hpp): the committed header is what
tools/make_mc_table.py generates, it agrees with the numpy oracle of the rule (_mc_ref.py, which
does not read it) on every case, and the rule's stated properties hold: 820 triangles, at most 5
per cube, no triangle below sqrt(3)/8, no fan diagonal in a cube face, and closed, oriented,
edge-manifold surfaces with inward normals on random interior masks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mc_ref as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "ptv_interpolation_amd", "csrc", "ptv_mc_table.hpp")


def _header_table():
    txt = open(HDR).read()
    counts = [int(t) for t in re.search(r"kMcCount\[256\] = \{(.*?)\};", txt, re.S).group(1).replace("\n", " ").split(",")
              if t.strip()]
    rows = re.findall(r"^\s*\{([0-9, ]+)\},\s*// (\d+)$", txt, re.M)
    assert len(counts) == 256 and len(rows) == 256 and [int(c) for _, c in rows] == list(range(256))
    tab = []
    for n, (row, _) in zip(counts, rows):
        ids = [int(t) for t in row.split(",")]
        assert len(ids) == 16 and all(e < 12 for e in ids[:3 * n]) and all(e == 255 for e in ids[3 * n:])
        tab.append([tuple(ids[3 * k:3 * k + 3]) for k in range(n)])
    return tab


@pytest.fixture(scope="module")
def header():
    return _header_table()


def test_committed_header_is_generated():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_mc_table.py"), "--stdout"],
                         capture_output=True, text=True, check=True).stdout
    assert out == open(HDR).read()


def test_table_equals_the_oracle_on_every_single_cube_volume(header):
    for case in range(256):
        vol = np.array([(case >> c) & 1 for c in range(8)], dtype=np.int32).reshape(2, 2, 2)
        got = mc.marching_cubes(vol, 1)
        want = header[case]
        if not want:
            assert got is None, case
            continue
        verts, faces = got
        # the table's triangles in coordinates, through the single cube's vertex numbering
        mids = np.array([mc._midpoint(e) for e in range(12)], dtype=np.float32)
        tri_pts = np.array([[mids[e] for e in tri] for tri in want], dtype=np.float32)
        assert np.array_equal(verts[faces], tri_pts), case
        assert mc.case_triangles(case) == want, case


def test_counts(header):
    per = [len(t) for t in header]
    assert sum(per) == 820 and max(per) == 5
    assert per[0] == 0 and per[255] == 0 and all(n > 0 for n in per[1:255])


def test_no_small_triangle_and_no_diagonal_in_a_face(header):
    mids = np.array([mc._midpoint(e) for e in range(12)])
    smallest = np.inf
    for case, tris in enumerate(header):
        for a, b, c in tris:
            smallest = min(smallest, np.linalg.norm(np.cross(mids[b] - mids[a], mids[c] - mids[a])) / 2.0)
        # fan diagonals: the triangle sides that are not sides of the cycle (= not face segments)
        sides = {}
        for tri in tris:
            for i in range(3):
                key = frozenset((tri[i], tri[(i + 1) % 3]))
                sides[key] = sides.get(key, 0) + 1
        for key, n in sides.items():
            e, f = tuple(key)
            if n == 2:  # shared by two triangles of the cube: a diagonal
                assert not mc._shares_a_face(e, f), (case, e, f)
            else:       # a side of the cycle lies in a face by construction
                assert n == 1 and mc._shares_a_face(e, f), (case, e, f)
    assert smallest >= np.sqrt(3.0) / 8.0 * (1.0 - 1e-12), smallest


@pytest.mark.parametrize("n, density, seed", [(10, 0.2, 0), (10, 0.5, 1), (12, 0.8, 2), (11, 0.5, 3)])
def test_random_interior_masks_give_closed_oriented_surfaces(header, n, density, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, n, n), dtype=np.int32)
    m[1:-1, 1:-1, 1:-1] = rng.random((n - 2,) * 3) < density
    verts, faces = mc.marching_cubes(m, 1)
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))  # every vertex is used, none twice made
    assert len(np.unique(verts, axis=0)) == len(verts)
    assert mc.closed_and_oriented(faces)
    assert mc.signed_volume(verts, faces) < 0.0
    # and the same surface assembled from the header's table, cube by cube
    want = set()
    for z, y, x in np.ndindex(n - 1, n - 1, n - 1):
        case = sum(int(m[z + (c >> 2 & 1), y + (c >> 1 & 1), x + (c & 1)]) << c for c in range(8))
        for tri in header[case]:
            want.add(tuple(tuple(2 * (mc._midpoint(e) + (z, y, x))) for e in tri))
    got = {tuple(tuple(2.0 * p) for p in verts[f].astype(np.float64)) for f in faces}
    assert got == want and len(got) == len(faces)
