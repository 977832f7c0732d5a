"""GPU checks of the device marching cubes (csrc/ptv_surface.hip behind ``ptv_marching_cubes``) and
of the mesh drag that integrates its mesh in place.

Every mesh is compared with the numpy oracle of the triangulation rule (tests/_mc_ref.py) by
``np.array_equal``, vertices and faces, label by label: every vertex is a half-integer, exact in
float32, and the order of vertices and triangles is part of the contract, so equality is bitwise.
Parity with scikit-image's triangle set is neither claimed nor tested.

Shapes are the smallest that reach each path: all 256 corner patterns in one slab, an x extent past
one wave with odd extents, step sizes with remainders, more labels than a block has lanes, and the
64^3 sphere pack of the reference's size class.
"""
import numpy as np
import pytest

import _mc_ref as mc
import _mesh_ref as mref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def surface():
    from ptv_interpolation_amd import _lib, surface

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return surface


@pytest.fixture(scope="module")
def va():
    from ptv_interpolation_amd import velocity_analysis

    return velocity_analysis


def same_meshes(got, want):
    assert list(got) == list(want), (list(got), list(want))
    for label in want:
        gv, gf = got[label]
        wv, wf = want[label]
        assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.shape == wv.shape and gf.shape == wf.shape, label
        assert np.array_equal(gv, wv), label
        assert np.array_equal(gf, wf), label


def all_cases_mask():
    """(2, 47, 47): sixteen by sixteen 2x2x2 blocks, one zero voxel apart, hold the 256 corner patterns."""
    m = np.zeros((2, 47, 47), dtype=np.int32)
    for case in range(256):
        by, bx = divmod(case, 16)
        for c in range(8):
            m[(c >> 2) & 1, 3 * by + ((c >> 1) & 1), 3 * bx + (c & 1)] = (case >> c) & 1
    return m


def test_all_256_cases(surface):
    m = all_cases_mask()
    want = mc.marching_cubes_labels(m, [1])
    cases = set()
    for y in range(46):
        for x in range(46):
            cases.add(sum(int(m[(c >> 2) & 1, y + ((c >> 1) & 1), x + (c & 1)]) << c for c in range(8)))
    assert cases == set(range(256))
    same_meshes(surface.marching_cubes_labels(m, [1]), want)
    same_meshes(surface.marching_cubes_labels(m), want)  # labels=None: np.unique(mask) > 0


def mixture_mask():
    """(9, 11, 70): 0, the requested labels 2, 5, 9 and the label 7 nobody asks for; 2 and 5 touch; 9
    is a blob kept off the boundary."""
    rng = np.random.default_rng(11)
    m = rng.choice(np.array([0, 2, 5, 7], dtype=np.int32), size=(9, 11, 70), p=[0.4, 0.25, 0.25, 0.1])
    m[2:7, 3:8, 20:40] = np.where(rng.random((5, 5, 20)) < 0.6, 9, m[2:7, 3:8, 20:40])
    return m


def test_random_mixture_of_labels(surface):
    m = mixture_mask()
    assert np.any((m[:, :, :-1] == 2) & (m[:, :, 1:] == 5))  # an edge that carries two vertices
    want = mc.marching_cubes_labels(m, [2, 5, 9])
    got = surface.marching_cubes_labels(m, [2, 5, 9])
    same_meshes(got, want)
    assert mc.closed_and_oriented(got[9][1]) and mc.signed_volume(*got[9]) < 0.0
    # the order of the labels is the caller's, repeats collapse, an unrequested label changes nothing
    same_meshes(surface.marching_cubes_labels(m, [9, 2, 9]), {9: want[9], 2: want[2]})
    same_meshes(surface.marching_cubes_labels(m, [7]), mc.marching_cubes_labels(m, [7]))


@pytest.mark.parametrize("step", [2, 3])
def test_step_sizes_with_remainders(surface, step):
    rng = np.random.default_rng(step)
    m = rng.integers(0, 3, size=(13, 12, 11)).astype(np.int32)
    assert any((n - 1) % step for n in m.shape)
    same_meshes(surface.marching_cubes_labels(m, [1, 2], step_size=step), mc.marching_cubes_labels(m, [1, 2], step))


def test_empty_results(surface):
    flat = np.ones((1, 8, 8), dtype=np.int32)
    flat[0, 2:5, 2:5] = 2
    assert surface.marching_cubes_labels(flat, [2]) == {}  # a singleton axis has no cubes
    m = np.zeros((6, 7, 8), dtype=np.int32)
    m[2:4, 2:5, 3:6] = 3
    assert surface.marching_cubes_labels(m, [4]) == {}  # absent from the mask
    assert list(surface.marching_cubes_labels(m, [4, 3])) == [3]
    assert surface.marching_cubes_labels(np.full((5, 5, 5), 6, dtype=np.int32)) == {}  # fills the volume
    assert surface.marching_cubes_labels(m, [3], step_size=6) == {}  # nz = 6 < step_size + 1
    assert surface.marching_cubes_labels(m, [3], step_size=9) == {}  # every extent < step_size + 1
    assert surface.marching_cubes_labels(np.zeros((4, 4, 4), dtype=np.int32)) == {}  # no label at all


def test_label_on_the_boundary_gives_the_oracles_open_surface(surface):
    m = np.zeros((7, 8, 9), dtype=np.int32)
    m[0:3, 0:4, 5:9] = 1
    m[5:7, 6:8, 0:2] = 2
    got = surface.marching_cubes_labels(m, [1, 2])
    same_meshes(got, mc.marching_cubes_labels(m, [1, 2]))
    assert not mc.closed_and_oriented(got[1][1])


def test_many_single_voxel_labels(surface):
    """300 labels, more slots than a block has lanes: each voxel's octahedron, in order."""
    n = 20
    rng = np.random.default_rng(3)
    cells = [(z, y, x) for z in range(1, n - 1, 2) for y in range(1, n - 1, 2) for x in range(1, n - 1, 2)]
    pick = rng.permutation(len(cells))[:300]
    m = np.zeros((n, n, n), dtype=np.int32)
    labels = rng.permutation(np.arange(1, 2001))[:300].astype(np.int32)
    for lab, i in zip(labels, pick):
        m[cells[i]] = lab
    got = surface.marching_cubes_labels(m, labels)
    assert list(got) == labels.tolist()
    for lab, i in zip(labels.tolist(), pick):
        verts, faces = got[lab]
        c = np.array(cells[i], dtype=np.float64)
        assert verts.shape == (6, 3) and faces.shape == (8, 3)
        # owner order: the edges below the voxel on z, y, x, then the voxel's own three
        want = np.array([c - (0.5, 0, 0), c - (0, 0.5, 0), c - (0, 0, 0.5), c + (0.5, 0, 0), c + (0, 0.5, 0),
                         c + (0, 0, 0.5)], dtype=np.float32)
        assert np.array_equal(verts, want), lab
        tri = verts[faces].astype(np.float64)
        normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert np.all(np.einsum("ij,ij->i", normal, c - tri.mean(axis=1)) > 0), lab
    same_meshes(got, mc.marching_cubes_labels(m, labels.tolist()))


def test_mask_dtypes(surface):
    m = mixture_mask()[:, :, :20]
    want = surface.marching_cubes_labels(m, [2, 5])
    for dt in (np.uint8, np.int64):
        same_meshes(surface.marching_cubes_labels(m.astype(dt), [2, 5]), want)
    same_meshes(surface.marching_cubes_labels(m == 2, [1]), {1: want[2]})


def test_two_calls_give_the_same_bytes(surface):
    m = mixture_mask()
    a = surface.marching_cubes_labels(m, [2, 5, 9])
    surface.marching_cubes_labels(all_cases_mask(), [1])  # an unrelated call on the same context
    b = surface.marching_cubes_labels(m, [2, 5, 9])
    for label in a:
        assert a[label][0].tobytes() == b[label][0].tobytes() and a[label][1].tobytes() == b[label][1].tobytes()


def sphere_pack(n, centres, radius):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    m = np.zeros((n, n, n), dtype=np.int32)
    for k, c in enumerate(centres):
        m[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= radius ** 2] = k + 1
    return m


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_end_to_end_drag_equals_the_oracle_meshes_bit_for_bit(va, dtype):
    n = 24
    m = sphere_pack(n, [(7.2, 8.1, 7.7), (15.6, 14.9, 16.3)], 4.6)
    u, v, w, p = mref.make_fields((n, n, n), 5, dtype=dtype)
    bg = np.ones((n, n, n), dtype=bool)
    bg[:, :, :9] = False
    h, visc, volume = (0.7, 1.1, 0.3), 1.5e-3, 2.5
    labels = [2, 3, 1]  # 3 has no surface
    meshes = mc.marching_cubes_labels(m, labels)
    assert list(meshes) == [2, 1]
    want = va.integrate_mesh_drag(meshes, u, v, w, p, visc, *h, background_mask=bg, volume=volume)
    got = va.compute_interface_drag_mesh(u, v, w, p, visc, *h, m, labels=labels, volume=volume, background_mask=bg,
                                         triangulation='device')
    assert list(got) == [2, 1]
    for label in want:
        assert list(got[label]) == list(want[label])
        for key in want[label]:
            assert got[label][key].tobytes() == want[label][key].tobytes(), (label, key)
        assert got[label]["Mx"] == got[label]["Fx"] / volume
    # and within the project's bar around the long-double chain, from the oracle's meshes alone
    f64 = [a.astype(np.float64) for a in (u, v, w, p)]
    exact = mref.integrate(meshes, *f64, visc, *h, background=bg, ft=mref.LD)
    plain = mref.integrate(meshes, *f64, visc, *h, background=bg, ft=np.float64)
    for label in want:
        ex, scale = exact[label]
        gap = np.abs(plain[label][0].astype(mref.LD) - ex).astype(np.float64)
        g = np.array([got[label][k] for k in mref.KEYS])
        err = np.abs(g.astype(mref.LD) - ex).astype(np.float64)
        bar = mref.bar(gap, scale)
        print(f"end to end {np.dtype(dtype).name} label {label}: max |g - exact| / bar = "
              f"{np.max(np.where(err == 0, 0.0, err / np.where(bar == 0, 1.0, bar))):.3f}")
        assert np.all(err <= bar), (label, dict(zip(mref.KEYS, err / np.where(bar == 0, 1.0, bar))))


def test_reference_size_sphere_pack(surface):
    n = 64
    centres = [(16 + 32 * a + 0.3, 16 + 32 * b - 0.2, 16 + 32 * c + 0.1) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    m = sphere_pack(n, centres, 13.4)
    want = mc.marching_cubes_labels(m, list(range(1, 9)))
    got = surface.marching_cubes_labels(m)
    assert len(want) == 8
    same_meshes(got, want)
    assert all(mc.closed_and_oriented(f) for _, f in got.values())
