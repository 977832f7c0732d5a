"""GPU checks of the device component labelling (csrc/ptv_label.hip behind ``labelling.label``).

Everything is compared with ``np.array_equal`` against ``scipy.ndimage.label`` on the same mask: the
labels are integers and the numbering is part of the contract, so there is no tolerance anywhere.

Shapes are the smallest that reach every path: single voxels and rows, rows longer than a wave, several
tiles with a partial tile on every axis, and per axis the tile's extent - 1, the extent itself and + 1.
Those nine shapes are derived from ``labelling.TILE``, which tests/test_label_host.py holds to the named
constants of the kernels (csrc/ptv_label.hpp kLabelTileZ / kLabelTileY / kLabelTileX).
"""
import itertools

import numpy as np
import pytest
from scipy import ndimage

import _label_ref as ref
import _mesh_ref as mref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lab():
    from ptv_interpolation_amd import _lib, labelling

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return labelling


def tile():
    from ptv_interpolation_amd import labelling

    return labelling.TILE


def same_as_scipy(lab, mask, connectivities=ref.CONNECTIVITIES, what=""):
    """The device's labels and count equal scipy's for each structure; returns the counts."""
    nums = []
    for c in connectivities:
        want, num = ndimage.label(mask, ref.structure(c))
        got, got_num = lab.label(mask, ref.structure(c))
        assert isinstance(got_num, int) and got_num == num, (what, c, got_num, num)
        assert got.dtype == np.int32 and got.shape == mask.shape, (what, c)
        assert np.array_equal(got, want), (what, c)
        nums.append(num)
    return nums


SHAPES = ref.SMALL_SHAPES + ref.LONG_ROW_SHAPES + [ref.MANY_TILES_SHAPE]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shapes_and_masks(lab, shape):
    for name, mask in ref.masks(shape):
        same_as_scipy(lab, mask, what=name)


def test_tile_edge_shapes(lab):
    """Per axis the tile's extent - 1, the extent and + 1, derived from ``labelling.TILE``."""
    shapes = ref.tile_edge_shapes(tile())
    assert len(shapes) == 9 and len(set(shapes)) == 9
    for shape in shapes:
        for name, mask in ref.masks(shape):
            same_as_scipy(lab, mask, what=(shape, name))


def test_default_structure_is_six_neighbours(lab):
    mask = np.random.default_rng(5).random((9, 10, 70)) < 0.3
    got, num = lab.label(mask)
    want, want_num = ndimage.label(mask)
    assert num == want_num and np.array_equal(got, want)
    got, num = lab.label(mask, output=np.int32)
    assert num == want_num and np.array_equal(got, want)


# ---- contact type: what tells 6, 18 and 26 neighbours, and the tile pass from the border pass, apart ----
def _contact_offsets():
    """One offset per direction up to sign: faces, edges and corners (the first nonzero component +1)."""
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]


def test_contact_type(lab):
    tz, ty, tx = tile()
    shape = (2 * tz + 2, 2 * ty + 2, 2 * tx + 2)
    for o in _contact_offsets():
        axes = [a for a in range(3) if o[a]]
        # inside one tile, then straddling a tile boundary on every non-empty subset of the offset's axes
        for k in range(len(axes) + 1):
            for across in itertools.combinations(axes, k):
                b = [2, 2, 2]
                for a in across:
                    b[a] = tile()[a] - 1 if o[a] > 0 else tile()[a]
                for a in axes:
                    if a not in across and o[a] < 0:
                        b[a] = 3
                mask = np.zeros(shape, bool)
                mask[tuple(b)] = True
                mask[tuple(p + d for p, d in zip(b, o))] = True
                assert mask.sum() == 2
                nums = same_as_scipy(lab, mask, what=(o, across))
                assert nums == [1 if len(axes) <= most else 2 for most in (1, 2, 3)], (o, across, nums)


# ---- deep trees ----
def serpentine(shape=(9, 9, 65)):
    """A one-voxel-wide path along x that turns at alternating ends in y, then in z."""
    nz, ny, nx = shape
    m = np.zeros(shape, bool)
    end = nx - 1  # the x at which the current row is left
    ys = list(range(0, ny, 2))
    for z in range(0, nz, 2):
        for j, y in enumerate(ys):
            m[z, y, :] = True
            if j + 1 < len(ys):
                m[z, (y + ys[j + 1]) // 2, end] = True
            elif z + 2 < nz:
                m[z + 1, y, end] = True
            end = nx - 1 - end
        ys = ys[::-1]
    return m


def spiral(n=41):
    """A square spiral, one voxel wide with one voxel between its turns, in (1, n, n)."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True

    def free(p, q):
        return not (0 <= p < n and 0 <= q < n) or not m[p, q]

    while True:
        for _ in range(2):
            if 0 <= y + dy < n and 0 <= x + dx < n and not m[y + dy, x + dx] and free(y + 2 * dy, x + 2 * dx):
                y, x = y + dy, x + dx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m[None]


@pytest.mark.parametrize("make", [serpentine, spiral])
def test_deep_trees(lab, make):
    mask = make()
    assert mask.sum() > 400
    assert ndimage.label(mask)[1] == 1  # the path is one component already under 6 neighbours
    assert same_as_scipy(lab, mask) == [1, 1, 1]
    # reversed along x: the first voxel is far from where the unions start
    assert same_as_scipy(lab, np.ascontiguousarray(mask[:, :, ::-1])) == [1, 1, 1]
    # the path's complement is one more deep shape (its corridors)
    same_as_scipy(lab, ~mask)


# ---- late equivalence ----
def combs():
    """Teeth that are separate until the last row, plane and tile."""
    out = []
    m = np.zeros((10, 11, 70), bool)  # planes at even x, joined in the last row of the last plane only
    m[:, :, ::2] = True
    m[:-1, -1, :] = False
    m[-1, -1, :] = True
    out.append(m)
    m = np.zeros((10, 19, 70), bool)  # rows at even y, joined at the last x of the last plane
    m[:, ::2, :] = True
    m[-1, :, -1] = True
    out.append(m)
    m = np.zeros((20, 9, 9), bool)  # slabs at even z, joined at the last corner
    m[::2] = True
    m[:, -1, -1] = True
    out.append(m)
    m = np.zeros((3, 20, 130), bool)  # nested U shapes, each closed in its last row
    for k in range(4):
        m[1, 2 * k:20 - 2 * k, 2 * k] = True
        m[1, 2 * k:20 - 2 * k, 129 - 2 * k] = True
        m[1, 19 - 2 * k, 2 * k:130 - 2 * k] = True
    out.append(m)
    return out


def test_late_equivalence(lab):
    for m in combs():
        for flip in ((), (2,), (1,), (0, 1, 2)):
            same_as_scipy(lab, np.ascontiguousarray(np.flip(m, flip)) if flip else m, what=(m.shape, flip))


# ---- wave edges ----
def _row(nx, runs):
    r = np.zeros(nx, bool)
    for a, b in runs:
        r[a:b + 1] = True  # clipped at nx
    return r


@pytest.mark.parametrize("nx", [63, 64, 65, 130])
def test_wave_edges(lab, nx):
    patterns = [[(0, 0)], [(63, 63)], [(64, 64)], [(0, 63)], [(60, 70)], [(63, 64)], [(1, 62)], [(0, 62), (64, 129)],
                [(0, 0), (62, 62), (64, 65), (127, 128)], [(0, 129)]]
    for pa, pb in itertools.product(patterns, repeat=2):
        mask = np.zeros((2, 2, nx), bool)
        mask[0, 0] = mask[1, 1] = _row(nx, pa)
        mask[0, 1] = _row(nx, pb)
        same_as_scipy(lab, mask, what=(pa, pb))


# ---- dtypes, repeats, sizes ----
def test_dtypes_and_repeats(lab):
    rng = np.random.default_rng(11)
    big = rng.random(ref.MANY_TILES_SHAPE) < 0.31
    small = rng.random((5, 7, 9)) < 0.5
    first, num = lab.label(big, ref.structure(26))
    again, num2 = lab.label(big, ref.structure(26))
    assert num == num2 and first.tobytes() == again.tobytes()
    assert np.array_equal(first, ndimage.label(big, ref.structure(26))[0])
    # a small volume after a larger one: the buffers are already grown
    same_as_scipy(lab, small)
    want = ndimage.label(small, ref.structure(18))[0]
    signed = np.where(small, rng.integers(-5, 0, small.shape), 0).astype(np.int32)
    wide = np.where(small, rng.integers(1, 2**40, small.shape), 0).astype(np.int64)
    for m in (small, small.astype(np.uint8) * 200, signed, wide, small.astype(np.uint16) * 256):
        assert (m != 0).sum() == small.sum()
        assert np.array_equal(lab.label(m, ref.structure(18))[0], want), m.dtype
    # a view that is not contiguous
    assert np.array_equal(lab.label(big[::2, 1::2, ::3])[0], ndimage.label(big[::2, 1::2, ::3])[0])


def test_sizes(lab):
    shape = (9, 17, 70)
    z, y, x = np.indices(shape)
    rng = np.random.default_rng(3)
    for mask in ((z + y + x) % 2 == 1, rng.random(shape) < 0.31, np.zeros(shape, bool), np.ones(shape, bool)):
        for c in ref.CONNECTIVITIES:
            labels, num, sizes = lab.label(mask, ref.structure(c), return_sizes=True)
            want, want_num = ndimage.label(mask, ref.structure(c))
            assert num == want_num and np.array_equal(labels, want)
            assert sizes.dtype == np.int64 and sizes.shape == (num + 1,)
            assert np.array_equal(sizes, np.bincount(labels.ravel(), minlength=num + 1))


def test_label_dev_keeps_the_labels_on_the_device(lab):
    import torch

    from ptv_interpolation_amd import _lib

    mask = np.random.default_rng(7).random((9, 17, 70)) < 0.2
    nz, ny, nx = mask.shape
    dev = torch.device("cuda:0")
    mk = torch.from_numpy(mask.view(np.uint8)).to(dev)
    labels = torch.full(mask.shape, -7, dtype=torch.int32, device=dev)
    sizes = torch.full((_lib.label_sizes_room(mask.size),), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx = _lib.Context.get(0)
    for c in ref.CONNECTIVITIES:
        st = ctx.label_dev(nx, ny, nz, mk.data_ptr(), labels.data_ptr(), c, sizes_ptr=sizes.data_ptr())
        want, num, want_sizes = lab.label(mask, ref.structure(c), return_sizes=True)
        assert st["n_components"] == num and st["n_foreground"] == int(mask.sum())
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy(), want)
        assert np.array_equal(sizes[:num + 1].cpu().numpy(), want_sizes)
        assert st["ms_merge"] > 0 and st["ms_number"] > 0
    st = ctx.label_dev(nx, ny, nz, mk.data_ptr(), labels.data_ptr(), 6)  # without the sizes
    assert np.array_equal(labels.cpu().numpy(), ndimage.label(mask)[0])


# ---- the chain: label, then the staircase drag on the labels ----
def test_chain_into_the_interface_drag(lab):
    from ptv_interpolation_amd import velocity_analysis as va

    shape = (20, 24, 28)
    solid = np.zeros(shape, bool)
    for z0, y0, x0 in itertools.product((2, 11), (2, 10, 18), (3, 15)):
        solid[z0:z0 + 4, y0:y0 + 3, x0:x0 + 5] = True
    u, v, w, p = mref.make_fields(shape, 0)
    labels, num = lab.label(solid)
    want, want_num = ndimage.label(solid)
    assert num == want_num == 12 and np.array_equal(labels, want)
    args = (u, v, w, p, 1.5e-3, 0.7, 1.1, 0.3)
    got = va.compute_interface_drag(*args, mask=labels)
    ref_drag = va.compute_interface_drag(*args, mask=want)
    assert list(got) == list(range(1, num + 1)) == list(ref_drag)
    for label in got:
        assert list(got[label]) == list(ref_drag[label])
        for key in got[label]:
            assert np.array_equal(np.asarray(got[label][key]), np.asarray(ref_drag[label][key])), (label, key)
