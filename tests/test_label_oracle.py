"""The numpy restatement of the labelling contract (tests/_label_ref.py) against
``scipy.ndimage.label``, with ``==``, for the three supported structures.

This is the proof, on the CPU, of the claim the device kernels rest on: scipy numbers the components
in the raster order (z slowest, x fastest) of each component's first voxel, so a union-find forest with
minimum-index roots, numbered by the rank of its roots, gives scipy's labels bit for bit.
"""
import numpy as np
import pytest
from scipy import ndimage

import _label_ref as ref

TILE = (8, 8, 64)  # ptv_interpolation_amd.labelling.TILE (test_label_host.py holds the two together)
SHAPES = ref.SMALL_SHAPES + ref.LONG_ROW_SHAPES + ref.tile_edge_shapes(TILE) + [(17, 20, 70)]


def same_as_scipy(mask, connectivity):
    want, num = ndimage.label(mask, ref.structure(connectivity))
    got, got_num, sizes = ref.label_ref(mask, connectivity)
    assert got_num == num
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(sizes, np.bincount(want.ravel(), minlength=num + 1))


def test_structures_are_scipys():
    for rank, connectivity in zip((1, 2, 3), ref.CONNECTIVITIES):
        assert np.array_equal(ref.structure(connectivity), ndimage.generate_binary_structure(3, rank))
        assert len(ref.backward_offsets(connectivity)) == {6: 3, 18: 9, 26: 13}[connectivity]


@pytest.mark.parametrize("connectivity", ref.CONNECTIVITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shapes_and_masks(shape, connectivity):
    for name, mask in ref.masks(shape):
        same_as_scipy(mask, connectivity)


@pytest.mark.parametrize("connectivity", ref.CONNECTIVITIES)
@pytest.mark.parametrize("fill", [0.1, 0.3, 0.5, 0.9])
def test_random_fills(fill, connectivity):
    rng = np.random.default_rng(int(fill * 100) + connectivity)
    same_as_scipy(rng.random((21, 23, 67)) < fill, connectivity)


@pytest.mark.parametrize("connectivity", ref.CONNECTIVITIES)
def test_late_equivalence(connectivity):
    # teeth that are separate until the last row and plane: the number follows the first voxel
    m = np.zeros((6, 9, 20), bool)
    m[:, :, ::2] = True
    m[:, :-1, 1::2] = False
    m[:-1, -1, :] = False
    m[-1, -1, :] = True
    same_as_scipy(m, connectivity)
    same_as_scipy(m[:, :, ::-1], connectivity)
