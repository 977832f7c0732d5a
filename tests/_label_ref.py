"""A numpy restatement of the labelling contract (ptv_interpolation_amd.labelling),
and the shapes and masks that the CPU oracle test and the GPU tests share.

``label_ref`` builds the components by union-find over the linear voxel index (z slowest, x fastest)
with minimum-index roots: every link lowers a parent (``np.minimum.at``), so a component's final root
is its first voxel in raster order.  The components are numbered by the rank of their roots.
tests/test_label_oracle.py holds this to ``scipy.ndimage.label`` with ``==``: it is the proof that
scipy's numbering is the raster order of the first voxels, on which the device kernels rest.
"""
import itertools

import numpy as np

CONNECTIVITIES = (6, 18, 26)


def structure(connectivity):
    """``scipy.ndimage.generate_binary_structure(3, c)`` for 6, 18, 26 neighbours (c = 1, 2, 3)."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return np.abs(np.indices((3, 3, 3)) - 1).sum(axis=0) <= most


def backward_offsets(connectivity):
    """The neighbours in front of a voxel in raster order: 3, 9 or 13 offsets (dz, dy, dx)."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3)
            if o < (0, 0, 0) and sum(c != 0 for c in o) <= most]


def _roots(parent):
    """Every voxel's root: pointer jumping until nothing moves (parent[v] <= v, so it ends)."""
    while True:
        up = parent[parent]
        if np.array_equal(up, parent):
            return parent
        parent = up


def label_ref(mask, connectivity=6):
    """``(labels int32, num_features, sizes int64)`` of the 3-D ``mask`` (nonzero = foreground)."""
    fg = np.asarray(mask) != 0
    nz, ny, nx = fg.shape
    n = fg.size
    index = np.arange(n, dtype=np.int64).reshape(fg.shape)
    pairs = []
    for dz, dy, dx in backward_offsets(connectivity):
        here = (slice(max(0, -dz), nz - max(0, dz)), slice(max(0, -dy), ny - max(0, dy)),
                slice(max(0, -dx), nx - max(0, dx)))
        there = (slice(max(0, dz), nz - max(0, -dz)), slice(max(0, dy), ny - max(0, -dy)),
                 slice(max(0, dx), nx - max(0, -dx)))
        both = fg[here] & fg[there]
        pairs.append((index[here][both], index[there][both]))
    a = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    b = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
    parent = np.arange(n, dtype=np.int64)
    while True:
        parent = _roots(parent)
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        if np.array_equal(lo, hi):
            break
        np.minimum.at(parent, hi, lo)  # a link only ever lowers the larger root's parent
    flat = fg.ravel()
    is_root = flat & (parent == np.arange(n))
    rank = np.cumsum(is_root) - is_root  # exclusive scan of the root flags
    labels = np.where(flat, rank[parent] + 1, 0).astype(np.int32).reshape(fg.shape)
    num = int(is_root.sum())
    return labels, num, np.bincount(labels.ravel(), minlength=num + 1).astype(np.int64)


# ---- shapes and masks shared by the oracle test and the GPU tests ----
SMALL_SHAPES = [(1, 1, 1), (1, 1, 7), (2, 2, 2), (1, 5, 9), (5, 1, 9), (5, 7, 9)]
LONG_ROW_SHAPES = [(3, 4, 70), (70, 3, 4), (3, 70, 4)]
MANY_TILES_SHAPE = (33, 65, 130)


def tile_edge_shapes(tile):
    """Per axis one shape whose extent is the tile's extent - 1, the extent itself and + 1 (the other
    axes short and odd), from the (z, y, x) tile of the device's tile-local pass."""
    base = (3, 5, 7)
    out = []
    for axis in range(3):
        for delta in (-1, 0, 1):
            s = list(base)
            s[axis] = tile[axis] + delta
            out.append(tuple(s))
    return out


def masks(shape, seed=0):
    """``[(name, bool mask)]``: the masks every shape is labelled with."""
    rng = np.random.default_rng(seed + 1000 * shape[0] + 100 * shape[1] + shape[2])
    z, y, x = np.indices(shape)
    out = [("background", np.zeros(shape, bool)), ("foreground", np.ones(shape, bool))]
    corner = np.zeros(shape, bool)
    corner[-1, -1, -1] = True
    out.append(("last corner", corner))
    out.append(("checkerboard", (z + y + x) % 2 == 1))
    for fill in (0.05, 0.2, 0.31, 0.5, 0.9):
        out.append((f"random {fill}", rng.random(shape) < fill))
    for axis, c in enumerate((z, y, x)):
        out.append((f"planes along axis {axis}", c % 2 == 0))
    return out
