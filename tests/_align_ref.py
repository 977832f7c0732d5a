"""A numpy restatement of the mask alignment (auto_align.find_best_offset's distance field and
objective), written from the behaviour, and the bound the GPU sums are held to.
test_align_oracle.py holds this module to scipy and to the reference's fixtures
(tests/golden/align_*.npz).

Distance transform: for every nonzero voxel the Euclidean distance to the nearest zero voxel, 0 at
zero voxels.  ``edt2_brute`` is the definition itself (a minimum over all zero voxels, integers),
usable for tiny shapes; ``edt`` is scipy's, whose float64 result is sqrt of that integer.

Objective at an offset o: s = points + o; indices = round half to even; a point is inside when all
three indices are in range; value = 1e9 when none is inside, else sum(dt at the inside points) +
(number outside) * max(dt).

Bound.  Every gathered distance is >= 0, so S = sum of them.  Any order of summing n float64 numbers
lies within gamma(n) S of the exact sum E.  The device adds the points of a block in a tree and then
combines at most MAX_PARTIALS per-block partial sums (kAlignMaxBlocks in csrc/ptv_kernels.hpp,
read off the code), so |gpu - E| <= gamma(n + MAX_PARTIALS) S, numpy's pairwise sum obeys the same
bound, and |gpu - numpy| <= 2 gamma(n + MAX_PARTIALS) S.
"""
import math

import numpy as np
from scipy import ndimage

U64 = 2.0**-53
MAX_PARTIALS = 1024
OUTSIDE_SCORE = 1e9
RECORD = np.dtype([("n_inside", np.int64), ("n_outside", np.int64), ("sum", np.float64)])


def gamma(n, u=U64):
    n = max(int(n), 1)
    return (n - 1) * u / (1.0 - (n - 1) * u)


def edt2_brute(mask):
    """Integer squared distances by the definition; the mask must hold a zero."""
    m = np.asarray(mask) != 0
    zeros = np.argwhere(~m).astype(np.int64)
    assert len(zeros), "no zero voxel"
    out = np.zeros(m.shape, dtype=np.int64)
    for idx in np.argwhere(m):
        out[tuple(idx)] = ((zeros - idx) ** 2).sum(axis=1).min()
    return out


def edt(mask):
    """scipy's float64 distances."""
    return ndimage.distance_transform_edt(np.asarray(mask) != 0)


def edt2(mask):
    """The integer squared distances behind scipy's float64 result."""
    d = edt(mask)
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), d), "scipy's result is not sqrt of an integer"
    return d2


def gathered(points, dt, offset):
    """(valid, distances at the valid points) at one offset."""
    nz, ny, nx = dt.shape
    s = np.asarray(points, dtype=np.float64).reshape(-1, 3) + np.asarray(offset, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # a coordinate past the int64 range casts to a value out of range
        ix = np.round(s[:, 0]).astype(np.int64)
        iy = np.round(s[:, 1]).astype(np.int64)
        iz = np.round(s[:, 2]).astype(np.int64)
    valid = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny) & (iz >= 0) & (iz < nz)
    return valid, dt[iz[valid], iy[valid], ix[valid]]


def record(points, dt, offset):
    """(n_inside, n_outside, numpy's sum, exact sum E) at one offset."""
    valid, d = gathered(points, dt, offset)
    n_in = int(valid.sum())
    return n_in, int(valid.size - n_in), float(np.sum(d)) if n_in else 0.0, math.fsum(d.tolist())


def objective(points, dt, offset):
    valid, d = gathered(points, dt, offset)
    if not valid.any():
        return OUTSIDE_SCORE
    return np.sum(d) + np.sum(~valid) * np.max(dt)


def sum_bound(n_inside, exact_sum):
    """|a float64 sum of the n_inside gathered distances, combined from at most MAX_PARTIALS partial
    sums, - E|.  The terms are >= 0, so S = E."""
    return gamma(n_inside + MAX_PARTIALS) * exact_sum


# ---- the seeded cases of the fixtures (tests/golden/make_align_golden.py) and of the GPU tests ----
def layered_case():
    """Mask (24, 10, 12), fluid at z in [3, 9) and [14, 21); 4000 points inside the layers, shifted
    by -3 in z.  Every distance of this field is an integer, so every sum is exact in any order."""
    rng = np.random.default_rng(2024)
    mask = np.zeros((24, 10, 12), dtype=bool)
    mask[3:9] = True
    mask[14:21] = True
    n = 4000
    layer = rng.integers(0, 2, n)
    z = np.where(layer == 0, rng.uniform(3.0, 8.0, n), rng.uniform(14.0, 20.0, n)) - 3.0
    pts = np.stack([rng.uniform(0.0, 11.0, n), rng.uniform(0.0, 9.0, n), z], axis=1)
    return mask, pts, (0, 0, 0)


def blob_case():
    """Fluid mask (20, 22, 26) of random cubic blobs, 3000 points drawn in the fluid and shifted."""
    rng = np.random.default_rng(77)
    coarse = rng.random((5, 6, 7)) < 0.6
    mask = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:20, :22, :26].copy()
    fluid = np.argwhere(mask)
    pick = fluid[rng.integers(0, len(fluid), 3000)]
    pts = pick[:, ::-1].astype(np.float64) + rng.uniform(-0.45, 0.45, (3000, 3)) + np.array([1.6, -2.2, 0.7])
    return mask, pts, (0, 0, 0)


CASES = {"layered": layered_case, "blob": blob_case}
PROBE_OFFSETS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [0.5, -0.5, 1.5], [-1.6, 2.2, -0.7], [100.0, 0.0, 0.0],
                          [2.5, 2.5, 2.5], [-7.0, 3.0, 11.0]])


class Frame:
    """The one thing find_best_offset asks of its DataFrame: ``df[['x', 'y', 'z']].values``."""

    def __init__(self, pts):
        self.pts = np.asarray(pts, dtype=np.float64)

    def __getitem__(self, cols):
        assert list(cols) == ["x", "y", "z"]
        return self

    @property
    def values(self):
        return self.pts
