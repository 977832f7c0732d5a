"""Seeded fields, shapes and coordinates for the cubic B-spline prefilter and the order 0 / 1 / 3
sampling (ptv_interpolation_amd/csrc/ptv_mesh.hip behind ``sampling.spline_filter_nearest`` and
``sampling.map_coordinates``), with their two references: scipy in float64 and the long-double chain
of tests/_mesh_ref.py.  No device and no fixture is needed.

Shapes are the smallest that reach each path of the kernels.  The padded length of an axis is n + 24.
  - x pass, 64-column chunks with the recursion's state carried across them: nx = 40 (one exactly
    full chunk), 41 (a last chunk of one column), 104 (two full chunks), 105 (three chunks: the first
    with a middle chunk), 200 (four chunks, the last half full).
  - x pass, 64 rows per block: (2, 8, 3) has (8 + 24)(2 + 24) = 832 = 13 * 64 rows, a full last block.
  - the start sum covers the whole line up to padded length 41 and 40 terms from 42: extents 17 and
    18, on each axis in turn (each pass has its own call).
  - long z and y axes (70): z is strided by a plane, y by a row.
  - (1, 1, 1), and (5, 6, 7) as the plain case.

Coordinates per shape (``coordinates``): inside the fixtures' range [-0.25, n - 0.75]; across the pad
and past it, [-14, n + 13]; every combination per axis of the integers {-13, -12, -1, 0, n - 1, n,
n + 11, n + 12}, and those plus 0.5; and single-axis excursions to -12.25, -12.5, -13, -30, -1e6,
-1e18, to their mirror images n - 1 + 12.25 ... n - 1 + 30 past the high end and to 1e6 and 1e18, the
other two axes inside the field.  Nothing lies beyond 1e18 in magnitude: scipy's integer cast
overflows from 1e19.
"""
import functools

import numpy as np
from scipy import ndimage

import _mesh_ref as mref

SHAPES = [(1, 1, 1), (5, 6, 7),
          (2, 3, 40), (3, 2, 41), (2, 2, 104), (2, 2, 105), (1, 1, 200),
          (2, 8, 3),
          (17, 2, 2), (18, 2, 2), (2, 17, 2), (2, 18, 2), (2, 2, 17), (2, 2, 18),
          (70, 2, 2), (2, 70, 2)]
KINDS = ("normal", "const", "huge", "ramp")
TYPED = ("float32", "int16", "bool")
# every shape with the standard-normal field; the other fields where the recursion's paths differ
# (one sample, the plain case, three chunks, both sides of the start-sum switch, a long strided axis)
OTHER_SHAPES = [(1, 1, 1), (5, 6, 7), (2, 2, 105), (2, 17, 2), (2, 18, 2), (70, 2, 2)]
CASES = ([("normal", s) for s in SHAPES] + [(k, s) for k in KINDS[1:] for s in OTHER_SHAPES] +
         [(k, (5, 6, 7)) for k in TYPED])
LOW = (-12.25, -12.5, -13.0, -30.0, -1e6, -1e18)


def case_id(case):
    return f"{case[0]}-{'x'.join(str(n) for n in case[1])}"


def _rng(tag, shape):
    return np.random.default_rng([tag, *shape])


def field(kind, shape):
    """The field of a case, in its own dtype."""
    normal = _rng(1, shape).standard_normal(shape)
    if kind == "normal":
        return normal
    if kind == "const":
        return np.full(shape, 3.7)
    if kind == "huge":  # a format extreme whose sums must not overflow
        return 1e150 * normal + 1e153
    if kind == "ramp":  # cancellation: the variation sits 1e-9 under the level
        z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
        return 1e6 + 1e-3 * (z + y + x)
    if kind == "float32":
        return normal.astype(np.float32)
    if kind == "int16":
        return np.round(1000.0 * normal).astype(np.int16)
    if kind == "bool":
        return normal > 0
    raise KeyError(kind)


def widen(a):
    """The float64 array the samplers compute on (float32 widens exactly, integers and bool too)."""
    return np.asarray(a).astype(np.float64)


def coordinates(shape):
    """``{kind: (3, n) float64}``, rows z, y, x."""
    rng = _rng(2, shape)
    n = np.array(shape, dtype=np.float64).reshape(3, 1)
    out = {"inside": rng.uniform(-0.25, n - 0.75, (3, 300)),
           "wide": rng.uniform(-14.0, n + 13.0, (3, 300))}
    per_axis = [np.unique([-13.0, -12.0, -1.0, 0.0, m - 1.0, m, m + 11.0, m + 12.0]) for m in shape]
    out["lattice"] = np.stack([g.ravel() for g in np.meshgrid(*per_axis, indexing="ij")])
    out["lattice_half"] = out["lattice"] + 0.5
    cols = []
    for a in range(3):
        m = float(shape[a])
        for v in LOW + tuple(m - 1.0 - v if v > -1e3 else -v for v in LOW):
            c = rng.uniform(-0.25, n - 0.75, (3, 8))
            c[a] = v
            cols.append(c)
    out["excursion"] = np.concatenate(cols, axis=1)
    return out


def past_the_pad(shape, coords):
    """True where a coordinate lies beyond the padded extent on some axis: below -12 or above
    n + 11.  Up to there a clamp to the padded extent and scipy's rule give the same sample."""
    n = np.array(shape, dtype=np.float64).reshape(3, 1)
    return np.any((coords < -mref.PAD) | (coords > n - 1 + mref.PAD), axis=0)


class Reference:
    """scipy's float64 results and the long-double chain's for one case, computed once."""

    def __init__(self, kind, shape):
        self.kind, self.shape = kind, shape
        self.field = field(kind, shape)
        wide = widen(self.field)
        self.fmax = np.abs(wide).max()
        self.coords = coordinates(shape)
        self.points = np.concatenate(list(self.coords.values()), axis=1)
        self.far = past_the_pad(shape, self.points)
        with np.errstate(invalid="ignore", over="ignore"):
            self.coef_scipy = ndimage.spline_filter(np.pad(wide, mref.PAD, mode="edge"), 3, mode="nearest")
            self.scipy = {o: ndimage.map_coordinates(wide, self.points, order=o, mode="nearest") for o in (0, 1, 3)}
            self.coef = mref.prefilter(wide)
            self.exact = {3: mref.sample3(self.coef, self.points), 1: mref.sample1(wide, self.points),
                          0: wide[mref.index0(shape, self.points)]}
        self.cmax = np.abs(self.coef_scipy).max()
        self.scale = {3: self.cmax, 1: self.fmax}

    def gap(self, order):
        """|scipy - exact| per point, float64."""
        return np.abs(self.scipy[order].astype(mref.LD) - self.exact[order]).astype(np.float64)

    def coef_gap(self):
        return np.abs(self.coef_scipy.astype(mref.LD) - self.coef).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    return Reference(kind, shape)


NONFINITE_SHAPE, NONFINITE_AT = (5, 6, 70), (2, 3, 50)


def nonfinite_case(value):
    """A standard-normal (5, 6, 70) field with ``value`` (NaN or Inf) at one interior sample, past the
    40-term horizon of the x pass's start sum (padded x index 62), and coordinates on and around it:
    the integers and half-integers of its neighbourhood, where a zero weight meets the sample, and
    points across the field and the pad."""
    f = field("normal", NONFINITE_SHAPE).copy()
    f[NONFINITE_AT] = value
    near = [np.arange(c - 1.5, c + 2.0, 0.5) for c in NONFINITE_AT]
    grid = np.stack([g.ravel() for g in np.meshgrid(*near, indexing="ij")])
    co = coordinates(NONFINITE_SHAPE)
    return f, np.concatenate([grid, co["inside"], co["wide"]], axis=1)
