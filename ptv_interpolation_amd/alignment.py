"""Mask alignment on the MI355X: the exact Euclidean distance transform of a mask and the
reference's offset search over it (auto_align.py:10-62).

``distance_transform_edt`` is ``scipy.ndimage.distance_transform_edt`` for 3-D masks with unit
spacing, bit for bit: an integer kernel produces the squared distances and the float64 field is
their correctly rounded square root (csrc/ptv_edt.hip).

``alignment_objective`` evaluates the reference's objective for a batch of offsets: per offset the
device returns ``{n_inside, n_outside, sum}`` and the host forms ``1e9`` when no point is inside,
else ``sum + n_outside * max(dt)``.

``find_best_offset`` has the reference's signature, prints and return value; scipy's Powell search
runs on the host over the GPU objective, with the particles and the field resident on the device.
There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib

__all__ = ["distance_transform_edt", "alignment_objective", "find_best_offset"]

OUTSIDE_SCORE = 1e9  # the reference's value when every point is outside the volume


def _foreground(input):
    """The mask as uint8 (nonzero = foreground), after the checks that need no data: bool or integer
    dtype, 3-D, a shape the 32-bit squared distances can hold.  The checks read the shape alone, so
    they come before any copy."""
    a = np.asarray(input)
    if a.dtype.kind not in "biu":
        raise NotImplementedError(f"mask of dtype {a.dtype} (GPU distance transform: bool or integer)")
    _lib.edt_check_shape(a.shape)
    if a.dtype == np.bool_:
        return np.ascontiguousarray(a).view(np.uint8)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a != 0).view(np.uint8)


def distance_transform_edt(input, sampling=None, return_distances=True, return_indices=False, *,
                           return_squared=False):
    """``scipy.ndimage.distance_transform_edt(input)`` on the GPU: for every nonzero voxel of the 3-D
    ``input`` (any bool or integer dtype) the float64 distance to the nearest zero voxel.  With
    ``return_squared`` the int32 squared distances instead.

    ``sampling`` other than None and ``return_indices`` raise ``NotImplementedError`` (anisotropic
    spacing has no integer kernel and no bit-exact oracle), as do shapes that are not 3-D or have
    nz^2 + ny^2 + nx^2 >= 2^31.  An input without a zero voxel raises ``ValueError``: scipy returns
    distances to a voxel that is not there.  An empty input gives an empty result."""
    if sampling is not None:
        raise NotImplementedError("sampling is not supported on the GPU (unit spacing only)")
    if return_indices:
        raise NotImplementedError("return_indices is not supported on the GPU")
    if not return_distances:
        raise ValueError("at least one of return_distances / return_indices must be True")
    mask = _foreground(input)
    if mask.size == 0:
        return np.zeros(mask.shape, dtype=np.int32 if return_squared else np.float64)
    d2, dist, _ = _lib.Context.get(0).edt(mask, want_d2=return_squared, want_distance=not return_squared)
    return d2 if return_squared else dist


def _points(points):
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be (n, 3) as x, y, z, got shape {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("points must be finite")
    return np.ascontiguousarray(p)


def _offsets(offsets):
    o = np.asarray(offsets, dtype=np.float64)
    if o.ndim == 1 and o.size == 3:
        o = o.reshape(1, 3)
    if o.ndim != 2 or o.shape[1] != 3:
        raise ValueError(f"offsets must be (m, 3) as dx, dy, dz, got shape {o.shape}")
    if not np.isfinite(o).all():
        raise ValueError("offsets must be finite")
    return np.ascontiguousarray(o)


def objective_values(records, max_dt):
    """The reference's objective from the device's records: ``1e9`` where no point is inside, else
    ``sum + n_outside * max(dt)`` (an int64 times a float64, then one float64 addition)."""
    rec = np.asarray(records)
    val = rec["sum"] + rec["n_outside"] * np.float64(max_dt)
    return np.where(rec["n_inside"] == 0, OUTSIDE_SCORE, val)


def alignment_objective(points, dt_or_mask, offsets):
    """The reference's objective at each of ``offsets`` (m, 3) for ``points`` (n, 3) as x, y, z.

    ``dt_or_mask``: the float64 distance field (nz, ny, nx), or a bool / integer solid mask whose
    distance transform is taken first.  Returns ``(values, records)``: float64 (m,) and the device's
    records (``_lib.ALIGN_RECORD``: n_inside, n_outside, sum)."""
    p = _points(points)
    o = _offsets(offsets)
    f = np.asarray(dt_or_mask)
    if f.dtype.kind == "f":
        if f.ndim != 3:
            raise ValueError(f"the distance field must be 3-D, got shape {f.shape}")
        _lib.edt_check_shape(f.shape)
        if f.size == 0:
            raise ValueError("the distance field is empty")
        dt = np.ascontiguousarray(f, dtype=np.float64)
        max_dt = dt.max()
        ctx = _lib.Context.get(0)
        session = _lib.AlignSession(ctx, p, dt.shape, dt)
    else:
        mask = _foreground(f)
        if mask.size == 0:
            raise ValueError("the mask is empty")
        ctx = _lib.Context.get(0)
        _, _, st = ctx.edt(mask, want_d2=False, want_distance=False, keep_distance=True)
        max_dt = np.sqrt(np.float64(st["max_d2"]))
        session = _lib.AlignSession(ctx, p, mask.shape)
    rec = session.score(o)
    return objective_values(rec, max_dt), rec


def find_best_offset(df, mask, initial_offset=(0, 0, 0), invert=False):
    """The (dx, dy, dz) offset that minimises the points in solid regions (auto_align.py:10-62):
    the distance transform of the solid and the objective on the GPU, scipy's Powell search on the
    host.  ``mask`` is True for fluid unless ``invert``.  Returns ``(res.x, res.fun)``."""
    from scipy.optimize import minimize

    mask = np.asarray(mask)
    if mask.dtype != np.bool_:
        # the reference's ~mask is a bitwise not: only a bool mask means fluid / solid there
        raise NotImplementedError(f"mask of dtype {mask.dtype} (GPU alignment: a bool mask)")
    _lib.edt_check_shape(mask.shape)
    points = _points(df[['x', 'y', 'z']].values)
    solid = np.ascontiguousarray(mask if invert else ~mask).view(np.uint8)

    print("Computing Distance Transform...")
    ctx = _lib.Context.get(0)
    _, _, st = ctx.edt(solid, want_d2=False, want_distance=False, keep_distance=True)
    max_dt = np.sqrt(np.float64(st["max_d2"]))  # sqrt is monotone: the maximum of the field
    session = _lib.AlignSession(ctx, points, solid.shape)

    def objective(offset):
        o = np.asarray(offset, dtype=np.float64).reshape(1, 3)
        if not np.isfinite(o).all():
            raise ValueError("offsets must be finite")
        return objective_values(session.score(o), max_dt)[0]

    print(f"Starting optimization from initial offset {initial_offset}...")
    res = minimize(objective, initial_offset, method='Powell', tol=1e-1)
    return res.x, res.fun
