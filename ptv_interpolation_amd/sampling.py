"""Cubic B-spline prefilter and ``map_coordinates`` on the GPU (csrc/ptv_mesh.hip behind
``ptv_spline_prefilter`` and ``ptv_map_coordinates``, include/ptv_api.h).

``map_coordinates(input, coordinates, order, mode='nearest')`` restates
``scipy.ndimage.map_coordinates`` for a 3-D real ``input``, ``order`` 0, 1 or 3 and
``mode='nearest'``; the result is float64.  ``spline_filter_nearest(input)`` returns what scipy
samples for order 3: the float64 cubic B-spline coefficients of the input padded by 12
edge-replicated samples on every side, ``spline_filter(np.pad(input, 12, mode='edge'), 3,
mode='nearest')``.  float32 input is widened exactly, integer and bool input is computed as
float64.  Anything else raises ``NotImplementedError``; there is no CPU fallback.

Coordinates outside the field follow scipy for any finite value it defines.  Orders 0 and 1 clamp
the coordinate to ``[0, n - 1]``.  Order 3 samples the padded coefficients at the padded coordinate
clamped to ``[-1, n + 24]``, one sample past either end, with the four indices edge-extended: up to
13 samples outside the field the value still moves, from there on it is saturated.  Beyond 2^62 in
magnitude scipy is undefined (its integer cast overflows; from 1e19 it returns garbage); here such
a coordinate gives the saturated value, the same as at 1e6.

Non-finite field values.  Orders 0 and 1 return NaN and +-Inf exactly where scipy does.  At order 3
one non-finite sample makes every coefficient non-finite, in scipy too; scipy's are NaN or Inf and
the double-double recursion here turns Inf into NaN, so the results agree in finiteness, not in kind.

An order-3 call filters the whole field.  To sample one field several times, filter it once:
``map_coordinates(None, coordinates, shape=input.shape)`` samples the coefficients the last
order-3 call left in the context.
"""
from __future__ import annotations

import numpy as np

from . import _lib, launcher

__all__ = ["spline_filter_nearest", "map_coordinates"]


def _ctx():
    return _lib.Context.get(launcher.devices()[0])


def _input(input):
    a = np.asarray(input)
    if a.ndim != 3:
        raise NotImplementedError(f"{a.ndim}-D input (GPU path: 3-D)")
    if a.dtype.kind in "biu":
        a = a.astype(np.float64)
    if a.dtype not in (np.float32, np.float64):
        raise NotImplementedError(f"input dtype {a.dtype} (GPU path: real, float32 / float64 or integer)")
    if a.size == 0:
        raise ValueError("input has no samples")
    return a


def spline_filter_nearest(input):
    """The coefficients scipy's order-3 ``map_coordinates(mode='nearest')`` samples: shape
    ``(nz + 24, ny + 24, nx + 24)``, float64."""
    a = _input(input)
    return _ctx().spline_prefilter(a)[0]


def map_coordinates(input, coordinates, order=3, mode='nearest', shape=None):
    """``scipy.ndimage.map_coordinates(input, coordinates, order=order, mode='nearest')`` for a 3-D
    real input: ``coordinates`` is ``(3, ...)`` in ``[z, y, x]`` index units and must be finite; the
    result has its trailing shape, float64.  ``input`` None with ``shape``: order 3 on the
    coefficients the last order-3 call left."""
    if mode != 'nearest':
        raise NotImplementedError(f"mode {mode!r} (GPU path: 'nearest')")
    if order not in (0, 1, 3):
        raise NotImplementedError(f"spline order {order!r} (GPU path: 0, 1, 3)")
    if input is None:
        if order != 3 or shape is None:
            raise ValueError("input=None samples resident order-3 coefficients: order=3 and a shape")
        a = None
    else:
        a = _input(input)
    co = np.asarray(coordinates)
    if co.dtype.kind not in "biuf":
        raise NotImplementedError(f"coordinates of dtype {co.dtype}")
    if co.ndim < 1 or co.shape[0] != 3:
        raise ValueError(f"coordinates must have 3 rows (z, y, x), got shape {co.shape}")
    co = co.astype(np.float64, copy=False)
    if not np.all(np.isfinite(co)):
        raise ValueError("coordinates must be finite")
    out_shape = co.shape[1:]
    if co[0].size == 0:
        return np.empty(out_shape, dtype=np.float64)
    out, _ = _ctx().map_coordinates(a, co.reshape(3, -1), order=order, shape=shape)
    return out.reshape(out_shape)
