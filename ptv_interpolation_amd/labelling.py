"""Connected-component labelling of 3-D masks on the GPU (csrc/ptv_label.hip behind ``ptv_label``,
include/ptv_api.h): the step in front of every per-grain result, which take an int32
label volume (the staircase drag, the marching cubes, the mesh tractions).

``label(input, structure)`` is ``scipy.ndimage.label(input, structure)`` for 3-D inputs, bit for bit:
the same voxels get the same numbers.  scipy numbers the components in the raster order (z slowest,
x fastest) of each component's first voxel; the device builds a union-find forest whose roots are
exactly those first voxels and numbers them by an exclusive scan.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib, launcher

__all__ = ["label", "TILE"]

# the tile (z, y, x) of the tile-local pass (csrc/ptv_label.hpp kLabelTileZ / Y / X): shapes around
# these extents are where the tile pass hands over to the border merge
TILE = (8, 8, 64)

_OFFSETS = np.abs(np.indices((3, 3, 3)) - 1).sum(axis=0)
# generate_binary_structure(3, c): the offsets with at most c nonzero components
_STRUCTURES = {6: _OFFSETS <= 1, 18: _OFFSETS <= 2, 26: _OFFSETS <= 3}


def _ctx():
    return _lib.Context.get(launcher.devices()[0])


def _connectivity(structure):
    """6, 18 or 26 for a structure equal to ``generate_binary_structure(3, 1 / 2 / 3)`` (None: 6)."""
    if structure is None:
        return 6
    s = np.asarray(structure)
    if s.shape != (3, 3, 3):
        raise ValueError(f"structure must have shape (3, 3, 3) for a 3-D input, got {s.shape}")
    s = s.astype(bool)
    for c, ref in _STRUCTURES.items():
        if np.array_equal(s, ref):
            return c
    raise NotImplementedError("structure: the GPU labelling supports generate_binary_structure(3, 1), (3, 2) and "
                              "(3, 3) only (6, 18 or 26 neighbours)")


def _checked(input):
    """The input as an array, after the checks that read the dtype and the shape alone: bool or
    integer, 3-D, fewer than 2^31 voxels."""
    a = np.asarray(input)
    if a.dtype.kind not in "biu":
        raise NotImplementedError(f"input of dtype {a.dtype} (GPU labelling: bool or integer)")
    _lib.label_check_shape(a.shape)
    return a


def _foreground(a):
    """The checked input as uint8, nonzero = foreground."""
    if a.dtype == np.bool_:
        return np.ascontiguousarray(a).view(np.uint8)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a != 0).view(np.uint8)


def _check_output(output):
    if output is None:
        return
    if isinstance(output, (type, np.dtype, str)):
        try:
            if np.dtype(output) == np.int32:
                return
        except TypeError:
            pass
    raise NotImplementedError("output: the GPU labelling returns a new int32 array (None or np.int32)")


def label(input, structure=None, output=None, *, return_sizes=False):
    """``scipy.ndimage.label(input, structure)`` on the GPU for a 3-D ``input`` of bool or any integer
    dtype (nonzero = foreground).  Returns ``(labels, num_features)``: int32 labels of the input's
    shape and a Python int; with ``return_sizes`` also the int64 voxel counts
    ``np.bincount(labels.ravel(), minlength=num_features + 1)`` (the background's at index 0).

    ``structure``: None or an array equal to ``generate_binary_structure(3, 1)``, ``(3, 2)`` or
    ``(3, 3)`` (6, 18, 26 neighbours; None means 6).  Another structure, a float input, an ``output``
    other than None or ``np.int32``, an input that is not 3-D or has 2^31 or more voxels raise
    ``NotImplementedError``; a structure of another shape raises ``ValueError``.  All are decided
    before any device work.  ``label.last_times`` holds the device times of the last call."""
    a = _checked(input)
    conn = _connectivity(structure)
    _check_output(output)
    m = _foreground(a)
    if m.size == 0:
        out = (np.zeros(m.shape, dtype=np.int32), 0)
        return out + (np.zeros(1, dtype=np.int64),) if return_sizes else out
    labels, sizes, st = _ctx().label(m, conn, want_sizes=return_sizes)
    label.last_times = {"ms_merge": st["ms_merge"], "ms_number": st["ms_number"]}
    out = (labels, st["n_components"])
    return out + (sizes,) if return_sizes else out


label.last_times = {}
