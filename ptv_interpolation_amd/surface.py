"""Marching cubes of a label mask on the GPU (csrc/ptv_surface.hip behind ``ptv_marching_cubes``,
include/ptv_api.h): the triangulation in front of the mesh interface drag, for all
labels in one pass over the mask.

``marching_cubes_labels(mask, labels, step_size)`` stands where the reference loops
``skimage.measure.marching_cubes((mask == label).astype(float), level=0.5, step_size=...)`` over the
labels (velocity_analysis.py:547-552).  It does NOT reproduce scikit-image's triangle set: on a 0/1
indicator at level 0.5 Lewiner's face tests are exact ties, and scikit-image's tables are not
available to this project.  The surface follows the project's own stated rule (one vertex per
crossing lattice edge at its midpoint, ambiguous faces separate the inside corners, fans that lay no
diagonal into a cube face, normals into the label), in a fixed order: two calls give
the same bytes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib, launcher

__all__ = ["marching_cubes_labels"]


def _ctx():
    return _lib.Context.get(launcher.devices()[0])


def _mask_int32(mask):
    """The 3-D mask as int32: bool or integers of the int32 range (``NotImplementedError`` otherwise)."""
    m = np.asarray(mask)
    if m.dtype.kind not in "biu":
        raise NotImplementedError(f"mask dtype {m.dtype} (GPU path: bool or integers)")
    if m.ndim != 3:
        raise ValueError(f"the mask must be 3-D, got {m.ndim}-D")
    if m.dtype.kind != "b" and m.dtype.itemsize >= 4 and m.dtype != np.int32 and m.size:
        if m.max() > np.iinfo(np.int32).max or m.min() < np.iinfo(np.int32).min:
            raise NotImplementedError("mask values outside the int32 range are not supported on the GPU path")
    return np.ascontiguousarray(m, dtype=np.int32)


def _step_arg(step_size):
    if isinstance(step_size, (bool, np.bool_)) or not isinstance(step_size, (int, np.integer)) or step_size < 1:
        raise ValueError(f"step_size must be an integer >= 1, got {step_size!r}")
    return int(step_size)


def _triangulate(mask, labels, step_size):
    """Validation, then the device call.  Returns ``(labels, slot, vert_counts, tri_counts)``: the
    labels as given (the reference's default when None), per label its slot in the counts, or None
    when there is nothing to triangulate.  The mesh is left in the context."""
    step = _step_arg(step_size)
    m = _mask_int32(mask)
    if labels is None:
        labels = np.unique(m)
        labels = labels[labels > 0]
        if labels.size == 0:
            return None
    table, slot = _lib.drag_label_table(labels)
    if m.size == 0:
        return None
    nv, nt, times = _ctx().marching_cubes(m, table, step)
    marching_cubes_labels.last_times = times
    return list(np.asarray(labels).tolist()), slot, nv, nt


def marching_cubes_labels(mask, labels=None, step_size=1):
    """``{label: (verts, faces)}``: per label the surface of ``mask == label``.  ``verts`` (n, 3) float32
    in ``[z, y, x]`` index coordinates (every coordinate a multiple of ``step_size / 2``), ``faces``
    (m, 3) int32 into them, normals ``cross(v1 - v0, v2 - v0)`` pointing into the label.  ``labels=None``
    means ``np.unique(mask)`` restricted to ``> 0``; a label without a triangle (absent, filling the
    lattice, or an axis shorter than ``step_size + 1``) is left out.  The surface is open where a
    label touches the volume's edge (no padding, as in the reference's call).
    ``marching_cubes_labels.last_times`` holds the device times of the last call."""
    got = _triangulate(mask, labels, step_size)
    if got is None:
        return {}
    labels, slot, nv, nt = got
    if nt.sum() == 0:
        return {}
    meshes = _ctx().surface_fetch(nv, nt)
    return {label: meshes[k] for label, k in zip(labels, slot) if nt[k] > 0}


marching_cubes_labels.last_times = {}
