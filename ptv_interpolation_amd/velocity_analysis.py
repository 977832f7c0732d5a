"""Drop-in for the flow analysis of the reference ``velocity_analysis`` module (MI355X path).

``compute_strain_rate`` (velocity_analysis.py:10-63), ``compute_viscous_dissipation`` (:65-92),
``compute_vorticity`` (:94-120), ``compute_astarita_flow_type`` (:151-188) and
``compute_permeability`` (:122-149) keep the reference's signatures and return types.  The four
fields come from one HIP stencil kernel (csrc/ptv_flow.hip behind ``ptv_flow_analysis``,
include/ptv_api.h) and are bit-identical to the reference, including numpy's two
division rules for float32 fields (Python-float spacings divide in float32, np.float64 spacings in
float64 with the quotient rounded to float32).  No CPU fallback.

Each per-function wrapper asks the kernel for its own output only.  ``analyze`` is the fused call:
one pass over u, v, w gives the four fields, the statistics the analysis report prints
(analyze_flow.py:335-368) and the permeability; a caller that wants more than one field should use
it.

``compute_permeability`` evaluates the reference's expression on the host from sums the device
accumulates in float64 in a fixed order; np.mean sums pairwise (and in float32 for float32 fields),
so the value agrees with the reference to rounding, not bit for bit.

``compute_pressure_field``, the interface-drag functions and ``compute_permeability_from_pressure``
stay with the reference.
"""
from __future__ import annotations

import numpy as np

from . import _lib, launcher

__all__ = ["compute_strain_rate", "compute_viscous_dissipation", "compute_vorticity", "compute_permeability",
           "compute_astarita_flow_type", "analyze"]

# np.gradient's message for an axis shorter than edge_order + 1
_TOO_SMALL = ("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
              "are required.")


def _field_dtype(arrays, what):
    fts = {a.dtype for a in arrays}
    if len(fts) != 1:
        raise NotImplementedError(f"{what} of mixed dtypes {sorted(map(str, fts))} are not supported on the GPU path")
    return fts.pop()


def _mask_arg(mask, shape):
    """None or a bool array of the fields' shape (the reference's ``~mask`` is bitwise on other dtypes)."""
    if mask is None:
        return None
    mask = np.asarray(mask)
    if mask.dtype != np.bool_:
        raise NotImplementedError(f"mask dtype {mask.dtype} (GPU path: bool, True = fluid, or None)")
    if mask.shape != tuple(shape):
        raise ValueError(f"mask shape {mask.shape} does not match the fields' {tuple(shape)}")
    return mask


def _viscosity_arg(viscosity, ft):
    if np.ndim(viscosity) != 0:
        raise NotImplementedError("viscosity must be a scalar on the GPU path")
    if np.result_type(np.empty(0, dtype=ft), viscosity) != ft:
        raise NotImplementedError(f"a {type(viscosity).__name__} viscosity promotes {ft} fields in the reference; "
                                  "pass a Python float")
    return float(viscosity)


def _stencil_args(u, v, w, dx, dy, dz, mask):
    """Validation shared by the stencil entry points, before any device call.  Returns the fields in
    their compute dtype, the mask, the float spacings and the float32 division rule."""
    u, v, w = (np.asarray(a) for a in (u, v, w))
    if not (u.shape == v.shape == w.shape) or u.ndim != 3:
        raise ValueError(f"u, v and w must share one 3-D shape, got {u.shape}, {v.shape}, {w.shape}")
    ft = _field_dtype((u, v, w), "fields")
    if ft.kind in "biu":
        ft = np.dtype(np.float64)  # np.gradient computes integer arrays as float64
    if ft not in (np.float32, np.float64):
        raise NotImplementedError(f"field dtype {ft} (GPU path: float32 / float64)")
    mask = _mask_arg(mask, u.shape)
    if min(u.shape) < 2:
        raise ValueError(_TOO_SMALL)
    for h in (dx, dy, dz):
        if np.ndim(h) != 0:
            raise NotImplementedError("coordinate-array spacings are not supported on the GPU path (scalars only)")
        if not (np.isfinite(h) and h > 0):
            raise ValueError(f"spacings must be positive and finite, got {h!r}")
    rts = {np.result_type(np.empty(0, dtype=ft), h) for h in (dx, dy, dz)}
    if len(rts) != 1:
        raise NotImplementedError("spacings that promote float32 fields differently per axis "
                                  f"({sorted(map(str, rts))}) are not supported on the GPU path")
    strong = ft == np.float32 and rts.pop() == np.float64
    fields = [a.astype(ft, copy=False) for a in (u, v, w)]
    return fields, mask, (float(dx), float(dy), float(dz)), strong


def _derived_args(arrays, mask):
    arrays = [np.asarray(a) for a in arrays]
    if len({a.shape for a in arrays}) != 1:
        raise ValueError(f"strain rate and vorticity magnitude must share one shape, got {[a.shape for a in arrays]}")
    ft = _field_dtype(arrays, "inputs")
    if ft not in (np.float32, np.float64):
        raise NotImplementedError(f"input dtype {ft} (GPU path: float32 / float64)")
    return arrays, _mask_arg(mask, arrays[0].shape)


def _ctx():
    return _lib.Context.get(launcher.devices()[0])  # PTV_DEVICE, else the first of PTV_DEVICES / all


def _stencil(u, v, w, dx, dy, dz, mask, outputs, viscosity=0.0):
    fields, mask, (dx, dy, dz), strong = _stencil_args(u, v, w, dx, dy, dz, mask)
    if "dissipation" in outputs:
        viscosity = _viscosity_arg(viscosity, fields[0].dtype)
    return _ctx().flow_analysis(*fields, dx, dy, dz, viscosity=viscosity, fluid_mask=mask, outputs=outputs,
                                spacing_strong=strong)


def compute_strain_rate(u, v, w, dx, dy, dz, mask=None):
    """velocity_analysis.py:10-63 on the GPU: the shear-rate magnitude, 0 at solid voxels."""
    return _stencil(u, v, w, dx, dy, dz, mask, ("strain_rate",))[0]["strain_rate"]


def compute_vorticity(u, v, w, dx, dy, dz, mask=None):
    """velocity_analysis.py:94-120 on the GPU: the vorticity magnitude, 0 at solid voxels."""
    return _stencil(u, v, w, dx, dy, dz, mask, ("vorticity",))[0]["vorticity"]


def compute_viscous_dissipation(strain_rate, viscosity, dx=1.0, dy=1.0, dz=1.0, mask=None):
    """velocity_analysis.py:65-92 on the GPU: ``viscosity * strain_rate**2``, 0 at solid voxels.  The
    spacings are unused, as in the reference."""
    (s,), mask = _derived_args((strain_rate,), mask)
    visc = _viscosity_arg(viscosity, s.dtype)
    if s.size == 0:
        return np.empty_like(s)
    return _ctx().flow_derived(s, None, viscosity=visc, fluid_mask=mask, outputs=("dissipation",))[0]["dissipation"]


def compute_astarita_flow_type(strain_rate, vorticity_mag, mask=None):
    """velocity_analysis.py:151-188 on the GPU: (S - O) / (S + O) where S + O > 1e-15, else 0."""
    (s, o), mask = _derived_args((strain_rate, vorticity_mag), mask)
    if s.size == 0:
        return np.empty_like(s)
    return _ctx().flow_derived(s, o, fluid_mask=mask, outputs=("flow_type",))[0]["flow_type"]


def _permeability(sum_u, sum_v, sum_w, sum_dissipation, n, viscosity):
    """velocity_analysis.py:134-149 from the sums over the whole volume."""
    n = np.float64(n)
    u_mean, v_mean, w_mean = (np.float64(s) / n for s in (sum_u, sum_v, sum_w))
    darcy_velocity_mag = np.sqrt(u_mean**2 + v_mean**2 + w_mean**2)
    mean_dissipation = np.float64(sum_dissipation) / n
    if mean_dissipation == 0:
        return 0.0
    return (viscosity * darcy_velocity_mag**2) / mean_dissipation


def compute_permeability(u, v, w, dissipation, viscosity, dx, dy, dz, mask=None):
    """velocity_analysis.py:122-149: k = viscosity * |mean velocity|^2 / mean(dissipation) over the whole
    volume, from the device's float64 sums.  The spacings and the mask are unused, as in the reference."""
    fields, _, _, _ = _stencil_args(u, v, w, 1.0, 1.0, 1.0, None)
    (d,), _ = _derived_args((dissipation,), None)
    if d.shape != fields[0].shape:
        raise ValueError(f"dissipation shape {d.shape} does not match the fields' {fields[0].shape}")
    ctx = _ctx()
    _, st = ctx.flow_analysis(*fields, 1.0, 1.0, 1.0, outputs=())
    _, sd = ctx.flow_derived(d, None, outputs=())
    return _permeability(st["sum_u"], st["sum_v"], st["sum_w"], sd["sum_u"], st["n_voxels"], viscosity)


def analyze(u, v, w, dx, dy, dz, viscosity, mask=None):
    """The fused call: one pass over u, v, w.  Returns a dict with the four fields
    (``strain_rate``, ``dissipation``, ``vorticity``, ``flow_type``), the ``permeability`` and
    ``stats``: the sums of u, v, w, per field its sum (``sum``, and ``sum_fluid`` = the sum of
    ``field[mask]``), ``max`` and ``min``, and the counts ``n_voxels`` and ``n_fluid``."""
    out, st = _stencil(u, v, w, dx, dy, dz, mask, _lib.FLOW_OUTPUTS, viscosity)
    out["permeability"] = _permeability(st["sum_u"], st["sum_v"], st["sum_w"], st["sum"]["dissipation"],
                                        st["n_voxels"], viscosity)
    out["stats"] = st
    return out
