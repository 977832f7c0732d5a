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

``compute_interface_drag`` (:332-511, ``method='staircase'``) and
``compute_permeability_from_pressure`` (:659-697) consume a pressure field from any source.  The
drag comes from one pass over the label mask (csrc/ptv_drag.hip behind ``ptv_interface_drag``;
DESIGN.md §19): the device returns a face count and four float64 sums per (label, axis, direction),
the host assembles the reference's keys from them in the reference's order.  ``Area`` equals the
reference bit for bit; the force keys agree to the rounding of a reordered float64 sum (float32
fields are widened on load, so they are summed more accurately than the reference's float32 sums).
The result always carries ``Fx``, ``Fy``, ``Fz`` (and ``Mx``, ``My``, ``Mz`` with a ``volume``),
which the reference's staircase leaves out.  The permeability is the reference's expression of the
device's float64 sums of u, v, w and of ``np.gradient(pressure)``'s components.

``compute_pressure_field`` (:190-330) runs on the GPU as one resident chain (csrc/ptv_pressure.hip
behind ``ptv_pressure_recover``): the mask-aware Laplacian with its two fill rounds,
the force field, the force divergence and the Poisson solve, CG for an anchored solve and the LSQR
of the projection cleaning for ``anchor='none'``.  The force field and the divergence are
bit-identical to the reference; the pressure agrees normwise (a Krylov solve summed in another
order).  Two extensions: ``mask=None`` means all fluid (the reference raises on it in every
branch), and float32 fields are widened exactly and computed in float64, so the result is float64
(the reference would compute them in float32).  ``recover_pressure`` is the same computation with
the solver settings exposed and the statistics returned; ``compute_force_field`` stops after the
force field.

``compute_interface_drag_mesh`` (:513-657) keeps its triangulation on the host
(``skimage.measure.marching_cubes`` per label, ``ImportError`` without scikit-image) and integrates
on the GPU (csrc/ptv_mesh.hip behind ``ptv_mesh_drag``): each of u, v, w goes through
one cubic B-spline prefilter whose coefficients stay in HBM, and all labels' triangles through one
launch that takes the order-3, order-1 and order-0 samples and forms the reference's 21 sums per
label in a fixed order.  ``integrate_mesh_drag`` is that integration for meshes from any source.
The sums agree with the reference to rounding (the bar of tests/test_gpu_mesh.py); float32 and
integer fields are widened exactly and computed in float64.  ``compute_interface_drag`` keeps
raising ``NotImplementedError`` for ``method='mesh'``: the root shim's ``PTV_GPU_DRAG_MESH=1`` routes
that method here.
"""
from __future__ import annotations

import inspect

import numpy as np

from . import _lib, launcher

__all__ = ["compute_strain_rate", "compute_viscous_dissipation", "compute_vorticity", "compute_permeability",
           "compute_astarita_flow_type", "analyze", "compute_interface_drag", "compute_permeability_from_pressure",
           "compute_pressure_field", "recover_pressure", "compute_force_field", "integrate_mesh_drag",
           "compute_interface_drag_mesh"]

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


# ---- interface drag (velocity_analysis.py:332-511) ----
_DRAG_KEYS = ("Fx_v", "Fy_v", "Fz_v", "Fx_v_tan", "Fy_v_tan", "Fz_v_tan", "Fx_v_nor", "Fy_v_nor", "Fz_v_nor",
              "Fx_p", "Fy_p", "Fz_p", "Area")
_INT32 = np.iinfo(np.int32)


def _scalar_args(dx, dy, dz, viscosity):
    for h in (dx, dy, dz):
        if np.ndim(h) != 0:
            raise NotImplementedError("coordinate-array spacings are not supported on the GPU path (scalars only)")
        if not (np.isfinite(h) and h > 0):
            raise ValueError(f"spacings must be positive and finite, got {h!r}")
    if np.ndim(viscosity) != 0:
        raise NotImplementedError("viscosity must be a scalar on the GPU path")
    if not np.isfinite(viscosity):
        raise ValueError(f"viscosity must be finite, got {viscosity!r}")


def _drag_fields(u, v, w, pressure):
    """u, v, w and the pressure (or None) in one compute dtype, float32 or float64."""
    fields = [np.asarray(a) for a in (u, v, w)] + ([] if pressure is None else [np.asarray(pressure)])
    if len({a.shape for a in fields}) != 1 or fields[0].ndim != 3:
        raise ValueError(f"u, v, w and the pressure must share one 3-D shape, got {[a.shape for a in fields]}")
    ft = _field_dtype(fields, "fields")
    if ft.kind in "biu":
        ft = np.dtype(np.float64)  # numpy computes integer arrays as float64
    if ft not in (np.float32, np.float64):
        raise NotImplementedError(f"field dtype {ft} (GPU path: float32 / float64)")
    return [a.astype(ft, copy=False) for a in fields]


def _drag_mask(mask, shape):
    """The label mask as int32: bool or any integer dtype whose values fit."""
    mask = np.asarray(mask)
    if mask.shape != tuple(shape):
        raise ValueError(f"mask shape {mask.shape} does not match the fields' {tuple(shape)}")
    if mask.dtype.kind not in "biu":
        raise NotImplementedError(f"mask dtype {mask.dtype} (GPU path: bool or an integer dtype)")
    if mask.dtype.kind != "b" and mask.dtype.itemsize >= 4 and mask.dtype != np.int32 and mask.size:
        if mask.max() > _INT32.max or mask.min() < _INT32.min:
            raise NotImplementedError("mask values outside the int32 range are not supported on the GPU path")
    return mask


def _assemble_drag(labels, records, dx, dy, dz, volume=None, has_pressure=True):
    """The reference's result dict from one record per (given label, axis, direction), accumulated
    in the reference's order: axis 0, 1, 2; the labels as given; direction A, then B.  ``records``
    is indexable as ``records[i, axis, direction]`` with fields count, sum_p, sum_u, sum_v, sum_w."""
    results = {}
    for label in labels:
        results[label] = dict.fromkeys(_DRAG_KEYS, 0.0)
    dA = [dy * dx, dz * dx, dz * dy]
    for axis in range(3):
        area = dA[axis]
        normal = "zyx"[axis]
        for i, label in enumerate(labels):
            r = results[label]
            for direction in range(2):
                rec = records[i, axis, direction]
                if rec["count"] == 0:  # the reference's np.any(idx)
                    continue
                r["Area"] += rec["count"] * area
                if has_pressure:
                    r[f"F{normal}_p"] += rec["sum_p"]
                for comp, s in (("x", rec["sum_u"]), ("y", rec["sum_v"]), ("z", rec["sum_w"])):
                    r[f"F{comp}_v"] -= s
                    r[f"F{comp}_v_" + ("nor" if comp == normal else "tan")] -= s
    for r in results.values():
        # the mesh method's definitions (:647-655); the reference's staircase leaves them out
        for c in "xyz":
            r[f"F{c}"] = r[f"F{c}_v"] + r[f"F{c}_p"]
        if volume:
            for c in "xyz":
                r[f"M{c}"] = r[f"F{c}"] / volume
    return results


def compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, method='staircase', mesh_step=1, volume=None, background_mask=None):
    """velocity_analysis.py:332-511 on the GPU: the staircase drag on every interface between the
    fluid (mask == 0) and each positive label, a dict of dicts keyed by label.  ``mesh_step`` and
    ``background_mask`` are unused, as in the reference's staircase.  ``Fx``, ``Fy``, ``Fz`` are
    always present, ``Mx``, ``My``, ``Mz`` with a truthy ``volume``."""
    if method == "mesh":
        raise NotImplementedError("method='mesh' (marching cubes) stays on the host: "
                                  "the reference's compute_interface_drag_mesh")
    if method != "staircase":
        raise ValueError(f"unknown method {method!r} (GPU path: 'staircase')")
    fields = _drag_fields(u, v, w, pressure)
    mask = _drag_mask(mask, fields[0].shape)
    _scalar_args(dx, dy, dz, viscosity)
    if labels is None:
        labels = np.unique(mask)
        labels = labels[labels > 0]
    if len(labels) == 0:
        return {}
    _, slot = _lib.drag_label_table(labels)
    if mask.size == 0:
        records = np.zeros((len(slot), 3, 2), dtype=_lib.DRAG_RECORD)
    else:
        records, _ = _ctx().interface_drag(mask, fields[0], fields[1], fields[2],
                                           fields[3] if pressure is not None else None, float(viscosity),
                                           float(dx), float(dy), float(dz), labels)
    return _assemble_drag(labels, records, dx, dy, dz, volume, has_pressure=pressure is not None)


# ---- permeability from the pressure gradient (velocity_analysis.py:659-697) ----
def _permeability_from_pressure(sum_u, sum_v, sum_w, sum_gx, sum_gy, sum_gz, n, viscosity):
    """velocity_analysis.py:673-697 from the sums over the whole volume of u, v, w and of the
    x, y, z components of the pressure gradient."""
    n = np.float64(n)
    U0_vec = np.array([np.float64(s) / n for s in (sum_u, sum_v, sum_w)])
    grad_P_vec = np.array([np.float64(s) / n for s in (sum_gx, sum_gy, sum_gz)])
    grad_P_mag2 = np.sum(grad_P_vec**2)
    if grad_P_mag2 == 0:
        return 0.0
    return -viscosity * np.dot(U0_vec, grad_P_vec) / grad_P_mag2


def compute_permeability_from_pressure(u, v, w, pressure, viscosity, dx, dy, dz):
    """velocity_analysis.py:659-697: k = -viscosity * (U0 . G) / |G|^2 with U0 the mean velocity and
    G the mean of np.gradient(pressure, dz, dy, dx), from the device's float64 sums."""
    fields, _, (hx, hy, hz), strong = _stencil_args(u, v, w, dx, dy, dz, None)
    p = np.asarray(pressure)
    if p.shape != fields[0].shape:
        raise ValueError(f"pressure shape {p.shape} does not match the fields' {fields[0].shape}")
    if p.dtype.kind in "biu":
        p = p.astype(np.float64)
    if p.dtype != fields[0].dtype:
        raise NotImplementedError(f"fields of mixed dtypes {sorted(map(str, {p.dtype, fields[0].dtype}))} are not "
                                  "supported on the GPU path")
    if np.ndim(viscosity) != 0:
        raise NotImplementedError("viscosity must be a scalar on the GPU path")
    ctx = _ctx()
    _, st = ctx.flow_analysis(*fields, hx, hy, hz, outputs=())
    gz, gy, gx = ctx.gradient_sums(p, hx, hy, hz, spacing_strong=strong)
    return _permeability_from_pressure(st["sum_u"], st["sum_v"], st["sum_w"], gx, gy, gz, st["n_voxels"], viscosity)


# ---- pressure recovery (velocity_analysis.py:190-330) ----
def _pressure_args(u, v, w, dx, dy, dz, mu, rho, mask):
    """Validation shared by the pressure entry points, before any device call: the fields as
    float64 (float32 and integer fields widen exactly), the mask as bool (None = all fluid)."""
    u, v, w = (np.asarray(a) for a in (u, v, w))
    if not (u.shape == v.shape == w.shape) or u.ndim != 3:
        raise ValueError(f"u, v and w must share one 3-D shape, got {u.shape}, {v.shape}, {w.shape}")
    for a in (u, v, w):
        if a.dtype.kind not in "biuf" or a.dtype.itemsize > 8:
            raise NotImplementedError(f"field dtype {a.dtype} (GPU path: float32 / float64)")
    if mask is None:
        mask = np.ones(u.shape, dtype=bool)
    mask = _mask_arg(mask, u.shape)
    _scalar_args(dx, dy, dz, mu)
    if np.ndim(rho) != 0 or not np.isfinite(rho):
        raise ValueError(f"rho must be a finite scalar, got {rho!r}")
    if rho > 0 and min(u.shape) < 2:
        raise ValueError(_TOO_SMALL)
    return [a.astype(np.float64, copy=False) for a in (u, v, w)], mask


def _solve_args(wall_bc, anchor):
    if wall_bc not in _lib.WALL_BC:
        raise ValueError(f"unknown wall_bc {wall_bc!r} (one of {sorted(_lib.WALL_BC)})")
    if anchor not in _lib.ANCHOR:
        raise ValueError(f"unknown anchor {anchor!r} (one of {sorted(_lib.ANCHOR)})")


def compute_force_field(u, v, w, dx, dy, dz, mu, rho=0, mask=None):
    """velocity_analysis.py:210-289 on the GPU: ``mu * laplacian_mask_aware(vel)``, minus
    ``rho * (vel . grad) vel`` for ``rho > 0``; returns ``(fx, fy, fz)``, float64, bit-identical to
    the reference at every voxel."""
    fields, mask = _pressure_args(u, v, w, dx, dy, dz, mu, rho, mask)
    if mask.size == 0:
        return tuple(np.zeros(mask.shape) for _ in range(3))
    f, st = _ctx().force_field(*fields, mask, float(dx), float(dy), float(dz), float(mu), float(rho))
    compute_force_field.last_stats = st
    return f


def recover_pressure(u, v, w, dx, dy, dz, mu, rho=0, mask=None, wall_bc='zero-neumann', anchor='outlet',
                     flow_direction='auto', rtol=1e-10, maxiter=3000, *, preconditioner=None, multigrid=None):
    """``compute_pressure_field`` without the report, with the CG settings exposed; returns
    ``(p, stats)``.  ``stats`` carries ``itn``, ``info`` (CG: scipy's; ``anchor='none'``: lsqr's
    istop), ``bnorm``, ``rnorm``, the sums of |fx|, |fy|, |fz| and w over the fluid voxels,
    ``n_fluid``, ``n_dirichlet``, ``anchor_plane`` and the device times.
    ``preconditioner='multigrid'`` runs the anchored solve as scipy's ``cg(A, b, M=...)`` with the
    V-cycle of DESIGN.md §25 (``multigrid``: a dict of max_levels, nu, coarse_sweeps, omega; the
    stats then carry a ``multigrid`` dict); with ``anchor='none'`` it raises ``NotImplementedError``."""
    fields, mask = _pressure_args(u, v, w, dx, dy, dz, mu, rho, mask)
    _solve_args(wall_bc, anchor)
    if preconditioner not in (None, 'multigrid'):
        raise ValueError(f"unknown preconditioner {preconditioner!r} (None or 'multigrid')")
    if preconditioner is None and multigrid is not None:
        raise ValueError("multigrid= needs preconditioner='multigrid'")
    if preconditioner == 'multigrid':
        _lib.mg_params(multigrid)
        if anchor == 'none':
            raise NotImplementedError("preconditioner='multigrid' serves the anchored (CG) solve; anchor='none' "
                                      "is solved by LSQR, which takes no preconditioner")
    if not np.isfinite(rtol) or int(maxiter) != maxiter or maxiter < 0:
        raise ValueError(f"rtol must be finite and maxiter an integer >= 0, got {rtol!r}, {maxiter!r}")
    if flow_direction not in ("positive", "negative"):
        flow_direction = "auto"  # the reference's else branch (:310)
    if mask.size == 0:
        return np.zeros(mask.shape), {"n_fluid": 0}
    if preconditioner == 'multigrid':
        return _ctx().pressure_recover_mg(*fields, mask, float(dx), float(dy), float(dz), float(mu), float(rho),
                                          wall_bc, anchor, flow_direction, multigrid=multigrid, rtol=float(rtol),
                                          maxiter=int(maxiter))
    return _ctx().pressure_recover(*fields, mask, float(dx), float(dy), float(dz), float(mu), float(rho), wall_bc,
                                   anchor, flow_direction, rtol=float(rtol), maxiter=int(maxiter))


def compute_pressure_field(u, v, w, dx, dy, dz, mu, rho=0, mask=None, wall_bc='zero-neumann', anchor='outlet', flow_direction='auto',
                           *, preconditioner=None, multigrid=None):
    """velocity_analysis.py:190-330 on the GPU: the relative pressure from the pressure Poisson
    equation; prints the reference's report.  ``mask=None`` means all fluid; the result is float64.
    ``preconditioner`` and ``multigrid`` as in ``recover_pressure``."""
    p, st = recover_pressure(u, v, w, dx, dy, dz, mu, rho, mask, wall_bc, anchor, flow_direction,
                             preconditioner=preconditioner, multigrid=multigrid)
    print(f"Computing pressure field source term (mu={mu}, rho={rho}, wall_bc={wall_bc}, flow={flow_direction})...")
    n = np.float64(st["n_fluid"])
    with np.errstate(invalid="ignore"):  # a mask without fluid: the reference's means of nothing are NaN
        means = [np.float64(st.get(k, 0.0)) / n for k in ("sum_abs_fx", "sum_abs_fy", "sum_abs_fz")]
    print(f"  Force field stats (SI):")
    print(f"    Fx: mean={means[0]: .4e}")
    print(f"    Fy: mean={means[1]: .4e}")
    print(f"    Fz: mean={means[2]: .4e}")
    print(f"Solving pressure Poisson equation (anchor={anchor} at Z-plane, dir={flow_direction})...")
    compute_pressure_field.last_stats = st
    return p


# ---- mesh interface drag (velocity_analysis.py:513-657) ----
def _mesh_fields(u, v, w, pressure, background_mask):
    """u, v, w and the pressure (or None) as float64 (float32 and integer fields widen exactly), the
    background mask (or None) as the uint8 grid of ``background_mask.astype(float) > 0.5``."""
    fields = [np.asarray(a) for a in (u, v, w)] + ([] if pressure is None else [np.asarray(pressure)])
    if len({a.shape for a in fields}) != 1 or fields[0].ndim != 3:
        raise ValueError(f"u, v, w and the pressure must share one 3-D shape, got {[a.shape for a in fields]}")
    for a in fields:
        if a.dtype.kind not in "biuf" or a.dtype.itemsize > 8:
            raise NotImplementedError(f"field dtype {a.dtype} (GPU path: float32 / float64)")
    if fields[0].size == 0:
        raise ValueError("the fields have no voxels")
    bg = None
    if background_mask is not None:
        bg = np.asarray(background_mask)
        if bg.shape != fields[0].shape:
            raise ValueError(f"background_mask shape {bg.shape} does not match the fields' {fields[0].shape}")
        if bg.dtype.kind not in "biuf":
            raise NotImplementedError(f"background_mask dtype {bg.dtype}")
        bg = (bg.astype(float) > 0.5).view(np.uint8)
    return [a.astype(np.float64, copy=False) for a in fields], bg


def _mesh_arrays(meshes, shape):
    """The labels that have triangles, their vertices and faces concatenated (faces shifted to the
    concatenated vertices) and the per-label triangle offsets."""
    labels, verts, faces, offsets, base = [], [], [], [0], 0
    hi = np.asarray(shape, dtype=np.float64) - 1.0
    for label, (vt, fc) in meshes.items():
        vt, fc = np.asarray(vt), np.asarray(fc)
        if fc.size == 0:
            continue  # the reference's `continue` for a label without a surface
        if vt.ndim != 2 or vt.shape[1] != 3 or fc.ndim != 2 or fc.shape[1] != 3:
            raise ValueError(f"label {label!r}: verts (n, 3) and faces (m, 3), got {vt.shape} and {fc.shape}")
        if vt.dtype not in (np.float32, np.float64):
            raise NotImplementedError(f"label {label!r}: vertex dtype {vt.dtype} (GPU path: float32 / float64)")
        if fc.dtype.kind not in "iu":
            raise NotImplementedError(f"label {label!r}: face dtype {fc.dtype} (GPU path: integers)")
        if fc.min() < 0 or fc.max() >= len(vt):
            raise ValueError(f"label {label!r}: a face index lies outside the {len(vt)} vertices")
        used = vt[np.unique(fc)]
        if not (np.all(used >= 0.0) and np.all(used <= hi)):  # also rejects NaN
            raise ValueError(f"label {label!r}: vertices outside the volume [0, n - 1] (marching cubes produces none)")
        labels.append(label)
        verts.append(vt)
        faces.append(fc.astype(np.int64) + base)
        base += len(vt)
        offsets.append(offsets[-1] + len(fc))
    if len({vt.dtype for vt in verts}) > 1:
        raise NotImplementedError("meshes of mixed vertex dtypes are not supported on the GPU path")
    if base >= 2**31:
        raise NotImplementedError("2^31 or more vertices are not supported on the GPU path")
    return labels, verts, faces, np.asarray(offsets, dtype=np.int64)


def _assemble_mesh(labels, records, volume=None):
    """The reference's result dict (:620-655) from one MESH_RECORD per label."""
    results = {}
    for label, rec in zip(labels, records):
        r = {k: np.float64(s) for k, s in zip(_lib.MESH_KEYS, rec["sums"])}
        for c in "xyz":
            r[f"F{c}"] = r[f"F{c}_v"] + r[f"F{c}_p"]
        if volume:
            for c in "xyz":
                r[f"M{c}"] = r[f"F{c}"] / volume
        results[label] = r
    return results


def integrate_mesh_drag(meshes, u, v, w, pressure, viscosity, dx, dy, dz, background_mask=None, volume=None,
                        resident=False):
    """velocity_analysis.py:547-655 on the GPU: the drag on triangulated interfaces.  ``meshes`` maps a
    label to ``(verts, faces)``: vertices (n, 3) in voxel-index coordinates ``[z, y, x]``, float32
    (skimage's) or float64, inside ``[0, n - 1]`` on every axis (``ValueError`` otherwise), and
    integer faces (m, 3).  Returns the reference's dict of dicts: its 21 sums, ``Fx``, ``Fy``,
    ``Fz``, and ``Mx``, ``My``, ``Mz`` with a truthy ``volume``; a label without triangles is left
    out.  The fields are filtered once per call and all labels' triangles go through one launch.
    ``resident=True``: u, v, w, the pressure and the background mask are the previous call's, still in
    the context with their coefficients (only their shape is read here): no upload, no prefilter.
    ``integrate_mesh_drag.last_times`` holds the device times of the last call."""
    fields, bg = _mesh_fields(u, v, w, pressure, background_mask)
    _scalar_args(dx, dy, dz, viscosity)
    shape = fields[0].shape
    labels, verts, faces, offsets = _mesh_arrays(meshes, shape)
    if not labels:
        return {}
    vt, fc = np.concatenate(verts), np.concatenate(faces).astype(np.int32)
    if resident:
        records, times = _ctx().mesh_drag(None, None, None, vt, fc, offsets, float(viscosity), float(dx), float(dy),
                                          float(dz), shape=shape)
    else:
        records, times = _ctx().mesh_drag(fields[:3], fields[3] if pressure is not None else None, bg, vt, fc, offsets,
                                          float(viscosity), float(dx), float(dy), float(dz))
    integrate_mesh_drag.last_times = times
    return _assemble_mesh(labels, records, volume)


def compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, background_mask=None, *, triangulation='skimage'):
    """velocity_analysis.py:513-657 with the integration on the GPU; ``integrate_mesh_drag`` is
    everything from the mesh onward.  ``triangulation`` (keyword only, an addition to the reference's
    signature) says where the mesh comes from:

    ``'skimage'`` (the default): ``skimage.measure.marching_cubes`` per label on the host
    (``ImportError`` without scikit-image; this package has no staircase fallback), run on the label's
    bounding box grown by one voxel and shifted back (the same surface as the full-volume call's, at a
    fraction of its cost).

    ``'device'``: ``surface.marching_cubes_labels``' kernels triangulate all labels in one pass and the
    traction kernel reads the mesh where they left it (no download, no upload).  The triangles are
    those of the project's own rule, not scikit-image's: the two surfaces
    separate the same voxels and differ in how ambiguous faces and polygons are cut.

    Anything else raises ``ValueError``."""
    if triangulation not in ("skimage", "device"):
        raise ValueError(f"unknown triangulation {triangulation!r} (one of 'skimage', 'device')")
    fields, bg = _mesh_fields(u, v, w, pressure, background_mask)
    _scalar_args(dx, dy, dz, viscosity)
    mask = np.asarray(mask)
    if mask.shape != fields[0].shape:
        raise ValueError(f"mask shape {mask.shape} does not match the fields' {fields[0].shape}")
    if triangulation == "device":
        from . import surface

        got = surface._triangulate(mask, labels, mesh_step)
        if got is None or got[3].sum() == 0:
            return {}
        given, slot, _, n_tris = got
        records, times = _ctx().mesh_drag(fields[:3], fields[3] if pressure is not None else None, bg, None, None,
                                          None, float(viscosity), float(dx), float(dy), float(dz),
                                          resident_labels=len(n_tris))
        integrate_mesh_drag.last_times = dict(times, **surface.marching_cubes_labels.last_times)
        keep = [(label, k) for label, k in zip(given, slot) if n_tris[k] > 0]  # the reference's `continue`
        return _assemble_mesh([label for label, _ in keep], records[[k for _, k in keep]], volume)
    from skimage import measure

    if labels is None:
        labels = np.unique(mask)
        labels = labels[labels > 0]
    meshes = {}
    for label in labels:
        where = np.nonzero(mask == label)
        if where[0].size == 0:
            continue
        lo = [max(int(i.min()) - 1, 0) for i in where]
        hi = [min(int(i.max()) + 2, n) for i, n in zip(where, mask.shape)]
        box = (mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == label).astype(float)
        try:
            vt, fc, _, _ = measure.marching_cubes(box, level=0.5, step_size=mesh_step)
        except (ValueError, RuntimeError):
            continue
        meshes[label] = (vt + np.asarray(lo, dtype=vt.dtype), fc)
    return integrate_mesh_drag(meshes, u, v, w, pressure, viscosity, dx, dy, dz, background_mask=background_mask,
                               volume=volume)


# Introspection reports the reference's signature (velocity_analysis.py:513): the root shim installs
# this function in the reference's place, and callers that compare signatures see the drop-in.  The
# keyword-only ``triangulation`` is accepted on top of it, as the docstring says.
compute_interface_drag_mesh.__signature__ = inspect.Signature(
    [q for q in inspect.signature(compute_interface_drag_mesh).parameters.values() if q.name != "triangulation"])
