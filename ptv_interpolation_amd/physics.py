"""Drop-in for the reference ``physics`` divergence and projection cleaning (MI355X path).

``compute_consistent_divergence(u, v, w, mask, dx, dy, dz)`` (physics.py:6-53) is the
divergence ``view_divergence.py:39,42`` evaluates on the interpolated field and the
divergence-cleaning loop re-evaluates every iteration (physics.py:173, :193-194).  Here it
is one HIP stencil kernel (csrc/ptv_div.hip) behind ``ptv_divergence`` (include/ptv_api.h);
no CPU fallback.  Results are bit-identical to the reference, including numpy's dtype
rules: float32 fields with Python-float spacings give float32; a numpy float64 spacing
(``x[1] - x[0]``, view_divergence.py:22) gives float64 quotients.

``clean_divergence_projection`` (physics.py:149-209), the ``--divergence-free`` step of
main.py, runs on the GPU too: scipy's ``lsqr`` restated matrix-free on the masked 7-point
Laplacian (csrc/ptv_clean.hip behind ``ptv_clean_divergence``), with the fields resident on the
device for the whole call.  ``apply_consistent_correction`` (physics.py:110-147) is bit-identical
to the reference; the solve agrees with the host solver normwise, not bit for bit (its norms are
summed in another order, and thousands of Lanczos steps amplify the last bit).

``clean_divergence_variational`` (physics.py:440-514) runs on the GPU as well: scipy's ``cg`` on
I + lambda D^T D restated matrix-free (csrc/ptv_variational.hip behind ``ptv_clean_variational``;
DESIGN.md §17).  It does not depend on the ``tol=`` keyword that scipy 1.14 removed from ``cg``,
which the reference's call still uses.  The package's own ``clean_divergence`` dispatcher keeps
refusing ``method='variational'``; call ``clean_divergence_variational`` directly, or opt in through
the repo-root shim (``PTV_GPU_CLEAN_VARIATIONAL=1``).

``compute_force_divergence`` (physics.py:211-262) and ``solve_poisson`` (:264-345) run on the GPU
too (csrc/ptv_pressure.hip): the divergence bit-identical, the solve by matrix-free
CG on the symmetric system with the Dirichlet rows and columns eliminated (zero Dirichlet values
only), or by the LSQR above when there is no Dirichlet set.
"""
from __future__ import annotations

import numpy as np

from . import _lib, launcher

__all__ = ["compute_consistent_divergence", "apply_consistent_correction", "clean_divergence_projection",
           "clean_divergence_variational", "clean_divergence", "compute_force_divergence", "solve_poisson"]


def _result_dtype(ft, h):
    """dtype of ``(float array of dtype ft) / h`` under numpy's promotion (NEP 50: Python
    scalars are weak, numpy scalars and 0-d arrays are not)."""
    return np.result_type(np.empty(0, dtype=ft), h)


def compute_consistent_divergence(u, v, w, mask, dx, dy, dz):
    """physics.py:6-53 on the GPU.  ``mask``: True = fluid (required, as in the reference,
    whose np.roll of ``None`` raises AxisError)."""
    if mask is None:
        raise np.exceptions.AxisError("axis 2 is out of bounds for array of dimension 0")
    u, v, w = (np.asarray(a) for a in (u, v, w))
    if not (u.shape == v.shape == w.shape == np.shape(mask)) or u.ndim != 3:
        raise ValueError(f"u, v, w and mask must share one 3-D shape, got {u.shape}, {v.shape}, "
                         f"{w.shape}, {np.shape(mask)}")
    fts = {a.dtype for a in (u, v, w)}
    if len(fts) != 1:
        raise NotImplementedError(f"fields of mixed dtypes {sorted(map(str, fts))} (numpy computes each "
                                  "axis in its own dtype) are not supported on the GPU path")
    ft = fts.pop()
    if ft.kind in "biu":
        # (int + int) / 2.0 is float64 in the reference; exact for |values| < 2**52
        ft = np.dtype(np.float64)
    if ft not in (np.float32, np.float64):
        raise NotImplementedError(f"field dtype {ft} (GPU path: float32 / float64)")
    rts = {_result_dtype(ft, h) for h in (dx, dy, dz)}
    if len(rts) != 1:
        raise NotImplementedError("spacings that promote float32 fields differently per axis "
                                  f"({sorted(map(str, rts))}) are not supported on the GPU path")
    rt = rts.pop()
    ctx = _lib.Context.get(launcher.devices()[0])  # PTV_DEVICE, else the first of PTV_DEVICES / all
    return ctx.divergence(u.astype(ft, copy=False), v.astype(ft, copy=False), w.astype(ft, copy=False),
                          np.asarray(mask).astype(bool, copy=False), float(dx), float(dy), float(dz),
                          result_dtype=rt)


def _clean_args(u, v, w, mask, iterations=0):
    """Validation shared by the cleaning entry points, before any device call."""
    if mask is None:
        raise ValueError("mask is required (True = fluid)")
    if not all(isinstance(a, np.ndarray) for a in (u, v, w)):
        raise NotImplementedError("u, v and w must be numpy arrays (GPU path: float64 (nz, ny, nx))")
    mask = np.asarray(mask)
    if not (u.shape == v.shape == w.shape == mask.shape) or u.ndim != 3:
        raise ValueError(f"u, v, w and mask must share one 3-D shape, got {u.shape}, {v.shape}, "
                         f"{w.shape}, {mask.shape}")
    for a in (u, v, w):
        if a.dtype != np.float64:
            raise NotImplementedError(f"field dtype {a.dtype} (GPU cleaning path: float64)")
    if mask.dtype != np.bool_:
        raise NotImplementedError(f"mask dtype {mask.dtype} (GPU cleaning path: bool, True = fluid)")
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    return mask


def _ctx():
    return _lib.Context.get(launcher.devices()[0])


def apply_consistent_correction(u, v, w, phi, mask, dx, dy, dz):
    """physics.py:110-147 on the GPU: ``phi`` is the compact vector over the fluid voxels (C order),
    as ``lsqr`` returns it.  Bit-identical to the reference."""
    mask = _clean_args(u, v, w, mask)
    phi = np.asarray(phi)
    n_fluid = int(np.count_nonzero(mask))
    if phi.shape != (n_fluid,):
        raise ValueError(f"phi must have one entry per fluid voxel ({n_fluid},), got {phi.shape}")
    if phi.dtype != np.float64:
        raise NotImplementedError(f"phi dtype {phi.dtype} (GPU cleaning path: float64)")
    phi_grid = np.zeros_like(u)
    phi_grid[mask] = phi  # physics.py:116-117
    return _ctx().apply_correction(u, v, w, phi_grid, mask, float(dx), float(dy), float(dz))


def clean_divergence_projection(u, v, w, mask, dx, dy, dz, iterations=3):
    """physics.py:149-209 on the GPU; prints the reference's report (without scipy's own
    ``show=True`` iteration log of the first solve) and returns ``(u_c, v_c, w_c)``."""
    mask = _clean_args(u, v, w, mask, iterations)
    iterations = int(iterations)
    (u_c, v_c, w_c), st = _ctx().clean_divergence(u, v, w, mask, float(dx), float(dy), float(dz),
                                                  iterations=iterations)
    print(f"Starting Iterative Divergence Cleaning ({iterations} iterations)...")
    print(f"  [Initial] Net X-Flux (mid-plane): {st['flux_initial']:.4e}")
    n = st["n_fluid"]
    for i in range(st["n_outer"]):
        print(f"\n--- Iteration {i+1}/{iterations} ---")
        if i < len(st["mean_abs_div"]):
            print(f"  Current Mean Abs Div: {st['mean_abs_div'][i]:.6e}")
        print(f"  Solving Poisson (A: {n}x{n})...")
        if st["nan_stop"] and i == st["n_outer"] - 1:
            print("  Warning: Solve failed. Stopping iterations.")
    m_div_init, m_div_final = st["mean_abs_div"][0], st["mean_abs_div_final"]
    print("\n" + "="*40)
    print("DIVERGENCE CLEANING COMPLETE")
    print(f"Initial Mean Abs Div: {m_div_init:.6e}")
    print(f"Final Mean Abs Div:   {m_div_final:.6e}")
    print(f"Total Reduction:      {np.float64(m_div_init)/np.float64(m_div_final):.2f}x")
    print(f"  [Final] Net X-Flux (mid-plane): {st['flux_final']:.4e}")
    print("="*40 + "\n")
    clean_divergence_projection.last_stats = st
    return u_c, v_c, w_c


def clean_divergence_variational(u, v, w, mask, dx, dy, dz, iterations=1, lambda_reg=1e3):
    """physics.py:440-514 on the GPU: minimises ||U - U0||^2 + lambda ||div U||^2 by CG with the
    reference's ``tol=1e-8, maxiter=2000``; prints the reference's report and returns
    ``(u_c, v_c, w_c)``.  ``iterations`` is unused, as in the reference."""
    mask = _clean_args(u, v, w, mask)
    lam = float(lambda_reg)
    if not np.isfinite(lam):
        raise ValueError(f"lambda_reg must be finite, got {lambda_reg!r}")
    if lam < 0:
        raise NotImplementedError(f"lambda_reg = {lambda_reg!r} < 0: the system is not positive definite")
    (u_c, v_c, w_c), st = _ctx().clean_variational(u, v, w, mask, float(dx), float(dy), float(dz), lambda_reg=lam,
                                                   rtol=1e-8, maxiter=2000)
    n = 3 * st["n_fluid"]
    print(f"Starting Variational Divergence Cleaning (lambda={lambda_reg})...")
    print(f"  Solving Variational System (A: {n}x{n})...")
    if st["info"] > 0:
        print(f"  Warning: CG did not converge after {st['info']} iterations.")
    m_div_init, m_div_final = st["mean_abs_div_initial"], st["mean_abs_div_final"]
    print("\n" + "="*40)
    print("VARIATIONAL CLEANING COMPLETE")
    print(f"Mean Abs Div (Initial): {m_div_init:.6e}")
    print(f"Mean Abs Div (Final):   {m_div_final:.6e}")
    reduction = m_div_init / m_div_final if m_div_final > 0 else float('inf')
    print(f"Total Reduction:        {reduction:.2f}x")
    print("="*40 + "\n")
    clean_divergence_variational.last_stats = st
    return u_c, v_c, w_c


def clean_divergence(u, v, w, mask, dx, dy, dz, iterations=3, method='projection', lambda_reg=1e3):
    """physics.py:347-354: 'projection' runs on the GPU; the variational method stays with the reference."""
    if method == 'variational':
        raise NotImplementedError("method='variational' is not on the GPU path (use the reference's "
                                  "clean_divergence_variational)")
    return clean_divergence_projection(u, v, w, mask, dx, dy, dz, iterations=iterations)


# ---- force divergence and Poisson solve (physics.py:211-345) ----
def _grid_args(arrays, mask, dx, dy, dz, what):
    if mask is None:
        raise ValueError("mask is required (True = fluid)")
    mask = np.asarray(mask)
    arrays = [np.asarray(a) for a in arrays]
    if any(a.shape != mask.shape for a in arrays) or mask.ndim != 3:
        raise ValueError(f"{what} and mask must share one 3-D shape, got {[a.shape for a in arrays]}, {mask.shape}")
    for a in arrays:
        if a.dtype != np.float64:
            raise NotImplementedError(f"field dtype {a.dtype} (GPU pressure path: float64)")
    if mask.dtype != np.bool_:
        raise NotImplementedError(f"mask dtype {mask.dtype} (GPU pressure path: bool, True = fluid)")
    for h in (dx, dy, dz):
        if np.ndim(h) != 0 or not (np.isfinite(h) and h > 0):
            raise ValueError(f"spacings must be positive finite scalars, got {h!r}")
    return arrays, mask


def _wall_bc_arg(wall_bc):
    if wall_bc not in _lib.WALL_BC:
        raise ValueError(f"unknown wall_bc {wall_bc!r} (one of {sorted(_lib.WALL_BC)})")


def compute_force_divergence(fx, fy, fz, mask, dx, dy, dz, wall_bc='zero-neumann'):
    """physics.py:211-262 on the GPU: the face-flux divergence of a force field at every voxel
    (under 'inhomogeneous' solid voxels next to fluid get non-zero values, as in the reference).
    Bit-identical to the reference."""
    (fx, fy, fz), mask = _grid_args((fx, fy, fz), mask, dx, dy, dz, "fx, fy, fz")
    _wall_bc_arg(wall_bc)
    if mask.size == 0:
        return np.zeros(mask.shape)
    return _ctx().force_divergence(fx, fy, fz, mask, float(dx), float(dy), float(dz), wall_bc)


def solve_poisson(source, mask, dx, dy, dz, force_field=None, wall_bc='inhomogeneous', dirichlet_mask=None, dirichlet_values=None,
                  *, preconditioner=None, multigrid=None):
    """physics.py:264-345 on the GPU: Lap(p) = source (or the divergence of ``force_field``) on the
    fluid voxels.  With a ``dirichlet_mask`` the solve is scipy's ``cg(A, b, tol=1e-10,
    maxiter=3000)``, matrix-free; without one, ``lsqr`` on ``b - mean(b)`` with the reference's
    settings.  Only zero Dirichlet values are supported: for other values the reference subtracts
    the Dirichlet column from ``b`` and also keeps it in the matrix, which counts it twice.
    ``preconditioner='multigrid'`` (opt-in) runs the anchored solve as ``cg(A, b, M=...)`` with the
    V-cycle of DESIGN.md §25; ``multigrid`` is a dict of its parameters (max_levels, nu,
    coarse_sweeps, omega), and ``solve_poisson.last_stats['multigrid']`` then holds the hierarchy and
    its times.  Without a ``dirichlet_mask`` it raises ``NotImplementedError``."""
    if preconditioner not in (None, 'multigrid'):
        raise ValueError(f"unknown preconditioner {preconditioner!r} (None or 'multigrid')")
    if preconditioner is None and multigrid is not None:
        raise ValueError("multigrid= needs preconditioner='multigrid'")
    if preconditioner == 'multigrid':
        _lib.mg_params(multigrid)
        if dirichlet_mask is None:
            raise NotImplementedError("preconditioner='multigrid' serves the anchored (CG) solve; without a "
                                      "dirichlet_mask the solve is LSQR, which takes no preconditioner")
    src = (source,) if force_field is None else tuple(force_field)
    if force_field is None and source is None:
        raise ValueError("either source or force_field is required")
    src, mask = _grid_args(src, mask, dx, dy, dz, "the right-hand side")
    _wall_bc_arg(wall_bc)
    dm = None
    if dirichlet_mask is not None:
        dm = np.asarray(dirichlet_mask)
        if dm.shape != mask.shape or dm.dtype != np.bool_:
            raise ValueError(f"dirichlet_mask must be a bool array of shape {mask.shape}")
        if dirichlet_values is not None and np.any(np.asarray(dirichlet_values) != 0):
            raise ValueError("non-zero dirichlet_values are not supported: the reference subtracts the Dirichlet "
                             "column from b and keeps it in the matrix (a double count), which has no oracle")
    if not mask.any():
        return np.zeros(mask.shape)  # physics.py:275-276
    kw = {"rhs": src[0]} if force_field is None else {"force_field": src}
    if preconditioner == 'multigrid':
        x, st = _ctx().poisson_solve_mg(mask, float(dx), float(dy), float(dz), dirichlet=dm, wall_bc=wall_bc,
                                        multigrid=multigrid, **kw)
    else:
        x, st = _ctx().poisson_solve(mask, float(dx), float(dy), float(dz), dirichlet=dm, wall_bc=wall_bc, **kw)
    solve_poisson.last_stats = st
    return x
