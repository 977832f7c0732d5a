"""Repo-root shim for the reference ``velocity_analysis`` module (drop-in, in the manner of the root
``physics.py``).

The reference module holds more than the flow analysis: the mesh interface drag stays on the host,
and by default so do ``compute_pressure_field``, ``compute_interface_drag`` and
``compute_permeability_from_pressure``.  When the reference ``velocity_analysis.py`` is on the path
(next to the caller's script), it is loaded under a private name and every one of its names is
re-exported; ``compute_strain_rate``, ``compute_viscous_dissipation``, ``compute_vorticity``,
``compute_permeability`` and ``compute_astarita_flow_type`` (velocity_analysis.py:10-188) are
replaced by the MI355X path, here and inside the reference module.  The four fields are
bit-identical to the reference; the permeability agrees to rounding (its means come from float64
device sums).

With ``PTV_GPU_DRAG=1`` in the environment when this module is imported, ``compute_interface_drag``
(the staircase method, :332-511) and ``compute_permeability_from_pressure`` (:659-697) are replaced
in the same way.  ``method='mesh'`` is forwarded to the reference's ``compute_interface_drag_mesh``;
where that function falls back to the staircase (no scikit-image), the fallback lands on the GPU.
The GPU drag agrees with the reference to the rounding of a reordered sum and adds the keys ``Fx``,
``Fy``, ``Fz`` (``Mx``, ``My``, ``Mz`` with a volume) that the reference's staircase leaves out
(INTEGRATION.md).

With ``PTV_GPU_PRESSURE=1``, independently, ``compute_pressure_field`` (:190-330) is replaced in the
same way.  The GPU pressure agrees with the reference normwise (its force field and right-hand side
bit for bit); it does not need the ``tol=`` keyword that scipy 1.14 removed from
``cg``, which the reference's ``solve_poisson`` still passes.  ``PTV_GPU_PRESSURE_PRECOND=multigrid``
on top of it runs the anchored solve with the multigrid preconditioner; for
``anchor='none'`` it is ignored, with one printed line saying so.

With ``PTV_GPU_DRAG_MESH=1``, independently, ``compute_interface_drag_mesh`` (:513-657) is replaced in
the same way: marching cubes stays on the host (scikit-image is required, there is no staircase
fallback), everything from the mesh onward runs on the GPU.  ``method='mesh'`` then reaches it
through the reference's own dispatch, and with ``PTV_GPU_DRAG=1`` through the forwarding above.
``integrate_mesh_drag`` (the integration for meshes from any source) is always provided.

With ``PTV_GPU_MARCHING_CUBES=1`` as well, the function installed for ``compute_interface_drag_mesh``
calls the GPU one with ``triangulation='device'``: marching cubes runs on the GPU too and scikit-image
is not needed.  Its triangles are those of this project's own rule, not scikit-image's (DESIGN.md
section 23).  The variable has no effect without ``PTV_GPU_DRAG_MESH=1``.

Without the reference module (the GPU box), the five functions, ``analyze``, the two drag functions
above, ``compute_interface_drag_mesh``, ``compute_pressure_field``, ``recover_pressure`` and
``compute_force_field`` are provided.

This module is found instead of the reference's when the repository root precedes the reference's
directory on ``sys.path``.  A script started from inside the reference's directory
(``analyze_flow.py``) has that directory first and keeps importing its own module.
"""
import importlib.util as _ilu
import os as _os
import sys as _sys

from ptv_interpolation_amd import velocity_analysis as _gpu

_NAMES = ("compute_strain_rate", "compute_viscous_dissipation", "compute_vorticity", "compute_permeability",
          "compute_astarita_flow_type")
_DRAG_NAMES = ("compute_interface_drag", "compute_permeability_from_pressure")
_PRESSURE_NAMES = ("compute_pressure_field", "recover_pressure", "compute_force_field")
_ROOT = _os.path.dirname(_os.path.abspath(__file__))


def _reference_module():
    key = "_ptv_reference_velocity_analysis"
    if key in _sys.modules:
        return _sys.modules[key]
    for d in _sys.path:
        d = _os.path.abspath(d or _os.getcwd())
        f = _os.path.join(d, "velocity_analysis.py")
        if d == _ROOT or not _os.path.isfile(f):
            continue
        spec = _ilu.spec_from_file_location(key, f)
        mod = _ilu.module_from_spec(spec)
        _sys.modules[key] = mod
        try:
            spec.loader.exec_module(mod)
        except BaseException:
            del _sys.modules[key]
            raise
        return mod
    return None


_ref = _reference_module()
if _ref is not None:
    globals().update({k: v for k, v in vars(_ref).items() if not k.startswith("__")})
for _n in _NAMES:
    globals()[_n] = getattr(_gpu, _n)
    if _ref is not None:
        setattr(_ref, _n, getattr(_gpu, _n))
analyze = _gpu.analyze


def _drag_with_host_mesh(mesh):
    """The GPU staircase drag with the reference's signature; ``method='mesh'`` goes to the host's
    ``compute_interface_drag_mesh`` as the reference's own dispatch does (:340-342)."""
    def compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, method='staircase', mesh_step=1, volume=None, background_mask=None):
        if method == 'mesh':
            return mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels,
                        mesh_step=mesh_step, volume=volume, background_mask=background_mask)
        return _gpu.compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels, method, mesh_step,
                                           volume, background_mask)
    compute_interface_drag.__doc__ = _gpu.compute_interface_drag.__doc__
    return compute_interface_drag


def _mesh_on_device():
    """The GPU mesh drag with the reference's signature and the triangulation on the device too."""
    def compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, background_mask=None):
        return _gpu.compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels, mesh_step,
                                                volume, background_mask, triangulation='device')
    compute_interface_drag_mesh.__doc__ = _gpu.compute_interface_drag_mesh.__doc__
    return compute_interface_drag_mesh


integrate_mesh_drag = _gpu.integrate_mesh_drag
# before the staircase opt-in, whose method='mesh' forwards to whatever the module holds by then
if _ref is None:
    compute_interface_drag_mesh = _gpu.compute_interface_drag_mesh
elif _os.environ.get("PTV_GPU_DRAG_MESH") == "1":
    compute_interface_drag_mesh = (_mesh_on_device() if _os.environ.get("PTV_GPU_MARCHING_CUBES") == "1"
                                   else _gpu.compute_interface_drag_mesh)
    _ref.compute_interface_drag_mesh = compute_interface_drag_mesh

if _ref is None:
    for _n in _DRAG_NAMES:
        globals()[_n] = getattr(_gpu, _n)
elif _os.environ.get("PTV_GPU_DRAG") == "1":
    _mesh = getattr(_ref, "compute_interface_drag_mesh", None)
    _new = {"compute_interface_drag": _drag_with_host_mesh(_mesh) if _mesh else _gpu.compute_interface_drag,
            "compute_permeability_from_pressure": _gpu.compute_permeability_from_pressure}
    for _n, _f in _new.items():
        globals()[_n] = _f
        setattr(_ref, _n, _f)

if _ref is None:
    for _n in _PRESSURE_NAMES:
        globals()[_n] = getattr(_gpu, _n)
elif _os.environ.get("PTV_GPU_PRESSURE") == "1":
    if _os.environ.get("PTV_GPU_PRESSURE_PRECOND") == "multigrid":
        def compute_pressure_field(u, v, w, dx, dy, dz, mu, rho=0, mask=None, wall_bc='zero-neumann', anchor='outlet',
                                   flow_direction='auto'):
            """The GPU ``compute_pressure_field`` with the multigrid-preconditioned anchored solve;
            ``anchor='none'`` (LSQR) takes no preconditioner and runs as without the switch."""
            pre = 'multigrid'
            if anchor == 'none':
                print("PTV_GPU_PRESSURE_PRECOND=multigrid ignored: anchor='none' is solved by LSQR")
                pre = None
            p = _gpu.compute_pressure_field(u, v, w, dx, dy, dz, mu, rho, mask, wall_bc, anchor, flow_direction,
                                            preconditioner=pre)
            compute_pressure_field.last_stats = _gpu.compute_pressure_field.last_stats
            return p
    else:
        compute_pressure_field = _gpu.compute_pressure_field
    _ref.compute_pressure_field = compute_pressure_field
