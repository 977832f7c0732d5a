"""Repo-root shim for the reference ``velocity_analysis`` module (drop-in, in the manner of the root
``physics.py``).

The reference module holds more than the flow analysis: ``compute_pressure_field``, the
interface-drag functions and ``compute_permeability_from_pressure`` stay on the host.  When the
reference ``velocity_analysis.py`` is on the path (next to the caller's script), it is loaded under
a private name and every one of its names is re-exported; ``compute_strain_rate``,
``compute_viscous_dissipation``, ``compute_vorticity``, ``compute_permeability`` and
``compute_astarita_flow_type`` (velocity_analysis.py:10-188) are replaced by the MI355X path, here
and inside the reference module.  The four fields are bit-identical to the reference; the
permeability agrees to rounding (its means come from float64 device sums).  Without
the reference module (the GPU box), only the five functions and ``analyze`` are provided.

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
