"""Repo-root shim for the reference ``physics`` module (drop-in, see sitecustomize.py).

The reference module holds more than the divergence: ``clean_divergence`` (main.py:10),
``solve_poisson`` (velocity_analysis.py:298), the sparse operators and cleaning solvers
(physics.py:55-514), which stay on the host.  When the reference ``physics.py`` is on the
path (next to the caller's script), it is loaded under a private name and every one of its
names is re-exported; only ``compute_consistent_divergence`` (physics.py:6-53) is replaced
by the MI355X kernel, also inside the reference module, so that the cleaning loops
(physics.py:173, :193-194) call the GPU stencil too (bit-identical results).  Without the
reference module (the GPU box), the divergence and the GPU ``compute_force_divergence`` and
``solve_poisson`` (physics.py:211-345) are provided; with the reference module present those two
stay the host's.

Opt-in: with ``PTV_GPU_CLEAN=1`` in the environment, ``clean_divergence_projection`` and
``apply_consistent_correction`` (physics.py:110-209) are replaced the same way, here and inside the
reference module, so that the reference's ``clean_divergence`` dispatcher (and ``main.py -d``)
reaches the GPU solver.  It is not the default because that solver agrees with the host's ``lsqr``
normwise, not bit for bit.

A second, independent opt-in: with ``PTV_GPU_CLEAN_VARIATIONAL=1``, ``clean_divergence_variational``
(physics.py:440-514) is replaced the same way, so that the reference's dispatcher (and ``main.py -d
--cleaning-method variational``) reaches the GPU CG solve.  ``PTV_GPU_CLEAN=1`` alone leaves the
variational method on the host.
"""
import importlib.util as _ilu
import os as _os
import sys as _sys

from ptv_interpolation_amd import physics as _gpu
from ptv_interpolation_amd.physics import compute_consistent_divergence as _gpu_divergence

compute_consistent_divergence = _gpu_divergence
_GPU_CLEAN = _os.environ.get("PTV_GPU_CLEAN", "") == "1"
_GPU_CLEAN_VARIATIONAL = _os.environ.get("PTV_GPU_CLEAN_VARIATIONAL", "") == "1"

_ROOT = _os.path.dirname(_os.path.abspath(__file__))


def _reference_module():
    key = "_ptv_reference_physics"
    if key in _sys.modules:
        return _sys.modules[key]
    for d in _sys.path:
        d = _os.path.abspath(d or _os.getcwd())
        f = _os.path.join(d, "physics.py")
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
    _ref.compute_consistent_divergence = _gpu_divergence
    compute_consistent_divergence = _gpu_divergence
if _GPU_CLEAN:
    clean_divergence_projection = _gpu.clean_divergence_projection
    apply_consistent_correction = _gpu.apply_consistent_correction
    if _ref is not None:
        _ref.clean_divergence_projection = _gpu.clean_divergence_projection
        _ref.apply_consistent_correction = _gpu.apply_consistent_correction
    else:
        clean_divergence = _gpu.clean_divergence
if _GPU_CLEAN_VARIATIONAL:
    clean_divergence_variational = _gpu.clean_divergence_variational
    if _ref is not None:
        _ref.clean_divergence_variational = _gpu.clean_divergence_variational
if _ref is None:
    compute_force_divergence = _gpu.compute_force_divergence
    solve_poisson = _gpu.solve_poisson
