"""Repo-root shim for the reference ``auto_align`` module (drop-in, see sitecustomize.py).

When the reference ``auto_align.py`` is on the path (next to the caller's script) and importable, it
is loaded under a private name and every one of its names is re-exported; ``find_best_offset``
(auto_align.py:10-62) is replaced by the MI355X version, here and inside the loaded module, so that
its ``main()`` (the command line) reaches the GPU: the distance transform of the solid mask and the
objective run on the device, scipy's Powell search on the host.

The reference module imports ``tifffile`` at the top, which it needs only to load mask files.  On a
machine without it the import fails; the shim then provides ``find_best_offset`` alone, as it does
without the reference module (the GPU box).
"""
import importlib.util as _ilu
import os as _os
import sys as _sys

from ptv_interpolation_amd.alignment import find_best_offset as _gpu_find_best_offset

find_best_offset = _gpu_find_best_offset

_ROOT = _os.path.dirname(_os.path.abspath(__file__))


def _reference_module():
    key = "_ptv_reference_auto_align"
    if key in _sys.modules:
        return _sys.modules[key]
    for d in _sys.path:
        d = _os.path.abspath(d or _os.getcwd())
        f = _os.path.join(d, "auto_align.py")
        if d == _ROOT or not _os.path.isfile(f):
            continue
        spec = _ilu.spec_from_file_location(key, f)
        mod = _ilu.module_from_spec(spec)
        _sys.modules[key] = mod
        try:
            spec.loader.exec_module(mod)
        except ImportError:  # tifffile (or another of its imports) is missing: the function alone
            del _sys.modules[key]
            return None
        except BaseException:
            del _sys.modules[key]
            raise
        return mod
    return None


_ref = _reference_module()
if _ref is not None:
    globals().update({k: v for k, v in vars(_ref).items() if not k.startswith("__")})
    _ref.find_best_offset = _gpu_find_best_offset
    find_best_offset = _gpu_find_best_offset

if __name__ == "__main__":
    if _ref is None:
        raise SystemExit("auto_align: the reference module (and tifffile) is needed for the command line")
    _ref.main()
