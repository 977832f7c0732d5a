"""Host-side checks of the device marching cubes (no device needed): the struct behind
``ptv_abi_sizes11``, the version and the exported names, the argument validation (before any device
call), the ``triangulation`` keyword of ``compute_interface_drag_mesh`` and the
``PTV_GPU_MARCHING_CUBES`` switch of the repo-root ``velocity_analysis`` shim (probes in subprocesses
over a stand-in layout, as test_mesh_host.py does it).
"""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, surface, velocity_analysis as va

import _mesh_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = (0.7, 1.1, 0.3)
VISC = 1.5e-3


def test_abi_sizes11_and_the_resident_flag():
    c, py = _lib.abi_sizes11()
    assert c == py, (c, py)
    c10, py10 = _lib.abi_sizes10()
    assert c10 == py10
    # the flag follows every older member of ptv_mesh_params
    names = [f[0] for f in _lib.MeshParams._fields_]
    assert names[-2:] == ["tri_offsets", "mesh_resident"]
    assert _lib.MeshParams.mesh_resident.offset > _lib.MeshParams.tri_offsets.offset


def test_version_and_exports():
    src = open(os.path.join(ROOT, "include", "ptv_api.h")).read()
    assert _lib.lib().ptv_version() == int(re.search(r"#define PTV_API_VERSION (\d+)", src).group(1))
    for name in ("ptv_abi_sizes11", "ptv_marching_cubes", "ptv_marching_cubes_dev", "ptv_surface_fetch"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for name in ("marching_cubes", "marching_cubes_dev", "surface_fetch"):
        assert callable(getattr(_lib.Context, name)), name
    assert surface.__all__ == ["marching_cubes_labels"]
    assert str(inspect.signature(surface.marching_cubes_labels)) == "(mask, labels=None, step_size=1)"
    assert surface.marching_cubes_labels.last_times == {} or isinstance(surface.marching_cubes_labels.last_times, dict)


def test_c_validation_needs_no_device():
    fn = _lib.lib().ptv_marching_cubes
    lab = (ctypes.c_int32 * 2)(3, 3)
    prm = _lib.SurfaceParams(4, 4, 4, 1, 2, lab)
    assert fn(None, ctypes.byref(prm), None, None, None, None) == _lib.PTV_E_ARG  # NULL context


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def test_validation_before_any_device_call(no_device):
    m = np.zeros((4, 5, 6), dtype=np.int32)
    m[1:3, 1:3, 1:3] = 2
    for bad in (0, -1, 1.0, 2.5, "2", None, True):
        with pytest.raises(ValueError):
            surface.marching_cubes_labels(m, [2], step_size=bad)
    for bad in (m.astype(np.float32), m.astype(np.float64), m.astype(np.complex64), m.astype(object)):
        with pytest.raises(NotImplementedError):
            surface.marching_cubes_labels(bad, [2])
    big = m.astype(np.int64)
    big[0, 0, 0] = 2**31
    with pytest.raises(NotImplementedError):
        surface.marching_cubes_labels(big, [2])
    with pytest.raises(NotImplementedError):
        surface.marching_cubes_labels(m.astype(np.uint32) + np.uint32(2**31), [2])
    with pytest.raises(ValueError):
        surface.marching_cubes_labels(m[0], [2])
    # the labels: _lib.drag_label_table's rules
    with pytest.raises(ValueError):
        surface.marching_cubes_labels(m, [])
    with pytest.raises(ValueError):
        surface.marching_cubes_labels(m, [[1, 2]])
    for bad in ([0], [-3], [2.0], [2**31]):
        with pytest.raises(NotImplementedError):
            surface.marching_cubes_labels(m, bad)
    # nothing to do is no device call either
    assert surface.marching_cubes_labels(np.zeros((3, 3, 3), dtype=np.int32)) == {}
    assert surface.marching_cubes_labels(np.zeros((0, 3, 3), dtype=np.int32), [1]) == {}


def _inputs(shape=(5, 6, 7)):
    u, v, w, p = mref.make_fields(shape, 0)
    mask = np.zeros(shape, np.int32)
    mask[1:4, 2:5, 2:5] = 1
    return u, v, w, p, mask


def test_triangulation_keyword(no_device):
    u, v, w, p, mask = _inputs()
    # introspection shows the reference's signature (velocity_analysis.py:513)
    assert "triangulation" not in inspect.signature(va.compute_interface_drag_mesh).parameters
    for bad in ("lewiner", "", None, "Device"):
        with pytest.raises(ValueError, match="triangulation"):
            va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, triangulation=bad)
    with pytest.raises(TypeError):  # keyword only: the reference's positional order is untouched
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, None, 1, None, None, 'device')
    # 'device' validates as the default does, then the triangulation's own arguments, then goes to the device
    with pytest.raises(ValueError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask[:, :, :4], triangulation='device')
    with pytest.raises(ValueError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, 0.0, 1.0, 1.0, mask, triangulation='device')
    with pytest.raises(ValueError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, mesh_step=0, triangulation='device')
    with pytest.raises(NotImplementedError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask.astype(float), triangulation='device')
    with pytest.raises(NotImplementedError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, labels=[0], triangulation='device')
    assert va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, np.zeros_like(mask), triangulation='device') == {}
    with pytest.raises(AssertionError, match="device call"):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, triangulation='device')
    # the default is today's host path: scikit-image or ImportError
    try:
        import skimage.measure  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask, triangulation='skimage')


# ---- the shim ----
LAYOUT = """
    def compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, method='staircase', mesh_step=1, volume=None, background_mask=None):
        return "host"
    def compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, background_mask=None):
        return "host mesh"
"""

PROBE = """
    import inspect, sys
    import velocity_analysis as m
    from ptv_interpolation_amd import velocity_analysis as gpu
    ref = sys.modules["_ptv_reference_velocity_analysis"]
    mode = {mode!r}
    seen = []
    real = gpu.compute_interface_drag_mesh
    def spy(*a, **k):
        seen.append(k.get("triangulation", "skimage"))
        return "gpu"
    gpu.compute_interface_drag_mesh = spy
    f = m.compute_interface_drag_mesh
    assert ref.compute_interface_drag_mesh is f
    if mode == "host":
        assert f(*[None] * 9) == "host mesh" and not seen
    elif mode == "skimage":
        assert f is real
    else:
        assert f is not real and f(*[None] * 9, mesh_step=2) == "gpu" and seen == ["device"]
        assert str(inspect.signature(f)) == str(inspect.signature(real))
    print("ok")
"""


@pytest.mark.parametrize("env, mode", [
    ({}, "host"),
    ({"PTV_GPU_MARCHING_CUBES": "1"}, "host"),
    ({"PTV_GPU_DRAG_MESH": "1"}, "skimage"),
    ({"PTV_GPU_DRAG_MESH": "1", "PTV_GPU_MARCHING_CUBES": "0"}, "skimage"),
    ({"PTV_GPU_DRAG_MESH": "1", "PTV_GPU_MARCHING_CUBES": "1"}, "device"),
])
def test_shim_switch(tmp_path, env, mode):
    ref = tmp_path / "layout"
    ref.mkdir()
    (ref / "velocity_analysis.py").write_text(textwrap.dedent(LAYOUT))
    full = dict(os.environ)
    for k in ("PTV_GPU_DRAG", "PTV_GPU_DRAG_MESH", "PTV_GPU_PRESSURE", "PTV_GPU_MARCHING_CUBES"):
        full.pop(k, None)
    full.update(env)
    full["PYTHONPATH"] = ROOT
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(PROBE.format(mode=mode)))
    r = subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {[ROOT, str(ref)]!r}; "
                        f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                       cwd=str(tmp_path), env=full, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
