"""Host-side checks of the GPU mesh interface drag and the spline sampling (no device needed): the
structs behind ``ptv_abi_sizes10``, the signatures and exported names, the argument validation
(before any device call), the host assembly of the reference's keys, and the ``PTV_GPU_DRAG_MESH``
opt-in of the repo-root ``velocity_analysis`` shim (probes in subprocesses over a stand-in layout, as
test_drag_host.py does it).
"""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, sampling, velocity_analysis as va

import _mesh_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = (0.7, 1.1, 0.3)
VISC = 1.5e-3


def test_abi_sizes10_match_ctypes():
    c, py = _lib.abi_sizes10()
    assert c == py, (c, py)
    assert _lib.MESH_RECORD.itemsize == py[2] and len(_lib.MESH_KEYS) == 21 and _lib.MESH_KEYS == mref.KEYS


def test_the_capability_probe_is_the_symbol_not_the_version():
    assert _lib.lib().ptv_version() == 11
    for name in ("ptv_abi_sizes10", "ptv_spline_prefilter", "ptv_spline_prefilter_dev", "ptv_map_coordinates",
                 "ptv_map_coordinates_dev", "ptv_mesh_drag", "ptv_mesh_drag_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    for name in ("spline_prefilter", "spline_prefilter_dev", "map_coordinates", "map_coordinates_dev", "mesh_drag",
                 "mesh_drag_dev"):
        assert callable(getattr(_lib.Context, name)), name


def test_signatures_and_names():
    want = ("(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, "
            "background_mask=None)")  # velocity_analysis.py:513
    assert str(inspect.signature(va.compute_interface_drag_mesh)) == want
    assert list(inspect.signature(va.integrate_mesh_drag).parameters)[:11] == [
        "meshes", "u", "v", "w", "pressure", "viscosity", "dx", "dy", "dz", "background_mask", "volume"]
    for name in ("compute_interface_drag_mesh", "integrate_mesh_drag"):
        assert name in va.__all__
    assert sampling.__all__ == ["spline_filter_nearest", "map_coordinates"]


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def _inputs(shape=(5, 6, 7)):
    u, v, w, p = mref.make_fields(shape, 0)
    return u, v, w, p, {1: mref.sphere_mesh((2.0, 2.5, 3.0), 1.5, 1)}


def _drag(meshes, u, v, w, p, h=H, visc=VISC, **kw):
    return va.integrate_mesh_drag(meshes, u, v, w, p, visc, *h, **kw)


def test_validation_fields_and_scalars(no_device):
    u, v, w, p, m = _inputs()
    with pytest.raises(ValueError):
        _drag(m, u, v[:, :, :4], w, p)
    with pytest.raises(ValueError):
        _drag(m, u, v, w, p[:2])
    with pytest.raises(ValueError):
        _drag(m, u[0], v[0], w[0], p[0])
    with pytest.raises(NotImplementedError):
        _drag(m, u.astype(np.complex128), v, w, p)
    with pytest.raises(NotImplementedError):
        _drag(m, u.astype(np.float16).astype(np.longdouble), v, w, p)
    with pytest.raises(ValueError):
        _drag(m, u, v, w, p, background_mask=np.ones((5, 6, 8), bool))
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            _drag(m, u, v, w, p, h=bad)
    with pytest.raises(NotImplementedError):
        _drag(m, u, v, w, p, h=(np.arange(5.0), 1.0, 1.0))
    with pytest.raises(ValueError):
        _drag(m, u, v, w, p, visc=float("nan"))
    with pytest.raises(NotImplementedError):
        _drag(m, u, v, w, p, visc=np.ones(3))


def test_validation_meshes(no_device):
    u, v, w, p, m = _inputs()
    vt, fc = m[1]
    for bad in (vt - 5.0, vt + 5.0, np.where(vt == vt.max(), np.float32(np.nan), vt)):  # outside [0, n - 1]
        with pytest.raises(ValueError):
            _drag({1: (bad.astype(np.float32), fc)}, u, v, w, p)
    edge = vt.copy()
    edge[:, 2] += np.float32(6.0 - vt[:, 2].max() + 2.0 ** -18)  # just past n - 1 on x
    with pytest.raises(ValueError):
        _drag({1: (edge, fc)}, u, v, w, p)
    with pytest.raises(ValueError):
        _drag({1: (vt, fc + len(vt))}, u, v, w, p)
    with pytest.raises(ValueError):
        _drag({1: (vt, -fc - 1)}, u, v, w, p)
    with pytest.raises(ValueError):
        _drag({1: (vt[:, :2], fc)}, u, v, w, p)
    with pytest.raises(NotImplementedError):
        _drag({1: (vt.astype(np.float16), fc)}, u, v, w, p)
    with pytest.raises(NotImplementedError):
        _drag({1: (vt, fc.astype(np.float64))}, u, v, w, p)
    with pytest.raises(NotImplementedError):
        _drag({1: (vt, fc), 2: (vt.astype(np.float64), fc)}, u, v, w, p)
    # nothing to do is no device call either: no label has a triangle
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert _drag({}, u, v, w, p) == {} and _drag({3: none}, u, v, w, p) == {}


def test_compute_interface_drag_mesh_validates_then_needs_skimage(no_device):
    u, v, w, p, _ = _inputs()
    mask = np.zeros(u.shape, np.int32)
    mask[1:4, 2:5, 2:5] = 1
    with pytest.raises(ValueError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask[:, :, :4])
    with pytest.raises(ValueError):
        va.compute_interface_drag_mesh(u, v, w, p, VISC, 0.0, 1.0, 1.0, mask)
    try:
        import skimage.measure  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):  # no staircase fallback
            va.compute_interface_drag_mesh(u, v, w, p, VISC, *H, mask)
    # the package's staircase entry point keeps refusing the method
    with pytest.raises(NotImplementedError):
        va.compute_interface_drag(u, v, w, p, VISC, *H, mask, method="mesh")


def test_sampling_validation(no_device):
    f = np.zeros((3, 4, 5))
    pts = np.zeros((3, 2))
    for kw in (dict(order=2), dict(order=5), dict(mode="reflect"), dict(mode="constant")):
        with pytest.raises(NotImplementedError):
            sampling.map_coordinates(f, pts, **kw)
    with pytest.raises(NotImplementedError):
        sampling.map_coordinates(f[0], pts[:2])
    with pytest.raises(NotImplementedError):
        sampling.map_coordinates(f.astype(np.complex64), pts)
    with pytest.raises(NotImplementedError):
        sampling.spline_filter_nearest(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        sampling.map_coordinates(f, pts[:2])
    with pytest.raises(ValueError):
        sampling.map_coordinates(f, np.full((3, 2), np.nan))
    with pytest.raises(ValueError):
        sampling.map_coordinates(None, pts, order=1, shape=f.shape)
    assert sampling.map_coordinates(f, np.zeros((3, 0))).shape == (0,)


def test_assembly_is_the_references():
    rec = np.zeros(2, dtype=_lib.MESH_RECORD)
    rec["sums"][0] = np.arange(1.0, 22.0)
    rec["sums"][1, 0] = np.nan
    res = va._assemble_mesh([7, 2], rec, volume=2.0)
    assert list(res) == [7, 2]
    r = res[7]
    assert list(r) == list(mref.KEYS) + ["Fx", "Fy", "Fz", "Mx", "My", "Mz"]
    assert r["Fx"] == 1.0 + 10.0 and r["Fz"] == 3.0 + 12.0 and r["My"] == (2.0 + 11.0) / 2.0
    assert np.isnan(res[2]["Fx"]) and np.isnan(res[2]["Mx"]) and res[2]["Fy"] == 0.0
    assert "Mx" not in va._assemble_mesh([1], rec[:1])[1] and "Mx" not in va._assemble_mesh([1], rec[:1], volume=0)[1]


def test_mesh_arrays_concatenate_and_drop_empty_labels():
    u, _, _, _, m = _inputs()
    vt, fc = m[1]
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    labels, verts, faces, off = va._mesh_arrays({4: (vt, fc), 9: none, 2: (vt, fc[:3])}, u.shape)
    assert labels == [4, 2] and off.tolist() == [0, len(fc), len(fc) + 3]
    assert faces[1].min() >= len(vt) and np.array_equal(faces[1] - len(vt), fc[:3])


# ---- the shim ----
LAYOUT = {
    "velocity_analysis": """
        def compute_strain_rate(u, v, w, dx, dy, dz, mask=None): return "host"
        def compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, method='staircase', mesh_step=1, volume=None, background_mask=None):
            if method == 'mesh':
                return compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels,
                                                   mesh_step=mesh_step, volume=volume, background_mask=background_mask)
            return "host"
        def compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, background_mask=None):
            return ("host mesh", mesh_step, volume)
        def compute_permeability_from_pressure(u, v, w, pressure, viscosity, dx, dy, dz): return "host"
    """,
}


def _run(code, tmp_path, env_extra):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in LAYOUT.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    env = dict(os.environ)
    for k in ("PTV_GPU_DRAG", "PTV_GPU_DRAG_MESH", "PTV_GPU_PRESSURE"):
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {[ROOT, str(ref)]!r}; "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)


PROBE = """
    import sys
    import velocity_analysis as m
    from ptv_interpolation_amd import velocity_analysis as gpu
    ref = sys.modules["_ptv_reference_velocity_analysis"]
    swapped = {swapped}
    for mod in (m, ref):
        assert (mod.compute_interface_drag_mesh is gpu.compute_interface_drag_mesh) == swapped
    assert m.integrate_mesh_drag is gpu.integrate_mesh_drag
    def reached_gpu(f):
        try:
            out = f(*[None] * 9, method='mesh', mesh_step=2, volume=3.0)
        except ValueError as e:  # the GPU function's validation rejects the placeholders
            assert "3-D shape" in str(e), e
            return True
        assert out == ("host mesh", 2, 3.0), out
        return False
    # through the reference's own dispatch, and through whatever the shim exports
    assert reached_gpu(ref.compute_interface_drag) == swapped
    assert reached_gpu(m.compute_interface_drag) == swapped
    assert (m.compute_interface_drag.__module__ == "velocity_analysis") == {staircase}
    print("ok")
"""


@pytest.mark.parametrize("env, swapped, staircase", [
    ({}, False, False),
    ({"PTV_GPU_DRAG": "1"}, False, True),
    ({"PTV_GPU_DRAG_MESH": "1"}, True, False),
    ({"PTV_GPU_DRAG_MESH": "1", "PTV_GPU_DRAG": "1"}, True, True),
    ({"PTV_GPU_DRAG_MESH": "0", "PTV_GPU_PRESSURE": "1"}, False, False),
])
def test_shim_opt_in(tmp_path, env, swapped, staircase):
    r = _run(PROBE.format(swapped=swapped, staircase=staircase), tmp_path, env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_exports_the_names_without_the_reference():
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("PTV_GPU_DRAG_MESH", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(f"""
        import sys
        sys.path[:] = [p for p in sys.path if p]
        sys.path.insert(0, {ROOT!r})
        import velocity_analysis as m
        for n in ("compute_interface_drag_mesh", "integrate_mesh_drag"):
            assert getattr(m, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        print("ok")
    """)], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
