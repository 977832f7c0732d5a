"""Host-side checks of the GPU interface drag and the pressure-based permeability (no device
needed): the structs behind ``ptv_abi_sizes7``, the signatures, the argument validation (before any
device call), the host assembly of the reference's keys from per-(label, axis, direction) records,
the permeability expression, and the ``PTV_GPU_DRAG`` opt-in of the repo-root ``velocity_analysis``
shim (probes in subprocesses over a stand-in layout, as test_flow_host.py does it).
"""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, velocity_analysis as va

import _drag_ref as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
H = (0.3, 1.1, 0.7)
VISC = 1.5e-3


def test_abi_sizes7_match_ctypes():
    c, py = _lib.abi_sizes7()
    assert c == py, (c, py)
    assert _lib.DRAG_RECORD.itemsize == py[1]


def test_the_capability_probe_is_the_symbol_not_the_version():
    assert _lib.lib().ptv_version() == 11
    for name in ("ptv_abi_sizes7", "ptv_interface_drag", "ptv_interface_drag_dev", "ptv_gradient_sums",
                 "ptv_gradient_sums_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    for name in ("interface_drag", "interface_drag_dev", "gradient_sums", "gradient_sums_dev"):
        assert callable(getattr(_lib.Context, name)), name


def test_signatures_are_the_references():
    want = {  # velocity_analysis.py:332, :659
        "compute_interface_drag": "(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, "
                                  "method='staircase', mesh_step=1, volume=None, background_mask=None)",
        "compute_permeability_from_pressure": "(u, v, w, pressure, viscosity, dx, dy, dz)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(va, name))) == sig, name
        assert name in va.__all__


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def _inputs(shape=(3, 4, 5), dtype=np.float64):
    rng = np.random.default_rng(0)
    u, v, w, p = (rng.standard_normal(shape).astype(dtype) for _ in range(4))
    mask = (rng.random(shape) < 0.4).astype(np.int32)
    return u, v, w, p, mask


def _drag(u, v, w, p, mask, h=H, visc=VISC, **kw):
    return va.compute_interface_drag(u, v, w, p, visc, *h, mask, **kw)


def test_drag_validation_shapes_and_dtypes(no_device):
    u, v, w, p, mask = _inputs()
    with pytest.raises(ValueError):
        _drag(u, v[:, :, :4], w, p, mask)
    with pytest.raises(ValueError):
        _drag(u, v, w, p[:2], mask)
    with pytest.raises(ValueError):
        _drag(u[0], v[0], w[0], p[0], mask[0])
    with pytest.raises(ValueError):
        _drag(u, v, w, p, mask[:, :, :4])
    with pytest.raises(NotImplementedError):  # mixed dtypes, as _field_dtype
        _drag(u, v.astype(np.float32), w, p, mask)
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p.astype(np.float32), mask)
    with pytest.raises(NotImplementedError):
        _drag(*(a.astype(np.float16) for a in (u, v, w, p)), mask)
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask.astype(np.float64))


def test_drag_validation_scalars(no_device):
    u, v, w, p, mask = _inputs()
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            _drag(u, v, w, p, mask, h=bad)
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask, h=(np.arange(5.0), 1.0, 1.0))
    with pytest.raises(ValueError):
        _drag(u, v, w, p, mask, visc=float("nan"))
    with pytest.raises(ValueError):
        _drag(u, v, w, p, mask, visc=float("inf"))
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask, visc=np.ones(3))


def test_drag_validation_labels_and_method(no_device):
    u, v, w, p, mask = _inputs()
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask, labels=[1, 2**31])
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask.astype(np.int64) * 2**31)
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask.astype(np.int64) * 2**40, labels=[1])
    with pytest.raises(NotImplementedError):
        _drag(u, v, w, p, mask, method="mesh")
    with pytest.raises(ValueError):
        _drag(u, v, w, p, mask, method="voxel")
    # nothing to do is no device call either: no positive label in the mask
    assert _drag(u, v, w, p, np.zeros_like(mask)) == {}


def test_permeability_validation(no_device):
    u, v, w, p, _ = _inputs()
    with pytest.raises(ValueError):
        va.compute_permeability_from_pressure(u, v, w, p[:2], VISC, *H)
    with pytest.raises(NotImplementedError):
        va.compute_permeability_from_pressure(u, v, w, p.astype(np.float32), VISC, *H)
    with pytest.raises(NotImplementedError):
        va.compute_permeability_from_pressure(u, v.astype(np.float32), w, p, VISC, *H)
    with pytest.raises(ValueError):
        va.compute_permeability_from_pressure(u, v, w, p, VISC, 0.0, 1.0, 1.0)
    for shape in ((1, 4, 5), (3, 1, 5), (3, 4, 1)):
        a = np.ones(shape)
        with pytest.raises(ValueError) as e:
            va.compute_permeability_from_pressure(a, a, a, a, VISC, *H)
        assert str(e.value) == va._TOO_SMALL
        with pytest.raises(ValueError) as e_np:
            np.gradient(a, 1.0, 1.0, 1.0)
        assert str(e.value) == str(e_np.value)


def test_label_table_is_sorted_unique_with_slots():
    table, slot = _lib.drag_label_table([7, 2, 7, 5])
    assert table.dtype == np.int32 and table.tolist() == [2, 5, 7] and slot.tolist() == [2, 0, 2, 1]
    table, slot = _lib.drag_label_table(np.array([True]))
    assert table.tolist() == [1] and slot.tolist() == [0]
    for bad in ([0, 1], [-3], [1.5], []):
        with pytest.raises((NotImplementedError, ValueError)):
            _lib.drag_label_table(bad)


# ---- the host assembly ----
@pytest.mark.parametrize("name", ["f64_579", "f64_579_dup", "f64_579_nop", "f64_70"])
def test_assembly_reproduces_the_references_keys(name):
    """Records computed by the restatement (exact sums) go through the host assembly; every key lands
    within the float64 bound of the fixture, ``Area`` exactly, a repeated label summed twice."""
    g = np.load(os.path.join(GOLDEN, f"drag_{name}.npz"), allow_pickle=False)
    c = dref.make_case(name)
    labels = c["labels"]
    args = (c["u"], c["v"], c["w"], c["pressure"], c["viscosity"], *c["spacing"], c["mask"], labels)
    rec = dref.records(*args)
    terms = dref.face_terms(*args)
    res = va._assemble_drag(labels, rec, *c["spacing"], volume=2.5, has_pressure=c["pressure"] is not None)
    keys = [k.item() for k in g["keys"]]
    assert list(res) == keys
    for i, k in enumerate(keys):
        r = res[k]
        assert list(r)[:13] == list(dref.KEYS)
        for j, q in enumerate(dref.KEYS):
            ref = g["values"][i, j]
            if q == "Area":
                assert r[q] == ref, (k, q)
            else:
                assert abs(r[q] - ref) <= 2 * dref.bound64(terms[k][q]), (k, q, r[q], ref)
        for ax in "xyz":
            assert r[f"F{ax}"] == r[f"F{ax}_v"] + r[f"F{ax}_p"]
            assert r[f"M{ax}"] == r[f"F{ax}"] / 2.5
        if c["pressure"] is None:
            assert r["Fx_p"] == 0.0 and r["Fy_p"] == 0.0 and r["Fz_p"] == 0.0
    if name.endswith("dup"):  # labels = [3, 1, 3, 2]: label 3 is the single-label result twice
        once = va._assemble_drag([3], rec[:1], *c["spacing"])[3]
        assert abs(res[3]["Fx_v"] - 2 * once["Fx_v"]) <= 4 * dref.bound64(terms[3]["Fx_v"])


def test_assembly_without_faces_and_without_volume():
    rec = np.zeros((2, 3, 2), dtype=_lib.DRAG_RECORD)
    res = va._assemble_drag([4, 9], rec, *H)
    assert list(res) == [4, 9]
    for r in res.values():
        assert all(r[q] == 0.0 for q in dref.KEYS)
        assert r["Fx"] == 0.0 and r["Fy"] == 0.0 and r["Fz"] == 0.0
        assert "Mx" not in r
    assert "Mx" not in va._assemble_drag([4], rec[:1], *H, volume=0)[4]
    assert va._assemble_drag([np.True_], rec[:1], *H).keys() == {np.True_}


def test_permeability_expression_is_the_references():
    c = dref.make_perm_case(np.float64, shape=(4, 5, 6))
    sums, _, k = dref.permeability_from_pressure(c["u"], c["v"], c["w"], c["pressure"], VISC, *H)
    got = va._permeability_from_pressure(*sums, c["u"].size, VISC)
    assert got == k and isinstance(got, np.float64)
    z = va._permeability_from_pressure(1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 8, VISC)
    assert z == 0.0 and type(z) is float


# ---- the shim ----
LAYOUT = {
    "velocity_analysis": """
        def compute_strain_rate(u, v, w, dx, dy, dz, mask=None): return "host"
        def compute_pressure_field(u, v, w, dx, dy, dz, mu, rho=0, mask=None): return "host"
        def compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, method='staircase', mesh_step=1, volume=None, background_mask=None):
            if method == 'mesh':
                return compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels,
                                                   mesh_step=mesh_step, volume=volume, background_mask=background_mask)
            return "host"
        def compute_interface_drag_mesh(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels=None, mesh_step=1, volume=None, background_mask=None):
            if mesh_step == "fallback":  # the reference's ImportError branch
                return compute_interface_drag(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels, method='staircase')
            return ("host mesh", mesh_step, volume)
        def compute_permeability_from_pressure(u, v, w, pressure, viscosity, dx, dy, dz): return "host"
        def report(*a): return compute_interface_drag(*a), compute_permeability_from_pressure(*a[:8])
    """,
}


def _run(code, tmp_path, env_extra):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in LAYOUT.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    env = dict(os.environ)
    env.pop("PTV_GPU_DRAG", None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {[ROOT, str(ref)]!r}; "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)


def test_shim_default_leaves_the_hosts_functions(tmp_path):
    r = _run("""
        import sys
        import velocity_analysis as m
        ref = sys.modules["_ptv_reference_velocity_analysis"]
        for mod in (m, ref):
            for n in ("compute_interface_drag", "compute_interface_drag_mesh", "compute_permeability_from_pressure",
                      "compute_pressure_field"):
                assert getattr(mod, n).__module__ == "_ptv_reference_velocity_analysis", n
        assert m.report(*[None] * 9) == ("host", "host")
        print("ok")
    """, tmp_path, {})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_opt_in_replaces_the_two(tmp_path):
    r = _run("""
        import inspect, sys
        import velocity_analysis as m
        from ptv_interpolation_amd import velocity_analysis as gpu
        ref = sys.modules["_ptv_reference_velocity_analysis"]
        for mod in (m, ref):
            assert mod.compute_permeability_from_pressure is gpu.compute_permeability_from_pressure
            assert mod.compute_interface_drag.__module__ == "velocity_analysis"
            assert inspect.signature(mod.compute_interface_drag) == inspect.signature(gpu.compute_interface_drag)
            assert mod.compute_pressure_field(*[None] * 7) == "host"
            assert mod.compute_interface_drag_mesh.__module__ == "_ptv_reference_velocity_analysis"
        # the reference's own callers reach the GPU function, whose validation rejects the placeholders
        try:
            m.report(*[None] * 9)
        except ValueError as e:
            assert "3-D shape" in str(e), e
        else:
            raise AssertionError("the reference module's caller did not reach the GPU entry point")
        # method='mesh' reaches the layout's own function, with the keywords
        assert m.compute_interface_drag(*[None] * 9, method='mesh', mesh_step=2, volume=3.0) == ("host mesh", 2, 3.0)
        # and its staircase fallback lands on the GPU function
        try:
            m.compute_interface_drag(*[None] * 9, method='mesh', mesh_step="fallback")
        except ValueError as e:
            assert "3-D shape" in str(e), e
        else:
            raise AssertionError("the mesh function's staircase fallback stayed on the host")
        print("ok")
    """, tmp_path, {"PTV_GPU_DRAG": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_exports_the_two_names_without_the_reference():
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("PTV_GPU_DRAG", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(f"""
        import sys
        sys.path[:] = [p for p in sys.path if p]
        sys.path.insert(0, {ROOT!r})
        import velocity_analysis as m
        for n in ("compute_interface_drag", "compute_permeability_from_pressure"):
            assert getattr(m, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        assert "_ptv_reference_velocity_analysis" not in sys.modules
        print("ok")
    """)], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
