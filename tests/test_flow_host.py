"""Host-side checks of the GPU flow analysis (no device needed): the structs behind
``ptv_abi_sizes6``, the signatures, the argument validation (before any device call) and the
repo-root ``velocity_analysis`` shim.

The shim tests write a stand-in for the reference's layout into a temporary directory and run a
probe in a subprocess, in the manner of test_dropin.py; with the real reference module available
(``PTV_REFERENCE_DIR``) its re-export is checked too.
"""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, velocity_analysis as va

import _flow_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ("compute_strain_rate", "compute_viscous_dissipation", "compute_vorticity", "compute_permeability",
        "compute_astarita_flow_type")


def test_abi_sizes6_match_ctypes():
    c, py = _lib.abi_sizes6()
    assert c == py, (c, py)


def test_the_capability_probe_is_the_symbol_not_the_version():
    assert _lib.lib().ptv_version() == 11
    for name in ("ptv_abi_sizes6", "ptv_flow_analysis", "ptv_flow_analysis_dev", "ptv_flow_derived",
                 "ptv_flow_derived_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name


def test_signatures_are_the_references():
    want = {  # velocity_analysis.py:10, :65, :94, :122, :151
        "compute_strain_rate": "(u, v, w, dx, dy, dz, mask=None)",
        "compute_viscous_dissipation": "(strain_rate, viscosity, dx=1.0, dy=1.0, dz=1.0, mask=None)",
        "compute_vorticity": "(u, v, w, dx, dy, dz, mask=None)",
        "compute_permeability": "(u, v, w, dissipation, viscosity, dx, dy, dz, mask=None)",
        "compute_astarita_flow_type": "(strain_rate, vorticity_mag, mask=None)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(va, name))) == sig, name
        assert name in va.__all__
    assert str(inspect.signature(va.analyze)) == "(u, v, w, dx, dy, dz, viscosity, mask=None)"


def _fields(shape=(3, 4, 5), dtype=np.float64):
    rng = np.random.default_rng(0)
    return [rng.standard_normal(shape).astype(dtype) for _ in range(3)]


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


STENCIL = [lambda u, v, w, m, h=(1.0, 1.0, 1.0): va.compute_strain_rate(u, v, w, *h, mask=m),
           lambda u, v, w, m, h=(1.0, 1.0, 1.0): va.compute_vorticity(u, v, w, *h, mask=m),
           lambda u, v, w, m, h=(1.0, 1.0, 1.0): va.analyze(u, v, w, *h, 1e-3, mask=m)]


@pytest.mark.parametrize("call", STENCIL)
def test_validation_shapes(no_device, call):
    u, v, w = _fields()
    with pytest.raises(ValueError):
        call(u, v[:, :, :4], w, None)
    with pytest.raises(ValueError):
        call(u[0], v[0], w[0], None)
    with pytest.raises(ValueError):
        call(u, v, w, np.ones((3, 4, 4), bool))


@pytest.mark.parametrize("call", STENCIL)
def test_validation_dtypes(no_device, call):
    u, v, w = _fields()
    with pytest.raises(NotImplementedError):
        call(u, v.astype(np.float32), w, None)
    with pytest.raises(NotImplementedError):
        call(*(a.astype(np.float16) for a in (u, v, w)), None)
    with pytest.raises(NotImplementedError):
        call(*(a.astype(np.complex128) for a in (u, v, w)), None)
    for bad in (np.uint8, np.int64, np.float64):
        with pytest.raises(NotImplementedError):
            call(u, v, w, np.ones(u.shape, bad))


@pytest.mark.parametrize("call", STENCIL)
@pytest.mark.parametrize("shape", [(1, 4, 5), (3, 1, 5), (3, 4, 1)])
def test_short_axis_raises_numpys_message(no_device, call, shape):
    u, v, w = _fields(shape)
    with pytest.raises(ValueError) as e:
        call(u, v, w, None)
    with pytest.raises(ValueError) as e_np:
        np.gradient(u, 1.0, 1.0, 1.0)
    assert str(e.value) == str(e_np.value)


@pytest.mark.parametrize("call", STENCIL)
def test_validation_spacings(no_device, call):
    u, v, w = _fields()
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            call(u, v, w, None, bad)
    with pytest.raises(NotImplementedError):  # coordinate arrays
        call(u, v, w, None, (np.arange(5.0), 1.0, 1.0))
    f32 = [a.astype(np.float32) for a in (u, v, w)]
    with pytest.raises(NotImplementedError):  # one axis divides in float32, another in float64
        call(*f32, None, (1.0, np.float64(1.0), 1.0))


def test_validation_derived(no_device):
    s = np.ones((3, 4, 5))
    with pytest.raises(ValueError):
        va.compute_astarita_flow_type(s, s[:2])
    with pytest.raises(NotImplementedError):
        va.compute_astarita_flow_type(s, s.astype(np.float32))
    with pytest.raises(NotImplementedError):
        va.compute_viscous_dissipation(s.astype(np.int64), 1e-3)
    with pytest.raises(NotImplementedError):
        va.compute_viscous_dissipation(s, 1e-3, mask=np.ones(s.shape, np.uint8))
    with pytest.raises(ValueError):
        va.compute_viscous_dissipation(s, 1e-3, mask=np.ones((3, 4, 4), bool))
    with pytest.raises(NotImplementedError):  # the reference's result would be float64
        va.compute_viscous_dissipation(s.astype(np.float32), np.float64(1e-3))
    with pytest.raises(ValueError):
        va.compute_permeability(s, s, s, s[:2], 1e-3, 1.0, 1.0, 1.0)


def test_permeability_expression_is_the_references():
    # from exact sums the helper gives what the reference's lines give from the means
    n = 8
    k = va._permeability(4.0, -2.0, 1.0, 0.5, n, 1e-3)
    assert k == fref.permeability_from_means(np.float64(0.5), np.float64(-0.25), np.float64(0.125),
                                             np.float64(0.0625), 1e-3)
    assert isinstance(k, np.float64)
    z = va._permeability(4.0, -2.0, 1.0, 0.0, n, 1e-3)
    assert z == 0.0 and type(z) is float


# ---- the shim ----
LAYOUT = {
    "analyze_flow": """
        from velocity_analysis import compute_strain_rate
    """,
    "velocity_analysis": """
        def compute_strain_rate(u, v, w, dx, dy, dz, mask=None): return "host"
        def compute_viscous_dissipation(strain_rate, viscosity, dx=1.0, dy=1.0, dz=1.0, mask=None): return "host"
        def compute_vorticity(u, v, w, dx, dy, dz, mask=None): return "host"
        def compute_permeability(u, v, w, dissipation, viscosity, dx, dy, dz, mask=None): return "host"
        def compute_astarita_flow_type(strain_rate, vorticity_mag, mask=None): return "host"
        def compute_pressure_field(u, v, w, dx, dy, dz, mu, rho=0, mask=None): return "host"
        def report(u, v, w): return compute_strain_rate(u, v, w, 1.0, 1.0, 1.0)
    """,
}


def _run(code, tmp_path, first, ref_dir=None):
    """Run a probe with the repository root and the layout on sys.path, `first` of them in front."""
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    if ref_dir is None:
        for name, src in LAYOUT.items():
            (ref / (name + ".py")).write_text(textwrap.dedent(src))
        ref_dir = str(ref)
    order = [ROOT, ref_dir] if first == "root" else [ref_dir, ROOT]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {order!r}; "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)


def test_shim_exports_the_five_names_without_the_reference():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(f"""
        import sys
        sys.path[:] = [p for p in sys.path if p]  # no current directory: nothing but the root holds the name
        sys.path.insert(0, {ROOT!r})
        import velocity_analysis as m
        assert m.__file__ == {os.path.join(ROOT, "velocity_analysis.py")!r}, m.__file__
        for n in {FIVE + ("analyze",)!r}:
            assert getattr(m, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        assert "_ptv_reference_velocity_analysis" not in sys.modules
        print("ok")
    """)], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_in_front_replaces_the_five_and_keeps_the_rest(tmp_path):
    r = _run(f"""
        import sys
        import velocity_analysis as m
        ref = sys.modules["_ptv_reference_velocity_analysis"]
        for mod in (m, ref):
            for n in {FIVE!r}:
                assert getattr(mod, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        assert m.compute_pressure_field(*[None] * 7) == "host"   # re-exported, still the host's
        # the reference's own callers reach the GPU function, whose validation rejects the placeholders
        try:
            m.report(None, None, None)
        except ValueError as e:
            assert "3-D shape" in str(e)
        else:
            raise AssertionError("the reference module's caller did not reach the GPU entry point")
        print("ok")
    """, tmp_path, "root")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_script_directory_in_front_keeps_its_own_module(tmp_path):
    r = _run("""
        import analyze_flow, velocity_analysis
        assert analyze_flow.compute_strain_rate.__module__ == "velocity_analysis"
        assert velocity_analysis.compute_strain_rate(*[None] * 6) == "host"
        print("ok")
    """, tmp_path, "layout")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_reexports_the_real_reference_module(tmp_path):
    ref_dir = os.environ.get("PTV_REFERENCE_DIR", "")
    if not ref_dir or not os.path.isfile(os.path.join(ref_dir, "velocity_analysis.py")):
        pytest.skip("the reference module is not available (PTV_REFERENCE_DIR)")
    r = _run(f"""
        import velocity_analysis as m
        for n in ("compute_pressure_field", "compute_interface_drag", "compute_interface_drag_mesh",
                  "compute_permeability_from_pressure"):
            assert getattr(m, n).__module__ == "_ptv_reference_velocity_analysis", n
        for n in {FIVE!r}:
            assert getattr(m, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        print("ok")
    """, tmp_path, "root", ref_dir=ref_dir)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
