"""Host-side checks of the pressure recovery (no GPU): argument validation before any device call,
and the ``PTV_GPU_PRESSURE`` opt-in of the repo-root shims (probes in subprocesses over a stand-in
layout, as test_drag_host.py does it)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, physics, velocity_analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (4, 5, 6)


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("validation must fail before a device call")

    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def fields(shape=SHAPE, dtype=np.float64):
    return [np.zeros(shape, dtype) for _ in range(3)]


def mask(shape=SHAPE):
    return np.ones(shape, bool)


@pytest.mark.parametrize("fn", [velocity_analysis.compute_pressure_field, velocity_analysis.recover_pressure,
                                velocity_analysis.compute_force_field])
def test_field_validation(fn):
    u, v, w = fields()
    with pytest.raises(ValueError):
        fn(u, v, np.zeros((4, 5, 7)), 1.0, 1.0, 1.0, 1e-3, mask=mask())
    with pytest.raises(ValueError):
        fn(u[0], v[0], w[0], 1.0, 1.0, 1.0, 1e-3)
    with pytest.raises(ValueError):
        fn(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=np.ones((4, 5, 7), bool))
    with pytest.raises(NotImplementedError):
        fn(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=np.ones(SHAPE, np.uint8))
    with pytest.raises(NotImplementedError):
        fn(u.astype(complex), v, w, 1.0, 1.0, 1.0, 1e-3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fn(u, v, w, 1.0, bad, 1.0, 1e-3, mask=mask())
    with pytest.raises(ValueError):
        fn(u, v, w, 1.0, 1.0, 1.0, float("inf"), mask=mask())
    with pytest.raises(ValueError):
        fn(u, v, w, 1.0, 1.0, 1.0, 1e-3, rho=float("nan"), mask=mask())
    with pytest.raises(ValueError, match="too small"):  # np.gradient's error for rho > 0
        fn(*fields((1, 5, 6)), 1.0, 1.0, 1.0, 1e-3, rho=1.0, mask=mask((1, 5, 6)))


@pytest.mark.parametrize("fn", [velocity_analysis.compute_pressure_field, velocity_analysis.recover_pressure])
def test_unknown_wall_bc_and_anchor(fn):
    u, v, w = fields()
    with pytest.raises(ValueError, match="wall_bc"):
        fn(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=mask(), wall_bc="periodic")
    with pytest.raises(ValueError, match="anchor"):
        fn(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=mask(), anchor="middle")


def test_recover_pressure_solver_settings():
    u, v, w = fields()
    with pytest.raises(ValueError):
        velocity_analysis.recover_pressure(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=mask(), maxiter=-1)
    with pytest.raises(ValueError):
        velocity_analysis.recover_pressure(u, v, w, 1.0, 1.0, 1.0, 1e-3, mask=mask(), rtol=float("nan"))


def test_force_divergence_validation():
    f = fields()
    with pytest.raises(ValueError):
        physics.compute_force_divergence(*f, None, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.compute_force_divergence(*f, mask((4, 5, 7)), 1.0, 1.0, 1.0)
    with pytest.raises(NotImplementedError):
        physics.compute_force_divergence(*fields(dtype=np.float32), mask(), 1.0, 1.0, 1.0)
    with pytest.raises(NotImplementedError):
        physics.compute_force_divergence(*f, np.ones(SHAPE, np.uint8), 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.compute_force_divergence(*f, mask(), 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="wall_bc"):
        physics.compute_force_divergence(*f, mask(), 1.0, 1.0, 1.0, wall_bc="free-slip")


def test_solve_poisson_validation():
    rhs = np.zeros(SHAPE)
    d = np.zeros(SHAPE, bool)
    d[-1] = True
    with pytest.raises(ValueError, match="double count"):
        physics.solve_poisson(rhs, mask(), 1.0, 1.0, 1.0, dirichlet_mask=d, dirichlet_values=1.0)
    with pytest.raises(ValueError, match="double count"):
        physics.solve_poisson(rhs, mask(), 1.0, 1.0, 1.0, dirichlet_mask=d, dirichlet_values=np.ones(SHAPE))
    with pytest.raises(ValueError):
        physics.solve_poisson(None, mask(), 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.solve_poisson(rhs, mask(), 1.0, 1.0, 1.0, dirichlet_mask=np.zeros((4, 5, 7), bool))
    with pytest.raises(ValueError):
        physics.solve_poisson(rhs, mask(), 1.0, -1.0, 1.0)
    with pytest.raises(ValueError, match="wall_bc"):
        physics.solve_poisson(None, mask(), 1.0, 1.0, 1.0, force_field=fields(), wall_bc="nope")
    # a mask with no fluid returns zeros without a device call (physics.py:275-276)
    out = physics.solve_poisson(rhs + 1.0, np.zeros(SHAPE, bool), 1.0, 1.0, 1.0, dirichlet_mask=d, dirichlet_values=0.0)
    assert out.shape == SHAPE and out.dtype == np.float64 and not out.any()


LAYOUT = {
    "velocity_analysis": """
        def compute_strain_rate(*a, **k): return "host"
        def compute_viscous_dissipation(*a, **k): return "host"
        def compute_vorticity(*a, **k): return "host"
        def compute_permeability(*a, **k): return "host"
        def compute_astarita_flow_type(*a, **k): return "host"
        def compute_pressure_field(*a, **k): return "host"
        def compute_interface_drag(*a, **k): return "host"
        def compute_permeability_from_pressure(*a, **k): return "host"
        def caller(*a, **k): return compute_pressure_field(*a, **k)
    """,
    "physics": """
        def compute_consistent_divergence(*a, **k): return "host"
        def compute_force_divergence(*a, **k): return "host"
        def solve_poisson(*a, **k): return "host"
    """,
}


def _run(code, tmp_path, env_extra):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in LAYOUT.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    env = dict(os.environ)
    for k in ("PTV_GPU_DRAG", "PTV_GPU_PRESSURE", "PTV_GPU_CLEAN", "PTV_GPU_CLEAN_VARIATIONAL"):
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {[ROOT, str(ref)]!r}; "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)


@pytest.mark.parametrize("env", [{}, {"PTV_GPU_DRAG": "1"}])
def test_shim_default_leaves_the_hosts_function(tmp_path, env):
    r = _run("""
        import sys
        import velocity_analysis as m, physics as ph
        ref = sys.modules["_ptv_reference_velocity_analysis"]
        assert m.compute_pressure_field() == "host" and ref.compute_pressure_field() == "host" and m.caller() == "host"
        assert not hasattr(m, "recover_pressure")
        assert ph.solve_poisson() == "host" and ph.compute_force_divergence() == "host"
        print("ok")
    """, tmp_path, env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_opt_in_replaces_the_function(tmp_path):
    r = _run("""
        import sys
        import velocity_analysis as m, physics as ph
        from ptv_interpolation_amd import velocity_analysis as gpu
        ref = sys.modules["_ptv_reference_velocity_analysis"]
        assert m.compute_pressure_field is gpu.compute_pressure_field
        assert ref.compute_pressure_field is gpu.compute_pressure_field  # the reference's own callers reach it
        assert m.compute_interface_drag() == "host"  # PTV_GPU_DRAG is a separate switch
        assert ph.solve_poisson() == "host" and ph.compute_force_divergence() == "host"
        print("ok")
    """, tmp_path, {"PTV_GPU_PRESSURE": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shims_export_the_names_without_the_reference():
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("PTV_GPU_PRESSURE", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(f"""
        import sys
        sys.path[:] = [p for p in sys.path if p]
        sys.path.insert(0, {ROOT!r})
        import velocity_analysis as m, physics as ph
        for n in ("compute_pressure_field", "recover_pressure", "compute_force_field"):
            assert getattr(m, n).__module__ == "ptv_interpolation_amd.velocity_analysis", n
        for n in ("compute_force_divergence", "solve_poisson"):
            assert getattr(ph, n).__module__ == "ptv_interpolation_amd.physics", n
        assert "_ptv_reference_velocity_analysis" not in sys.modules
        print("ok")
    """)], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
