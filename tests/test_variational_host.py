"""Host-side checks of the GPU variational cleaning (no device needed): the structs behind
``ptv_abi_sizes5``, the Python entry point's signature and argument validation, and the
``PTV_GPU_CLEAN_VARIATIONAL`` opt-in of the repo-root ``physics`` shim.

The shim tests write a stand-in for the reference's layout into a temporary directory and run a
probe there in a subprocess, in the manner of test_clean_host.py.
"""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, physics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_sizes5_match_ctypes():
    c, py = _lib.abi_sizes5()
    assert c == py, (c, py)


def test_the_capability_probe_is_the_symbol_not_the_version():
    assert _lib.lib().ptv_version() == 11
    assert hasattr(_lib.lib(), "ptv_abi_sizes5")
    for name in ("ptv_clean_variational", "ptv_clean_variational_dev", "ptv_variational_apply",
                 "ptv_divergence_operator_apply"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name


def test_signature_is_the_references():
    # physics.py:440
    assert str(inspect.signature(physics.clean_divergence_variational)) == \
        "(u, v, w, mask, dx, dy, dz, iterations=1, lambda_reg=1000.0)"
    assert "clean_divergence_variational" in physics.__all__


def _fields(shape=(3, 4, 5), dtype=np.float64):
    rng = np.random.default_rng(0)
    return [rng.standard_normal(shape).astype(dtype) for _ in range(3)], np.ones(shape, bool)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def test_validation_shape_mismatch(no_device):
    (u, v, w), m = _fields()
    with pytest.raises(ValueError):
        physics.clean_divergence_variational(u, v[:, :, :4], w, m, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.clean_divergence_variational(u, v, w, m[:2], 1.0, 1.0, 1.0)


def test_validation_dtypes(no_device):
    (u, v, w), m = _fields(dtype=np.float32)
    with pytest.raises(NotImplementedError):
        physics.clean_divergence_variational(u, v, w, m, 1.0, 1.0, 1.0)
    (u, v, w), m = _fields()
    with pytest.raises(NotImplementedError):
        physics.clean_divergence_variational(u, v, w, m.astype(np.uint8), 1.0, 1.0, 1.0)


def test_validation_mask_none(no_device):
    (u, v, w), _ = _fields()
    with pytest.raises(ValueError):
        physics.clean_divergence_variational(u, v, w, None, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("lam, exc", [(-1.0, NotImplementedError), (float("nan"), ValueError),
                                      (float("inf"), ValueError)])
def test_validation_lambda(no_device, lam, exc):
    (u, v, w), m = _fields()
    with pytest.raises(exc):
        physics.clean_divergence_variational(u, v, w, m, 1.0, 1.0, 1.0, lambda_reg=lam)


# ---- the shim's opt-in ----
LAYOUT = {
    # the entry script marks the directory as the reference's layout (sitecustomize.py)
    "main": """
        from physics import clean_divergence
    """,
    "physics": """
        def compute_consistent_divergence(u, v, w, mask, dx, dy, dz): return "host"
        def apply_consistent_correction(u, v, w, phi, mask, dx, dy, dz): return "host"
        def clean_divergence_projection(u, v, w, mask, dx, dy, dz, iterations=3): return "host"
        def clean_divergence_variational(u, v, w, mask, dx, dy, dz, iterations=1, lambda_reg=1e3): return "host"
        def clean_divergence(u, v, w, mask, dx, dy, dz, iterations=3, method='projection', lambda_reg=1e3):
            if method == 'variational':
                return clean_divergence_variational(u, v, w, mask, dx, dy, dz, lambda_reg=lambda_reg)
            return clean_divergence_projection(u, v, w, mask, dx, dy, dz, iterations=iterations)
    """,
}


def _run(code, tmp_path, extra_env=None):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in LAYOUT.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    env = dict(os.environ)
    env.pop("PTV_GPU_CLEAN", None)
    env.pop("PTV_GPU_CLEAN_VARIATIONAL", None)
    env["PYTHONPATH"] = ROOT
    env.update(extra_env or {})
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    # the probe runs as a script in the layout's directory, its own directory first on sys.path
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path.insert(0, {str(ref)!r}); "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(ref), env=env, capture_output=True, text=True, timeout=240)


HOST_PROBE = """
    import physics, sys
    ref = sys.modules["_ptv_reference_physics"]
    assert physics.clean_divergence_variational(*[None] * 7) == "host"
    assert ref.clean_divergence_variational.__module__ == "_ptv_reference_physics"
    assert physics.clean_divergence(*[None] * 7, method='variational') == "host"
    print("ok")
"""


def test_shim_leaves_the_variational_method_alone_by_default(tmp_path):
    r = _run(HOST_PROBE, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_projection_switch_alone_leaves_it_on_the_host(tmp_path):
    r = _run(HOST_PROBE, tmp_path, {"PTV_GPU_CLEAN": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_opt_in_replaces_the_variational_method(tmp_path):
    r = _run("""
        import physics, sys
        ref = sys.modules["_ptv_reference_physics"]
        for mod in (physics, ref):
            assert mod.clean_divergence_variational.__module__ == "ptv_interpolation_amd.physics"
            # independent of PTV_GPU_CLEAN: the projection stays the host's
            assert mod.clean_divergence_projection.__module__ == "_ptv_reference_physics"
        # the reference's dispatcher survives and now reaches the GPU function (whose validation
        # rejects the placeholder arguments before any device call)
        assert physics.clean_divergence.__module__ == "_ptv_reference_physics"
        try:
            physics.clean_divergence(*[None] * 7, method='variational')
        except ValueError as e:
            assert "mask" in str(e)
        else:
            raise AssertionError("the dispatcher did not reach the GPU entry point")
        assert physics.clean_divergence(*[None] * 7) == "host"
        print("ok")
    """, tmp_path, {"PTV_GPU_CLEAN_VARIATIONAL": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
