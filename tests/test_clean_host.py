"""Host-side checks of the GPU divergence cleaning (no device needed): the ABI v11 structs, the
Python entry points' signatures and argument validation, and the ``PTV_GPU_CLEAN`` opt-in of the
repo-root ``physics`` shim.

The shim test writes a stand-in for the reference's layout into a temporary directory and runs a
probe there in a subprocess (the technique of test_dropin.py, restated here).
"""
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, physics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_version_is_11_and_matches_the_header():
    src = open(os.path.join(ROOT, "include", "ptv_api.h")).read()
    assert int(re.search(r"#define PTV_API_VERSION (\d+)", src).group(1)) == 11
    assert _lib.lib().ptv_version() == 11


def test_abi_sizes4_match_ctypes():
    c, py = _lib.abi_sizes4()
    assert c == py, (c, py)
    src = open(os.path.join(ROOT, "include", "ptv_api.h")).read()
    assert int(re.search(r"#define PTV_CLEAN_MAX_OUTER (\d+)", src).group(1)) == _lib.CLEAN_MAX_OUTER


def test_signatures_are_the_references():
    # physics.py:149, :110, :347
    assert str(inspect.signature(physics.clean_divergence_projection)) == \
        "(u, v, w, mask, dx, dy, dz, iterations=3)"
    assert str(inspect.signature(physics.apply_consistent_correction)) == "(u, v, w, phi, mask, dx, dy, dz)"
    assert str(inspect.signature(physics.clean_divergence)) == \
        "(u, v, w, mask, dx, dy, dz, iterations=3, method='projection', lambda_reg=1000.0)"


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
        physics.clean_divergence_projection(u, v[:, :, :4], w, m, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.clean_divergence(u, v, w, m[:2], 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.apply_consistent_correction(u, v, w, np.zeros(7), m, 1.0, 1.0, 1.0)  # phi: one per fluid voxel


def test_validation_float32_field(no_device):
    (u, v, w), m = _fields(dtype=np.float32)
    with pytest.raises(NotImplementedError):
        physics.clean_divergence_projection(u, v, w, m, 1.0, 1.0, 1.0)
    with pytest.raises(NotImplementedError):
        physics.apply_consistent_correction(u, v, w, np.zeros(m.sum()), m, 1.0, 1.0, 1.0)


def test_validation_mask_none_and_iterations(no_device):
    (u, v, w), m = _fields()
    with pytest.raises(ValueError):
        physics.clean_divergence_projection(u, v, w, None, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        physics.clean_divergence_projection(u, v, w, m, 1.0, 1.0, 1.0, iterations=-1)


def test_variational_is_not_on_the_gpu_path(no_device):
    (u, v, w), m = _fields()
    with pytest.raises(NotImplementedError):
        physics.clean_divergence(u, v, w, m, 1.0, 1.0, 1.0, method='variational')


# ---- the shim's opt-in ----
LAYOUT = {
    # the entry script marks the directory as the reference's layout (sitecustomize.py)
    "main": """
        from physics import clean_divergence
    """,
    "physics": """
        def compute_consistent_divergence(u, v, w, mask, dx, dy, dz): return "host"
        def build_laplacian_matrix(mask, dx, dy, dz): return "host"
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
    env["PYTHONPATH"] = ROOT
    env.update(extra_env or {})
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    # the probe runs as a script in the layout's directory, its own directory first on sys.path
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path.insert(0, {str(ref)!r}); "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(ref), env=env, capture_output=True, text=True, timeout=240)


def test_shim_leaves_the_projection_alone_by_default(tmp_path):
    r = _run("""
        import physics, sys
        ref = sys.modules["_ptv_reference_physics"]
        assert physics.clean_divergence_projection(*[None] * 7) == "host"
        assert physics.apply_consistent_correction(*[None] * 8) == "host"
        assert ref.clean_divergence_projection.__module__ == "_ptv_reference_physics"
        assert physics.clean_divergence(*[None] * 7) == "host"
        assert physics.compute_consistent_divergence.__module__ == "ptv_interpolation_amd.physics"
        print("ok")
    """, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_opt_in_replaces_the_projection(tmp_path):
    r = _run("""
        import physics, sys
        ref = sys.modules["_ptv_reference_physics"]
        for mod in (physics, ref):
            assert mod.clean_divergence_projection.__module__ == "ptv_interpolation_amd.physics"
            assert mod.apply_consistent_correction.__module__ == "ptv_interpolation_amd.physics"
        # the reference's dispatcher survives and now reaches the GPU function (whose validation
        # rejects the placeholder arguments before any device call)
        assert physics.clean_divergence.__module__ == "_ptv_reference_physics"
        try:
            physics.clean_divergence(*[None] * 7)
        except ValueError as e:
            assert "mask" in str(e)
        else:
            raise AssertionError("the dispatcher did not reach the GPU entry point")
        assert physics.clean_divergence(*[None] * 7, method='variational') == "host"
        print("ok")
    """, tmp_path, {"PTV_GPU_CLEAN": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
