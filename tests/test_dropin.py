"""The zero-edit drop-in (sitecustomize.py + the repo-root shims): a ``main.py`` in the
reference's layout imports the MI355X modules when this repo is on ``PYTHONPATH``, and the
``physics`` shim keeps every reference name (``clean_divergence``, ``solve_poisson``, ...).

CPU only and self-contained: the test writes a stand-in for the reference's layout into a
temporary directory, an entry script ``main.py`` with the reference's import lines
(main.py:9-12) next to ``interpolator.py``, ``filtering.py``, ``physics.py``, ``visualizer.py``
and ``velocity_analysis.py`` that define the names those lines ask for.  ``tifffile`` (not a
dependency of this project) is stubbed for the import.
"""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the stand-in layout: module name -> source.  Only the names matter (what main.py imports, what
# the physics shim must keep), every body is a host-side placeholder.
LAYOUT = {
    "main": """
        import tifffile
        from interpolator import load_ptv_data, load_mask, create_grid, interpolate_field, extract_boundary_particles
        from physics import clean_divergence
        from visualizer import show
        from filtering import apply_filters
    """,
    "interpolator": """
        import tifffile
        def load_ptv_data(filepath): return "host"
        def load_mask(filepath): return "host"
        def create_grid(bounds, resolution): return "host"
        def interpolate_field(df, grid_tuple, method="linear", **kw): return "host"
        def sample_mask_on_grid(mask_raw, grid_tuple, bounds_raw): return "host"
        def extract_boundary_particles(mask, bounds, sampling_step=1, thickness=1): return "host"
    """,
    "filtering": """
        def remove_outliers_knn(df, k=25, threshold=3.0): return "host"
        def remove_outliers_threshold(df, max_speed=10.0): return "host"
        def apply_filters(df, args): return "host"
    """,
    "physics": """
        def compute_consistent_divergence(u, v, w, mask, dx, dy, dz): return "host"
        def build_laplacian_matrix(mask, dx, dy, dz): return "host"
        def solve_poisson(source, mask, dx, dy, dz, **kw): return "host"
        def clean_divergence(u, v, w, mask, dx, dy, dz, iterations=3, **kw):
            return compute_consistent_divergence(u, v, w, mask, dx, dy, dz)
        def clean_divergence_variational(u, v, w, mask, dx, dy, dz, iterations=1, lambda_reg=1e3): return "host"
    """,
    "visualizer": """
        def show(*a, **k): return None
    """,
    "velocity_analysis": """
        def pressure(source, mask):
            from physics import solve_poisson
            return solve_poisson(source, mask, 1.0, 1.0, 1.0)
    """,
}


def _run(code, tmp_path, extra_env=None):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in LAYOUT.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    stub = tmp_path / "stub"
    stub.mkdir(exist_ok=True)
    (stub / "tifffile.py").write_text("def imread(*a, **k):\n    raise OSError('stub')\n"
                                      "def imwrite(*a, **k):\n    raise OSError('stub')\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, str(stub)])
    env["MPLBACKEND"] = "Agg"
    env.update(extra_env or {})
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    # run the probe as a script in the layout's directory: its own directory comes first
    # on sys.path, exactly like `python main.py` there
    r = subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path.insert(0, {str(ref)!r}); "
                        f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                       cwd=str(ref), env=env, capture_output=True, text=True, timeout=240)
    return r


def test_main_imports_the_mi355x_modules(tmp_path):
    r = _run("""
        import main
        import interpolator, filtering, physics
        assert main.interpolate_field.__module__ == "ptv_interpolation_amd.interpolator", main.interpolate_field.__module__
        assert main.apply_filters.__module__ == "ptv_interpolation_amd.filtering"
        assert main.load_ptv_data.__module__ == "ptv_interpolation_amd.interpolator"
        # physics: the reference names survive, the divergence is the GPU one everywhere
        assert callable(main.clean_divergence) and callable(physics.solve_poisson)
        assert physics.compute_consistent_divergence.__module__ == "ptv_interpolation_amd.physics"
        ref = __import__("sys").modules["_ptv_reference_physics"]
        assert ref.compute_consistent_divergence is physics.compute_consistent_divergence
        import velocity_analysis  # velocity_analysis.py:298 imports solve_poisson lazily
        assert velocity_analysis.pressure(None, None) == "host"  # the solver stays the layout's own
        from physics import solve_poisson, build_laplacian_matrix, clean_divergence_variational
        print("ok")
    """, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_dropin_can_be_disabled(tmp_path):
    r = _run("""
        import main
        assert main.interpolate_field.__module__ == "interpolator", main.interpolate_field.__module__
        print("ok")
    """, tmp_path, {"PTV_DROPIN": "0"})
    assert r.returncode == 0, r.stdout + r.stderr
