"""Host-side checks of the GPU mask alignment (no device needed): the structs behind
``ptv_abi_sizes8``, the signatures, every validation (before any device call, and the size limit
before any copy), the host's assembly of the objective from the device's records, and the repo-root
``auto_align`` shim (probes in subprocesses over a stand-in layout, as test_drag_host.py does it).
"""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, alignment as al

import _align_ref as aref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_sizes8_match_ctypes():
    c, py = _lib.abi_sizes8()
    assert c == py, (c, py)
    assert _lib.ALIGN_RECORD.itemsize == py[3]
    assert _lib.ALIGN_RECORD == aref.RECORD


def test_the_capability_probe_is_the_symbol_not_the_version():
    assert _lib.lib().ptv_version() == 11
    for name in ("ptv_abi_sizes8", "ptv_edt", "ptv_edt_dev", "ptv_align_score", "ptv_align_score_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    for name in ("edt", "edt_dev", "align_score", "align_score_dev"):
        assert callable(getattr(_lib.Context, name)), name
    assert callable(_lib.AlignSession.score)


def test_signatures():
    assert str(inspect.signature(al.distance_transform_edt)) == (
        "(input, sampling=None, return_distances=True, return_indices=False, *, return_squared=False)")
    assert str(inspect.signature(al.alignment_objective)) == "(points, dt_or_mask, offsets)"
    # auto_align.py:10
    assert str(inspect.signature(al.find_best_offset)) == "(df, mask, initial_offset=(0, 0, 0), invert=False)"


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_edt_validation(no_device):
    m = np.ones((3, 4, 5), dtype=bool)
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(m, sampling=(1.0, 2.0, 1.0))
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(m, sampling=1.0)
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(m, return_indices=True)
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(m[0])
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(np.ones((2, 2, 2, 2), dtype=np.uint8))
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(m.astype(np.float64))
    with pytest.raises(ValueError):
        al.distance_transform_edt(m, return_distances=False)


def test_the_size_limit_comes_before_any_copy(no_device):
    big = np.broadcast_to(np.True_, (40000, 40000, 1))  # a view that owns no memory
    with pytest.raises(NotImplementedError):
        al.distance_transform_edt(big)
    with pytest.raises(NotImplementedError):
        al.alignment_objective(np.zeros((1, 3)), big, [(0, 0, 0)])
    with pytest.raises(NotImplementedError):
        al.find_best_offset(aref.Frame(np.zeros((1, 3))), big)
    # the last shape below the limit passes the check (46340^2 < 2^31 <= 46341^2)
    assert _lib.edt_check_shape((46340, 1, 1)) == (46340, 1, 1)
    with pytest.raises(NotImplementedError):
        _lib.edt_check_shape((46341, 1, 1))
    with pytest.raises(NotImplementedError):
        _lib.edt_check_shape((26755, 26755, 26755))


def test_empty_in_empty_out(no_device):
    for shape in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
        d = al.distance_transform_edt(np.ones(shape, dtype=bool))
        assert d.shape == shape and d.dtype == np.float64
        d2 = al.distance_transform_edt(np.ones(shape, dtype=np.int32), return_squared=True)
        assert d2.shape == shape and d2.dtype == np.int32


def test_objective_validation(no_device):
    dt = np.ones((3, 4, 5))
    ok = np.zeros((2, 3))
    for bad in (np.zeros((2, 2)), np.zeros(3), np.array([[0.0, np.nan, 0.0]]), np.array([[np.inf, 0.0, 0.0]])):
        with pytest.raises(ValueError):
            al.alignment_objective(bad, dt, [(0, 0, 0)])
    for bad in (np.zeros((2, 2)), np.zeros((2, 3, 1)), [(0.0, np.nan, 0.0)], [(0.0, -np.inf, 0.0)]):
        with pytest.raises(ValueError):
            al.alignment_objective(ok, dt, bad)
    with pytest.raises(ValueError):
        al.alignment_objective(ok, dt[0], [(0, 0, 0)])
    with pytest.raises(ValueError):
        al.alignment_objective(ok, np.ones((0, 4, 5)), [(0, 0, 0)])


def test_find_best_offset_validation(no_device):
    mask = np.ones((3, 4, 5), dtype=bool)
    with pytest.raises(ValueError):
        al.find_best_offset(aref.Frame(np.array([[0.0, np.nan, 1.0]])), mask)
    with pytest.raises(NotImplementedError):
        al.find_best_offset(aref.Frame(np.zeros((1, 3))), mask.astype(np.uint8))
    with pytest.raises(NotImplementedError):
        al.find_best_offset(aref.Frame(np.zeros((1, 3))), mask[0])


def test_objective_values_are_the_references_expression():
    rec = np.zeros(3, dtype=_lib.ALIGN_RECORD)
    rec[0] = (0, 7, 0.0)
    rec[1] = (5, 2, 1.25)
    rec[2] = (7, 0, 0.0)
    v = al.objective_values(rec, np.sqrt(np.float64(3)))
    assert v.dtype == np.float64
    assert v[0] == 1e9
    assert v[1] == np.float64(1.25) + np.int64(2) * np.sqrt(np.float64(3))
    assert v[2] == 0.0


# ---- the shim ----
LAYOUT = {
    "auto_align": """
        import helper
        def find_best_offset(df, mask, initial_offset=(0, 0, 0), invert=False): return "host"
        def main(): return find_best_offset(None, None)
    """,
    "helper": "",
}
LAYOUT_NO_TIFF = {
    "auto_align": """
        import module_that_is_not_installed_anywhere
        def find_best_offset(df, mask, initial_offset=(0, 0, 0), invert=False): return "host"
        def main(): return find_best_offset(None, None)
    """,
}


def _run(code, tmp_path, layout):
    ref = tmp_path / "layout"
    ref.mkdir(exist_ok=True)
    for name, src in layout.items():
        (ref / (name + ".py")).write_text(textwrap.dedent(src))
    env = dict(os.environ, PYTHONPATH=ROOT)
    script = tmp_path / "probe.py"
    script.write_text(textwrap.dedent(code))
    return subprocess.run([sys.executable, "-c", f"import runpy, sys; sys.path[:0] = {[ROOT, str(ref)]!r}; "
                           f"runpy.run_path({str(script)!r}, run_name='__main__')"],
                          cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)


def test_shim_replaces_the_function_inside_the_reference_module(tmp_path):
    r = _run("""
        import sys
        import auto_align as m
        from ptv_interpolation_amd import alignment as gpu
        ref = sys.modules["_ptv_reference_auto_align"]
        assert m.find_best_offset is gpu.find_best_offset and ref.find_best_offset is gpu.find_best_offset
        assert m.main is ref.main and m.helper is ref.helper
        # the reference's main() reaches the GPU function, whose validation rejects the placeholders
        try:
            m.main()
        except (TypeError, AttributeError, NotImplementedError, ValueError):
            pass
        else:
            raise AssertionError("the reference module's main() did not reach the GPU entry point")
        print("ok")
    """, tmp_path, LAYOUT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_survives_a_reference_module_that_cannot_import(tmp_path):
    r = _run("""
        import sys
        import auto_align as m
        from ptv_interpolation_amd import alignment as gpu
        assert m.find_best_offset is gpu.find_best_offset
        assert "_ptv_reference_auto_align" not in sys.modules and not hasattr(m, "main")
        print("ok")
    """, tmp_path, LAYOUT_NO_TIFF)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")


def test_shim_exports_the_function_without_the_reference():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(f"""
        import sys
        sys.path[:] = [p for p in sys.path if p]
        sys.path.insert(0, {ROOT!r})
        import auto_align as m
        assert m.find_best_offset.__module__ == "ptv_interpolation_amd.alignment"
        assert "_ptv_reference_auto_align" not in sys.modules
        print("ok")
    """)], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
