"""Host-side checks of the device component labelling (no device needed): the structs behind
``ptv_abi_sizes12``, the version and the exported names, the C validation, and every
``NotImplementedError`` / ``ValueError`` of ``labelling.label``'s contract, raised before any device
work.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ptv_interpolation_amd import _lib, labelling

import _label_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_sizes12():
    c, py = _lib.abi_sizes12()
    assert c == py, (c, py)
    assert [f[0] for f in _lib.LabelParams._fields_] == ["nz", "ny", "nx", "connectivity"]
    assert [f[0] for f in _lib.LabelStats._fields_] == ["n_components", "n_foreground", "ms_merge", "ms_number"]


def test_version_and_exports():
    src = open(os.path.join(ROOT, "include", "ptv_api.h")).read()
    assert _lib.lib().ptv_version() == 11 == int(re.search(r"#define PTV_API_VERSION (\d+)", src).group(1))
    for name in ("ptv_abi_sizes12", "ptv_label", "ptv_label_dev"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for name in ("label", "label_dev"):
        assert callable(getattr(_lib.Context, name)), name
    assert labelling.__all__ == ["label", "TILE"]
    assert str(inspect.signature(labelling.label)) == "(input, structure=None, output=None, *, return_sizes=False)"


def test_tile_constant_is_the_kernels():
    hpp = open(os.path.join(ROOT, "ptv_interpolation_amd", "csrc", "ptv_label.hpp")).read()
    tile = tuple(int(re.search(r"constexpr int kLabelTile%s = (\d+);" % a, hpp).group(1)) for a in "ZYX")
    assert tile == labelling.TILE


def test_c_validation_needs_no_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8)()
    out = (ctypes.c_int32 * 8)()
    ok = _lib.LabelParams(2, 2, 2, 6)
    fake = ctypes.c_void_p(1)  # a context that is never dereferenced: every check below comes first
    for fn, extra in ((L.ptv_label, ()), (L.ptv_label_dev, (None,))):
        assert fn(None, ctypes.byref(ok), buf, out, None, *extra, None) == _lib.PTV_E_ARG
        assert fn(fake, None, buf, out, None, *extra, None) == _lib.PTV_E_ARG
        assert fn(fake, ctypes.byref(ok), None, out, None, *extra, None) == _lib.PTV_E_ARG
        assert fn(fake, ctypes.byref(ok), buf, None, None, *extra, None) == _lib.PTV_E_ARG
        for bad in (0, 4, 8, 27, -6):
            prm = _lib.LabelParams(2, 2, 2, bad)
            assert fn(fake, ctypes.byref(prm), buf, out, None, *extra, None) == _lib.PTV_E_ARG
        for dims in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
            prm = _lib.LabelParams(*dims, 6)
            assert fn(fake, ctypes.byref(prm), buf, out, None, *extra, None) == _lib.PTV_E_ARG
        for dims in ((2**11, 2**10, 2**10), (1, 1, 2**31), (2**40, 2**40, 2**40), (2**21, 2**21, 1)):
            prm = _lib.LabelParams(*dims, 26)
            assert fn(fake, ctypes.byref(prm), buf, out, None, *extra, None) == _lib.PTV_E_UNSUPPORTED
        assert b"2^31" in L.ptv_last_error()


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("device call before validation")
    monkeypatch.setattr(_lib.Context, "get", classmethod(boom))


def test_validation_before_any_device_call(no_device):
    m = np.zeros((4, 5, 6), dtype=bool)
    m[1:3, 1:3, 1:3] = True
    for bad in (m.astype(np.float32), m.astype(np.float64), m.astype(np.complex64), m.astype(object)):
        with pytest.raises(NotImplementedError):
            labelling.label(bad)
    for bad in (m[0], m[0, 0], m[None]):  # 2-D, 1-D, 4-D
        with pytest.raises(NotImplementedError):
            labelling.label(bad)
    # 2^31 voxels: the shape alone decides, nothing is copied (the array is a view of one byte)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(2**11, 2**10, 2**10), strides=(0, 0, 0))
    with pytest.raises(NotImplementedError, match="2\\^31"):
        labelling.label(huge)
    # a structure that is not one of the three: named in the message
    cross = ref.structure(6).copy()
    cross[0, 0, 0] = True
    for bad in (cross, np.zeros((3, 3, 3), bool), np.ones((3, 3, 3)) - ref.structure(6)):
        with pytest.raises(NotImplementedError, match=r"\(3, 1\).*\(3, 2\).*\(3, 3\)"):
            labelling.label(m, bad)
    for bad in (np.ones((3, 3), bool), np.ones((3, 3, 5), bool), np.ones((1, 3, 3, 3), bool), np.ones(27, bool)):
        with pytest.raises(ValueError):
            labelling.label(m, bad)
    for bad in (np.int64, np.uint8, np.float64, "int64", np.zeros(m.shape, np.int32), np.zeros(m.shape, np.int64)):
        with pytest.raises(NotImplementedError):
            labelling.label(m, output=bad)
    # what is valid reaches the device
    for structure in (None, ref.structure(6), ref.structure(18).astype(int), ref.structure(26).tolist()):
        for output in (None, np.int32, np.dtype("int32")):
            with pytest.raises(AssertionError, match="device call"):
                labelling.label(m, structure, output)
    with pytest.raises(TypeError):  # keyword only
        labelling.label(m, None, None, True)


def test_empty_input_is_no_device_call(no_device):
    for shape in ((0, 3, 4), (3, 0, 4), (3, 4, 0)):
        labels, num = labelling.label(np.zeros(shape, bool))
        assert labels.shape == shape and labels.dtype == np.int32 and num == 0 and isinstance(num, int)
        labels, num, sizes = labelling.label(np.zeros(shape, np.int16), ref.structure(26), return_sizes=True)
        assert labels.shape == shape and num == 0
        assert sizes.dtype == np.int64 and np.array_equal(sizes, np.bincount(labels.ravel(), minlength=1))


def test_sizes_room_is_enough():
    # the 6-neighbour checkerboard has the most components a volume can have
    for shape in ((1, 1, 1), (3, 3, 3), (2, 5, 7), (4, 4, 4)):
        z, y, x = np.indices(shape)
        for parity in (0, 1):
            num = ref.label_ref((z + y + x) % 2 == parity, 6)[1]
            assert num + 1 <= _lib.label_sizes_room(int(np.prod(shape)))
