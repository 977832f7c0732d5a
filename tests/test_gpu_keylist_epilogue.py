"""The weight-and-sum epilogue of the packed-key lists (13 <= k <= 127, ``ptv_knn_epilogue.hpp``):
one implementation walked three ways (KMAX <= 32 in half blocks of 4, up to 56 in whole blocks of
8, both unrolled; 64, 96 and 128 slots in a rolled loop).  A query of k neighbours takes the list
of the next length above k.

Against ``oracle.cpu_ref`` on every voxel: the inputs have n >= k, so the reference defines all of
them (asserted).  Grid 24 x 20 x 12: no multiple of the 4^3 tile, so padded lanes and the partial
x-tile take part.  IDW p = 2 uses IEEE-exact operations only and is held bit for bit; p = 3 goes
through ``pow`` and Sibson through ``exp``, which no other implementation reproduces bit for bit:
those are held to the project's normwise bar (``TOL`` of ``test_gpu_parity``).
Runs only on an MI355X (``-m gpu``).
"""
import numpy as np
import pytest

from tests._util import normwise
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

AX, AY, AZ = np.arange(24.0), np.arange(20.0), np.arange(12.0)
HI = np.array([23.0, 19.0, 11.0])
# every list length (16 .. 128) at its fullest k (k + 1 = KMAX), and with a multiple of 8 where
# the length admits one (16, 32, 48, 56, 64, 96: no tail block); a tail in each of the three forms
K_EXACT = [13, 15, 16, 23, 31, 32, 39, 47, 48, 55, 56, 63, 64, 95, 96, 127]
K_NORMWISE = [13, 24, 31, 40, 55, 63, 127]
_REF = {}


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _particles():
    rng = np.random.default_rng(7)
    return rng.uniform(0.0, 1.0, (1500, 3)) * HI, rng.standard_normal((1500, 3))


def _ref(method, k, power=2.0, z0=0, z1=None):
    """Oracle outputs of a case, computed once and shared (read-only)."""
    from oracle import cpu_ref

    key = (method, k, power, z0, z1)
    if key not in _REF:
        P, Q = _particles()
        ref = cpu_ref.interp_grid(P, Q, AX, AY, AZ, method, k, power, z0=z0, z1=z1)
        for r in ref:
            assert np.isfinite(r).all()  # the reference defines every voxel: none is left out
            r.setflags(write=False)
        _REF[key] = (P, Q, ref)
    return _REF[key]


def _bits(out, ref, what):
    for c, (a, b) in enumerate(zip(out, ref)):
        assert a.shape == b.shape
        bad = int(np.sum(a != b))
        print(f"{what} {'UVW'[c]}: {bad} of {a.size} voxels differ")
        assert np.array_equal(a, b), f"{bad} voxels differ"


def _norm(out, ref, what):
    for c, (a, b) in enumerate(zip(out, ref)):
        assert a.shape == b.shape and np.isfinite(a).all()
        err = normwise(a, b)
        print(f"{what} {'UVW'[c]}: normwise {err:.2e}")
        assert err <= TOL


@pytest.mark.parametrize("k", K_EXACT)
def test_idw_p2_bit_exact(ctx, k):
    P, Q, ref = _ref("idw", k)
    _bits(ctx.interp_knn(P, Q, axes=(AX, AY, AZ), k=k, power=2.0), ref, f"idw p=2 k={k}")


@pytest.mark.parametrize("k", K_NORMWISE)
def test_idw_p3_normwise(ctx, k):
    P, Q, ref = _ref("idw", k, 3.0)
    _norm(ctx.interp_knn(P, Q, axes=(AX, AY, AZ), k=k, power=3.0), ref, f"idw p=3 k={k}")


@pytest.mark.parametrize("k", K_NORMWISE)
def test_sibson_normwise(ctx, k):
    from ptv_interpolation_amd import _lib

    P, Q, ref = _ref("sibson", k)
    _norm(ctx.interp_knn(P, Q, axes=(AX, AY, AZ), method=_lib.METHOD_SIBSON, k=k), ref, f"sibson k={k}")


def test_nan_to_num_flag(ctx):
    """Every output is finite, so the flag must change nothing."""
    from ptv_interpolation_amd import _lib

    P, Q, ref = _ref("idw", 39)
    _bits(ctx.interp_knn(P, Q, axes=(AX, AY, AZ), k=39, power=2.0, flags=_lib.FLAG_NAN_TO_NUM), ref,
          "idw p=2 k=39 nan_to_num")


def test_z_slab_off_tile_boundary(ctx):
    """A slab from z = 3 to 9: it starts and ends inside a tile, so the output offset differs from
    the voxel's grid index."""
    P, Q, ref = _ref("idw", 23, z0=3, z1=9)
    _bits(ctx.interp_knn(P, Q, axes=(AX, AY, AZ), k=23, power=2.0, z_range=(3, 9)), ref, "idw p=2 k=23 z 3..9")
