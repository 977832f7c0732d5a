"""Geometry cases shared by tests/test_geometry_cases.py (CPU preconditions) and
tests/test_gpu_geometry.py (GPU parity): one small cloud and grid, moved off the unit grid
(scaled by powers of two, offset by 1e6 and 2^40, anisotropic), flattened (planar, collinear,
nearly planar, fully coincident), put on descending and uneven axes, and placed away from the
particles.  Every case returns ``(P, Q, ax, ay, az)``; the same arrays go to the GPU and the oracle.

The base case is 3000 particles uniform in [-0.5, 12.5]^3 and a 13 x 10 x 9 grid (1170 voxels; the
x length is no multiple of the 4-voxel tile).  That grid is far below the 50 000 voxels from which
the library builds its coarse lattice, so ``<case>@dense`` is the same cloud on a 45 x 41 x 40 grid
(73 800 voxels) over the same extent: the count bounds, ``lattice_ub`` and, on the slab
DENSE_SLAB (51 660 voxels), the slab cull map run there.  The oracle results are computed once per
(case, k) and shared read-only.
"""
import functools

import numpy as np

N = 3000
SCALE_EXPONENTS = (-80, -30, 30, 80)
OFFSETS = {"offset_1e6": 1e6 + 0.3, "offset_2^40": 2.0 ** 40}
ANISO = np.array([1.0, 1e-3, 1e3])
GRID_FAR_SHIFT = np.array([40.0, -25.0, 100.0])
COINCIDENT = (3.0, 4.0, 5.0)

CASES = ([f"scale_2^{e}" for e in SCALE_EXPONENTS] + list(OFFSETS) +
         ["planar", "collinear", "near_planar", "coincident_all", "aniso", "axes_irregular", "grid_far",
          "grid_inside_gap", "n_eq_k", "n_1"])
# the cases that also run k = 1, 7, 12, 50, 130 and Sibson k = 30
WIDE_CASES = ["scale_2^-80", "scale_2^80", "offset_2^40", "planar", "near_planar", "axes_irregular", "grid_far"]
K_ALL = (8, 20)
K_WIDE = (1, 7, 12, 50, 130)
K_SIBSON = 30
RADIUS = 1.5  # base units
RADIUS_CASES = ["scale_2^-30", "scale_2^30", "offset_1e6", "planar", "grid_far"]
FILTER_CASES = ["scale_2^-80", "scale_2^80", "offset_2^40", "planar", "collinear", "aniso"]
FILTER_K = (10, 25)
RBF_CASES = ["scale_2^-30", "scale_2^30", "offset_1e6", "grid_far"]
LINEAR_CASES = ["scale_2^-30", "scale_2^30", "offset_1e6", "axes_irregular", "grid_far"]
MODE_CASES = ["offset_1e6", "axes_irregular", "planar"]
# the lattice-sized grid: shape (x, y, z), the cases run on it, and a z-slab that still builds the lattice
DENSE = (45, 41, 40)
DENSE_CASES = ["scale_2^-80", "scale_2^80", "offset_1e6", "offset_2^40", "axes_irregular", "planar"]
DENSE_SLAB = (8, 36)
DENSE_CULL_CASES = ["scale_2^-80", "scale_2^80", "offset_1e6", "offset_2^40", "axes_irregular"]
# ... of which the map must drop particles.  Not offset_2^40 (cg.mg = 1e-12 * 2^40 is 1.1 units there and
# enters the map's need several times) nor axes_irregular (its widest lattice cells span half the
# cloud): their maps may keep every particle, which costs time and no bit.
DENSE_MUST_CULL = ["scale_2^-80", "scale_2^80", "offset_1e6"]
# value-heterogeneous tie share allowed per case (0 everywhere else): near_planar's z extent is
# 1e-10 of the others', so two particles' distances to a voxel can round to the same double
TIE_CAP = {"near_planar": 0.01}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def base(dense=False):
    """(P0, Q, ax, ay, az, irregular_ax): the base case and the uneven x axis of axes_irregular
    (drawn from the same stream, after the particles; the dense grid's after the small grid's)."""
    rng = np.random.default_rng(1)
    P0 = rng.uniform(-0.5, 12.5, (N, 3))
    Q = rng.standard_normal((N, 3))
    nx, ny, nz = DENSE if dense else (13, 10, 9)
    ax = np.linspace(0.0, 12.0, nx)
    ay = np.linspace(0.25, 11.5, ny)
    az = np.linspace(1.0, 11.0, nz)
    irr = np.sort(rng.uniform(0.0, 12.0, 13))[::-1].copy()
    if dense:
        irr = np.sort(rng.uniform(0.0, 12.0, nx))[::-1].copy()
    return _ro(P0, Q, ax, ay, az, irr)


def scale_of(name):
    """The length unit of a case relative to the base case (1 unless scale_2^e)."""
    name = name.split("@")[0]
    return 2.0 ** int(name.split("^")[1]) if name.startswith("scale_2^") else 1.0


@functools.lru_cache(maxsize=None)
def case(name, k=None):
    """(P, Q, ax, ay, az) of a named case, read-only.  ``k`` matters to n_eq_k only;
    ``<name>@dense`` is the case on the lattice-sized grid."""
    name, _, grid = name.partition("@")
    P0, Q, ax, ay, az, irr = base(grid == "dense")
    P = P0.copy()
    if name == "base":
        pass
    elif name.startswith("scale_2^"):
        s = scale_of(name)  # exact: every comparison of the base case is preserved
        P, ax, ay, az = P * s, ax * s, ay * s, az * s
    elif name in OFFSETS:
        t = OFFSETS[name] * np.array([1.0, -1.0, 1.0])
        P, ax, ay, az = P + t, ax + t[0], ay + t[1], az + t[2]
    elif name == "planar":
        P[:, 2] = 6.0
    elif name == "collinear":
        P[:, 1] = 3.0
        P[:, 2] = 6.0
    elif name == "near_planar":
        P[:, 2] = 6.0 + 1e-10 * (P0[:, 2] - 6.0)
    elif name == "coincident_all":
        P[:] = COINCIDENT
        Q = np.tile(Q[0], (N, 1))
    elif name == "aniso":
        P, ax, ay, az = P * ANISO, ax * ANISO[0], ay * ANISO[1], az * ANISO[2]
    elif name == "axes_irregular":
        ax, ay, az = irr, np.geomspace(0.01, 12.0, len(ay)), az[::-1].copy()
    elif name == "grid_far":
        ax, ay, az = ax + GRID_FAR_SHIFT[0], ay + GRID_FAR_SHIFT[1], az + GRID_FAR_SHIFT[2]
    elif name == "grid_inside_gap":
        sel = (P0[:, 0] < 2.0) | (P0[:, 0] > 10.0)
        P, Q = P[sel], Q[sel]
        ax = np.linspace(3.0, 9.0, len(ax))
    elif name == "n_eq_k":
        assert k is not None
        P, Q = P[:k], Q[:k]
    elif name == "n_1":
        P, Q = P[:1], Q[:1]
    else:
        raise KeyError(name)
    return _ro(*(np.ascontiguousarray(a, dtype=np.float64) for a in (P, Q, ax, ay, az)))


def method_of(k):
    """k = 1 is method='nearest' (the reference's IDW branch needs k >= 2: its row sums take
    axis 1 of the (V, k) distances, which cKDTree returns one-dimensional for k = 1); k = 30 is
    the Sibson run; everything else IDW with p = 2."""
    return "nearest" if k == 1 else ("sibson" if k == K_SIBSON else "idw")


def get(name, k):
    """The case as run with k neighbours: (arrays, k actually used)."""
    return case(name, k if name == "n_eq_k" else None), k


def runs():
    """Every (case, k) pair of the k-NN interpolation tests: k = 8 and 20 everywhere (n_1: k = 1),
    the wider list and Sibson's 30 on WIDE_CASES, k = 8 and 20 on the lattice-sized grid."""
    out = [(n, k) for n in CASES if n != "n_1" for k in K_ALL] + [("n_1", 1)]
    out += [(n, k) for n in WIDE_CASES for k in K_WIDE + (K_SIBSON,)]
    out += [(n + "@dense", k) for n in DENSE_CASES for k in K_ALL]
    return out


@functools.lru_cache(maxsize=None)
def hetero(name, k):
    """(nz, ny, nx) bool: voxels where two correct searches may give different bits
    (tests/_util.hetero_ties).  A case whose particles all carry one (u, v, w) has none by
    definition: whatever particles a tie picks, the terms are identical."""
    from tests._util import hetero_ties

    (P, Q, ax, ay, az), kk = get(name, k)
    if (Q == Q[0]).all():
        h = np.zeros((len(az), len(ay), len(ax)), bool)
    else:
        _, h = hetero_ties(P, Q, ax, ay, az, kk)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def oracle_knn(name, k):
    """cpu_ref.interp_grid of the case with method_of(k): (U, V, W), read-only."""
    from oracle import cpu_ref

    (P, Q, ax, ay, az), kk = get(name, k)
    return _ro(*cpu_ref.interp_grid(P, Q, ax, ay, az, method_of(kk), kk, 2.0))


def queries(name, k=None):
    from oracle import cpu_ref

    _, _, ax, ay, az = case(name, k)
    return cpu_ref.grid_queries(ax, ay, az)
