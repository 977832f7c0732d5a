"""Seeded edge cases for the three rows beside the k-NN hot path: the pore-mask path
(ptv_mask.hip), the consistent divergence (ptv_div.hip) and the k-NN outlier filter
(ptv_filter.hip and the filter epilogue of the search kernel).

Plain numpy, no GPU import.  tests/test_rows_edge_cases.py holds the oracle (oracle/cpu_ref.py)
to scipy and numpy on these cases; tests/test_gpu_{mask,div,filter}_edges.py hold the kernels to
the oracle on the same cases, bit for bit.
"""
import functools

import numpy as np


def blob_mask(shape, n_spheres, seed):
    """Random union of solid spheres (False) in fluid (True), as tests/golden/make_golden.py builds it."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    fluid = np.ones(shape, dtype=bool)
    for _ in range(n_spheres):
        c = rng.uniform(0, 1, 3) * np.array([nx, ny, nz])
        r = rng.uniform(2.0, 0.25 * min(shape) + 2.0)
        fluid &= (X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2 > r * r
    return fluid


# ----------------------------------------------------------------------------- mask sampling
def raw_bounds(shape, descending=(False, False, False), lo=0.0):
    """bounds_raw ((xmin, xmax), (ymin, ymax), (zmin, zmax)) whose raw axes ``linspace(min, max - 1, n)``
    are ``lo + arange(n)``, or that reversed where ``descending`` (x, y, z) says so."""
    nz, ny, nx = shape
    out = []
    for n, d in zip((nx, ny, nz), descending):
        out.append((lo + n - 1, lo + 1) if (d and n > 1) else (lo, lo + n))
    return tuple(out)


def _raw_u8(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0, 0, 1, 2, 255], dtype=np.uint8), size=shape)


def _raw_float(shape, seed):
    """float raw mask on the `> 0.5` threshold: exactly 0.5 and NaN are solid, the next float up is fluid."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.5, np.nextafter(0.5, 1.0), np.nan, 1.0, 0.25])
    return rng.choice(vals, size=shape)


HALF_SHAPE = (5, 6, 9)
DESCENDING = [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
              (True, True, True)]


def half_way_cases():
    """[(name, raw, bounds, (ax, ay, az))]: a 2x resampling of a (5, 6, 9) raw mask: every second grid
    point lies exactly half-way between two raw voxels, with each raw axis descending in turn."""
    nz, ny, nx = HALF_SHAPE
    axes = tuple(np.linspace(0, n - 1, 2 * n - 1) for n in (nx, ny, nz))
    assert all((a[1::2] % 1.0 == 0.5).all() for a in axes)
    out = []
    for kind, raw in (("u8", _raw_u8(HALF_SHAPE, 11)), ("float", _raw_float(HALF_SHAPE, 12))):
        for d in DESCENDING:
            out.append((f"half_{kind}_desc{''.join(str(int(v)) for v in d)}", raw, raw_bounds(HALF_SHAPE, d), axes))
    return out


def beyond_bounds_cases():
    """A grid one voxel wider than the raw box on every side; both raw end points exactly, and the
    floats next to them on either side."""
    out = []
    for d in (DESCENDING[0], DESCENDING[-1]):
        axes = []
        for n in HALF_SHAPE[::-1]:
            e = float(n - 1)
            axes.append(np.array([-1.0, np.nextafter(0.0, -1.0), 0.0, np.nextafter(0.0, 1.0), 0.5, 1.0, e - 1.0,
                                  np.nextafter(e, 0.0), e, np.nextafter(e, np.inf), e + 1.0]))
        out.append((f"beyond_desc{int(d[0])}", _raw_u8(HALF_SHAPE, 13), raw_bounds(HALF_SHAPE, d), tuple(axes)))
    return out


def length_one_cases():
    """One length-1 raw axis per dimension; the grid holds its one in-bounds coordinate (2.0), the
    floats on either side of it and the voxels one step away."""
    out = []
    for shape in ((1, 6, 9), (5, 1, 9), (5, 6, 1)):
        axes = []
        for n in shape[::-1]:
            if n == 1:
                axes.append(np.array([1.0, np.nextafter(2.0, 0.0), 2.0, np.nextafter(2.0, 3.0), 3.0]))
            else:
                axes.append(np.linspace(2.0, 2.0 + n - 1, 2 * n - 1))
        out.append((f"len1_{'x'.join(map(str, shape))}", _raw_u8(shape, 14 + sum(shape)), raw_bounds(shape, lo=2.0),
                    tuple(axes)))
    return out


ROW_STORE_NX = (1, 7, 8, 9, 15, 16, 23)


def row_store_cases():
    """nx on either side of the 8-voxel run with ny = 3, nz = 2: the six row starts fall on every
    alignment mod 8 the extent allows; the grid overhangs the raw box by a voxel."""
    raw = _raw_u8((4, 5, 6), 15)
    out = []
    for nx in ROW_STORE_NX:
        axes = (np.linspace(-1.0, 6.0, nx) if nx > 1 else np.array([2.5]), np.linspace(0.0, 4.0, 3),
                np.array([0.5, 3.0]))
        out.append((f"rows_nx{nx}", raw, raw_bounds(raw.shape), axes))
    return out


def mask_sample_cases():
    return half_way_cases() + beyond_bounds_cases() + length_one_cases() + row_store_cases()


def slab_case():
    """(raw, bounds, (ax, ay, az)) for the z_range launches: 7 planes, nx = 13 (a row tail)."""
    raw = _raw_u8((6, 7, 8), 16)
    axes = (np.linspace(-0.5, 8.0, 13), np.linspace(0.0, 6.0, 5), np.linspace(-1.0, 6.0, 7))
    return raw, raw_bounds(raw.shape), axes


SLABS = ((0, 1), (1, 4), (4, None))


# ----------------------------------------------------------------------------- boundary particles
SWAR_SHAPES = ((3, 5, 16), (6, 9, 48), (9, 17, 64))
GENERIC_SHAPES = ((6, 9, 47), (9, 17, 63))
THICKNESSES = (1, 2, 3, 4)
STEPS = (1, 2, 7)
MASK_KINDS = ("blob", "checker", "corners", "face", "first", "last")


@functools.lru_cache(maxsize=None)
def bool_mask(kind, shape):
    """The bool masks of the boundary cases (read-only).  The same `kind` on (.., 48) and (.., 47) is the
    same content cut one column short, so the 16-voxel kernels and the per-voxel ones see one picture."""
    nz, ny, nx = shape
    full = (nz, ny, (nx + 15) // 16 * 16)
    if kind == "blob":
        m = blob_mask(full, 6, 21)
    elif kind == "checker":
        z, y, x = np.indices(full)
        m = (z + y + x) % 2 == 0
    else:
        m = np.zeros(full, dtype=bool)
        if kind == "corners":
            m[np.ix_([0, nz - 1], [0, ny - 1], [0, nx - 1])] = True
        elif kind == "face":
            m[:, :, 0] = True
        elif kind == "first":
            m[0, 0, 0] = True
        elif kind == "last":
            m[nz - 1, ny - 1, nx - 1] = True
        else:
            raise KeyError(kind)
    m = np.ascontiguousarray(m[:, :, :nx])
    m.setflags(write=False)
    return m


def shape_bounds(shape):
    """Non-trivial float bounds ((xmin, xmax), (ymin, ymax), (zmin, zmax)) for a mask shape."""
    nz, ny, nx = shape
    return ((1.5, 2.0 * nx), (0, ny), (-4, nz - 1))


WIDE_DTYPES = (np.int8, np.uint8, np.int16, np.int32, np.int64)
WIDE_VALUES = (0, 1, 2, 3, 254, 255, -1, -2, -128, 256, 257, 65536, 2**40)


def wide_mask(shape, dtype, seed=31):
    """Integer mask drawn from WIDE_VALUES clipped to the dtype's range, half of it zero: non-zero
    values with a zero low byte, negative ones, odd ones with high bits set."""
    info = np.iinfo(dtype)
    vals = np.unique(np.clip(np.array(WIDE_VALUES, dtype=np.int64), info.min, info.max)).astype(dtype)
    rng = np.random.default_rng(seed)
    m = rng.choice(vals, size=shape)
    m[rng.uniform(size=shape) < 0.5] = 0
    return m


SCAN_SHAPES = ((65, 256, 256), (65, 257, 255))  # 1040 count blocks of 4096 voxels each: the scan's carry loop


@functools.lru_cache(maxsize=None)
def scan_mask(shape):
    m = blob_mask(shape, 40, 41)
    m.setflags(write=False)
    return m


DEGENERATE_SHAPES = ((1, 1, 16), (1, 1, 5), (1, 7, 1), (4, 1, 32))


def degenerate_mask(shape):
    rng = np.random.default_rng(51 + sum(shape))
    m = rng.uniform(size=shape) < 0.4
    m.reshape(-1)[0] = True
    m.reshape(-1)[-1] = False
    return m


# ----------------------------------------------------------------------------- divergence
def div_fields(shape, dtype, seed, fluid=0.6):
    rng = np.random.default_rng(seed)
    u, v, w = (rng.standard_normal(shape).astype(dtype) for _ in range(3))
    m = rng.uniform(size=shape) < fluid
    return u, v, w, m


def nan_in_solid(u, v, w, m):
    """An un-filled interpolation: NaN in every solid cell of all three components."""
    return tuple(np.where(m, a, a.dtype.type(np.nan)) for a in (u, v, w))


def nonfinite_in_fluid(u, v, w, m, seed, share=0.05):
    """NaN, +inf and -inf at `share` of the fluid cells of each component, chosen at random."""
    rng = np.random.default_rng(seed)
    out = []
    for a in (u, v, w):
        a = a.copy()
        idx = np.flatnonzero(m)
        pick = rng.choice(idx, max(3, int(share * len(idx))), replace=False)
        a.reshape(-1)[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf]), len(pick)).astype(a.dtype)
        out.append(a)
    return tuple(out)


def extreme_fields(shape, dtype, seed):
    """Fields drawn from the edges of the format: smallest normal, subnormals, 0.75 max (sums of two
    overflow), signed zeros, ordinary values."""
    fi = np.finfo(dtype)
    sub = fi.smallest_subnormal
    vals = np.array([fi.tiny, -fi.tiny, sub, -sub, 3 * sub, 1025 * sub, 0.75 * fi.max, -0.75 * fi.max, 0.0, -0.0,
                     1.0, -1.5], dtype=dtype)
    rng = np.random.default_rng(seed)
    u, v, w = (rng.choice(vals, size=shape) for _ in range(3))
    m = rng.uniform(size=shape) < 0.7
    return u, v, w, m


DIV_NX = (1, 2, 3, 4, 5, 8, 64, 65, 256, 260)
DIV_NZ = (1, 2, 31, 32, 33, 35, 65)
DIV_TINY = ((1, 1, 1), (1, 1, 7), (1, 5, 1), (5, 1, 1))
DIV_SLAB_CUTS = (0, 1, 34, 37, 70)


# ----------------------------------------------------------------------------- outlier filter
def filter_ref(points, values, k, threshold=3.0, mad_eps=1e-6, knn="kdtree"):
    """cpu_ref.outlier_filter with `mad_eps` free (the oracle has 1e-6 fixed) -> (keep, kth distance)."""
    from scipy.spatial import KDTree

    from oracle import cpu_ref

    P = np.asarray(points, dtype=np.float64)
    u, v, w = (np.asarray(values, dtype=np.float64)[:, c] for c in range(3))
    speed = np.sqrt(u**2 + v**2 + w**2)
    if knn == "kdtree":
        dist, idx = KDTree(P).query(P, k=k + 1)
    else:
        dist, idx = cpu_ref.knn_bruteforce(P, P, k + 1)
    ns = speed[idx[:, 1:]]
    med = np.median(ns, axis=1)
    mad = np.median(np.abs(ns - med[:, None]), axis=1)
    z = np.abs(speed - med) / (mad + mad_eps)
    return z <= threshold, dist[:, -1]


def cloud(n, seed, outliers=0):
    """Continuous random cloud in a 10-box with normal velocities, `outliers` of them 8x faster."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 10.0, (n, 3))
    Q = rng.standard_normal((n, 3))
    if outliers:
        Q[rng.choice(n, outliers, replace=False)] *= 8.0
    return P, Q


SWEEP_KS = tuple(range(1, 127))


@functools.lru_cache(maxsize=None)
def sweep_cloud():
    return cloud(700, 61, outliers=20)


TINY_KS = (1, 2, 5, 25, 62)
BIG_KS = (127, 128)


def tiny_cases():
    """[(k, n)]: clouds just above k, below, at and above one wave tile (64) and one block (256)."""
    out = []
    for k in TINY_KS:
        for n in sorted({k + 1, k + 2, 63, 64, 65, 255, 256, 257}):
            if n > k:
                out.append((k, n))
    for k in BIG_KS:
        out += [(k, k + 1), (k, k + 2), (k, 300)]
    return out


def tiny_cloud(k, n):
    return cloud(n, 1000 * k + n, outliers=min(3, n // 8))


NONFINITE_KS = (6, 25, 50, 130)


@functools.lru_cache(maxsize=None)
def nonfinite_cloud():
    """1000 particles: 1 % with one NaN component, 1 % with one infinite component, 4 all-infinite."""
    P, Q = cloud(1000, 71, outliers=10)
    rng = np.random.default_rng(72)
    pick = rng.choice(1000, 24, replace=False)
    for i in pick[:10]:
        Q[i, rng.integers(3)] = np.nan
    for i in pick[10:20]:
        Q[i, rng.integers(3)] = rng.choice([np.inf, -np.inf])
    for i in pick[20:]:
        Q[i] = rng.choice([np.inf, -np.inf], 3)
    return P, Q


QUANT_KS = (4, 9, 25, 40)
QUANT_KINDS = ("levels", "one_outlier", "zeros")


@functools.lru_cache(maxsize=None)
def quantised_cloud(kind):
    """500 particles whose speeds repeat exactly: many medians on a tie, MAD often exactly 0."""
    P, _ = cloud(500, 81)
    Q = np.zeros((500, 3))
    if kind == "levels":
        Q[:, 1] = np.random.default_rng(82).integers(0, 4, 500)
    elif kind == "one_outlier":
        Q[:, 0] = 0.6
        Q[:, 2] = -0.8
        Q[137] = (30.0, 0.0, -40.0)
    elif kind != "zeros":
        raise KeyError(kind)
    return P, Q


PARAM_KS = (8, 25)
THRESHOLDS = (0.0, 0.5, 1e9)
MAD_EPS = (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def param_clouds():
    return {"continuous": cloud(600, 91, outliers=15), "levels": quantised_cloud("levels")}


DUP_KS = (8, 25)
DUP_CAP = 0.10  # largest share of tie-dependent particles the coincident case may exclude


@functools.lru_cache(maxsize=None)
def coincident_cloud():
    """1000 particles, 30 of them coincident copies of another one (with their own velocities)."""
    P, Q = cloud(1000, 95, outliers=20)
    rng = np.random.default_rng(96)
    src = rng.choice(970, 30, replace=False)
    P[970:] = P[src]
    return P, Q


def all_filter_clouds():
    """[(name, P, ks, may_tie)] of every cloud the GPU filter tests use, with every k it is used at."""
    out = [("sweep", sweep_cloud()[0], SWEEP_KS, False)]
    for k, n in tiny_cases():
        out.append((f"tiny_k{k}_n{n}", tiny_cloud(k, n)[0], (k,), False))
    out.append(("nonfinite", nonfinite_cloud()[0], NONFINITE_KS, False))
    out.append(("quantised", quantised_cloud("levels")[0], QUANT_KS, False))
    out.append(("params", param_clouds()["continuous"][0], PARAM_KS, False))
    out.append(("params_levels", param_clouds()["levels"][0], PARAM_KS, False))
    out.append(("coincident", coincident_cloud()[0], DUP_KS, True))
    return out
