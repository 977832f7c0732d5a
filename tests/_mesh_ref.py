"""Numpy restatement of the mesh interface drag (reference velocity_analysis.py:547-655) and of the
spline sampling under it, written from the formulae; imports scipy only.

Two chains over the same code path (``terms``):
  - float64 with ``scipy.ndimage.map_coordinates`` as the sampler: the reference's arithmetic,
    operation for operation (tests/test_mesh_ref.py holds it to the reference's fixtures);
  - ``np.longdouble`` (x87 extended, 64-bit significand) with the prefilter and the samplers below:
    used as "exact".  What is data in the reference's definition stays as it is: the centroid and
    the edge differences are formed in the vertices' dtype, and the fields are the given values.

The bar of the GPU tests: a value g passes when |g - exact| <= 8 * max(gap, eps * scale) with
gap = |reference - exact|, scale = the sum of |term| and eps = 2^-52 (``bar``).
"""
import numpy as np
from scipy import ndimage

KEYS = ("Fx_v", "Fy_v", "Fz_v", "Fx_v_tan", "Fy_v_tan", "Fz_v_tan", "Fx_v_nor", "Fy_v_nor", "Fz_v_nor",
        "Fx_p", "Fy_p", "Fz_p", "Area", "Fx_water", "Fy_water", "Fz_water", "Fx_solid", "Fy_solid", "Fz_solid",
        "Area_water", "Area_solid")
PAD = 12
EPS = 2.0 ** -52
LD = np.longdouble


def bar(gap, scale):
    return 8.0 * np.maximum(np.asarray(gap, dtype=np.float64), EPS * np.asarray(scale, dtype=np.float64))


# ---- meshes ----
def sphere_mesh(center, radius, levels=2):
    """An octahedron subdivided ``levels`` times, projected on the sphere; float32 vertices (as
    skimage's), int32 faces with outward winding."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, dtype=np.float64) for p in v]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    verts = np.asarray(center, dtype=np.float64) + np.asarray(radius, dtype=np.float64) * np.array(v)
    return verts.astype(np.float32), np.array(f, dtype=np.int32)


def sheet_mesh(origin, a, b, na, nb):
    """A flat sheet: the lattice origin + i * a + j * b, two triangles per cell; float32 vertices."""
    origin, a, b = (np.asarray(x, dtype=np.float64) for x in (origin, a, b))
    i, j = np.meshgrid(np.arange(na + 1), np.arange(nb + 1), indexing="ij")
    verts = origin + i.reshape(-1, 1) * a + j.reshape(-1, 1) * b
    idx = lambda p, q: p * (nb + 1) + q  # noqa: E731
    f = []
    for p in range(na):
        for q in range(nb):
            f += [(idx(p, q), idx(p + 1, q), idx(p, q + 1)), (idx(p + 1, q), idx(p + 1, q + 1), idx(p, q + 1))]
    return verts.astype(np.float32), np.array(f, dtype=np.int32)


# ---- the long-double spline chain ----
def _filter_axis(c, axis):
    c = np.moveaxis(c, axis, 0).copy()
    n = c.shape[0]
    z = np.sqrt(LD(3)) - LD(2)
    c *= (1 - z) * (1 - 1 / z)
    zn = z ** n
    c0 = c[0].copy()
    s = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n):  # scipy's reflect start
        s = s + zi * (c[i] + zn * c[n - 1 - i])
        zi = zi * z
    c[0] = s * (z / (1 - zn * zn)) + c0
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] *= z / (z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def prefilter(field, ft=LD):
    """The cubic B-spline coefficients of the field padded by 12 edge-replicated samples."""
    c = np.pad(np.asarray(field).astype(ft), PAD, mode="edge")
    for axis in range(3):
        c = _filter_axis(c, axis)
    return c


def sample3(coef, coords):
    """Order 3 on the padded coefficients at coords (3, n) of the raw field's index space.

    scipy's rule past the pad (probed in tests/test_spline_edge_cases.py): the padded coordinate is
    clamped to [-1, N], one sample past either end of the padded extent N, not to [0, N - 1]; the
    fraction is kept there and only the four indices are edge-extended, so the value still moves
    between -1 and 0 and between N - 1 and N and saturates at -1 and at N."""
    ft = coef.dtype.type
    total = np.zeros(coords.shape[1], dtype=ft)
    wts, idx = [], []
    for a in range(3):
        c = np.clip(coords[a].astype(ft) + PAD, -1, coef.shape[a])
        f = np.floor(c)
        t = c - f
        wts.append([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6,
                    t ** 3 / 6])
        i0 = f.astype(np.int64) - 1
        idx.append([np.clip(i0 + k, 0, coef.shape[a] - 1) for k in range(4)])
    for kz in range(4):
        for ky in range(4):
            for kx in range(4):
                total = total + wts[0][kz] * wts[1][ky] * wts[2][kx] * coef[idx[0][kz], idx[1][ky], idx[2][kx]]
    return total


def sample1(field, coords, ft=LD):
    field = np.asarray(field)
    total = np.zeros(coords.shape[1], dtype=ft)
    wts, idx = [], []
    for a in range(3):
        c = np.clip(coords[a].astype(ft), 0, field.shape[a] - 1)
        f = np.floor(c)
        t = c - f
        wts.append([1 - t, t])
        i0 = f.astype(np.int64)
        idx.append([i0, np.minimum(i0 + 1, field.shape[a] - 1)])
    for kz in range(2):
        for ky in range(2):
            for kx in range(2):
                total = total + wts[0][kz] * wts[1][ky] * wts[2][kx] * field[idx[0][kz], idx[1][ky], idx[2][kx]].astype(ft)
    return total


def index0(shape, coords):
    """Order 0: the index of the sample at floor(c + 0.5), clamped; a NaN coordinate reads index 0
    (what scipy's cast of NaN gives on x86-64)."""
    out = []
    for a in range(3):
        c = np.asarray(coords[a], dtype=np.float64)
        c = np.where(c > 0, c, 0.0)  # NaN -> 0
        c = np.minimum(c, shape[a] - 1)
        out.append(np.floor(c + 0.5).astype(np.int64))
    return tuple(out)


# ---- the traction terms ----
class ScipySampler:
    """The reference's own calls, on the fields as given."""

    def __init__(self, u, v, w, pressure, background):
        self.f, self.p, self.bg = (u, v, w), pressure, background

    def inner(self, k, coords):
        return ndimage.map_coordinates(self.f[k], coords, order=3, mode="nearest")

    def interface(self, k, coords):
        return ndimage.map_coordinates(self.f[k], coords, order=1, mode="nearest")

    def pressure(self, coords):
        return ndimage.map_coordinates(self.p, coords, order=1) if self.p is not None else np.zeros(coords.shape[1])

    def water(self, coords):
        if self.bg is None:
            return np.ones(coords.shape[1], dtype=bool)
        return ndimage.map_coordinates(self.bg.astype(float), coords, order=0, mode="nearest") > 0.5


class ExactSampler:
    """The long-double chain; the coefficients are computed once per field."""

    def __init__(self, u, v, w, pressure, background):
        self.f, self.p, self.bg = (u, v, w), pressure, background
        self.coef = [prefilter(a) for a in self.f]

    def inner(self, k, coords):
        return sample3(self.coef[k], coords)

    def interface(self, k, coords):
        return sample1(self.f[k], coords)

    def pressure(self, coords):
        return sample1(self.p, coords) if self.p is not None else np.zeros(coords.shape[1], dtype=LD)

    def water(self, coords):
        if self.bg is None:
            return np.ones(coords.shape[1], dtype=bool)
        return self.bg.astype(float)[index0(self.bg.shape, coords)] > 0.5


def terms(verts, faces, sampler, viscosity, dx, dy, dz, ft=np.float64):
    """The 21 per-triangle terms (21, n_tri) behind the reference's sums, in ``ft``."""
    with np.errstate(invalid="ignore", divide="ignore"):
        tri = verts[faces]
        cen = tri.mean(axis=1)  # the vertices' dtype
        h = np.array([dz, dy, dx], dtype=ft)
        e1 = (tri[:, 1] - tri[:, 0]).astype(ft) * h
        e2 = (tri[:, 2] - tri[:, 0]).astype(ft) * h
        half = ft(0.5)
        ns = np.stack([half * (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]),
                       half * (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]),
                       half * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])], axis=1)
        area = np.sqrt((ns[:, 0] ** 2 + ns[:, 1] ** 2) + ns[:, 2] ** 2)
        nph = ns / np.maximum(area[:, None], ft(1e-20))
        nvx = nph / h
        nvx = nvx / np.sqrt((nvx[:, 0] ** 2 + nvx[:, 1] ** 2) + nvx[:, 2] ** 2)[:, None]
        quarter = ft(0.25)
        dphys = quarter * np.sqrt(((nvx[:, 0] * h[0]) ** 2 + (nvx[:, 1] * h[1]) ** 2) + (nvx[:, 2] * h[2]) ** 2)
        inner = (cen + quarter * nvx).T
        outer = (cen - quarter * nvx).T
        visc = viscosity if ft is np.float64 else ft(viscosity)
        tv = [visc * (sampler.interface(k, cen.T) - sampler.inner(k, inner)) / dphys for k in range(3)]  # x, y, z
        p = sampler.pressure(cen.T)
        nrm = [nph[:, 2], nph[:, 1], nph[:, 0]]  # x, y, z
        tp = [p * n for n in nrm]
        dot = tv[0] * nrm[0] + tv[1] * nrm[1] + tv[2] * nrm[2]
        nor = [dot * n for n in nrm]
        tan = [a - b for a, b in zip(tv, nor)]
        water = sampler.water(outer)
        zero = np.zeros_like(area)
        both = [(a + b) * area for a, b in zip(tv, tp)]
        rows = ([a * area for a in tv] + [a * area for a in tan] + [a * area for a in nor] + [a * area for a in tp] +
                [area] + [np.where(water, b, zero) for b in both] + [np.where(~water, b, zero) for b in both] +
                [np.where(water, area, zero), np.where(~water, area, zero)])
        return np.stack([np.asarray(r, dtype=ft) for r in rows]), water


def integrate(meshes, u, v, w, pressure, viscosity, dx, dy, dz, background=None, ft=np.float64):
    """``{label: (sums, scale)}`` with ``sums`` the 21 sums in ``ft`` (np.sum, as the reference) and
    ``scale`` the float64 sum of |term| per key.  float64: scipy's samplers; long double: the exact
    chain.  A label without faces is left out.  The phase-split sums are taken over the class's
    triangles only, as the reference's boolean indexing does."""
    if ft is np.float64:
        sampler = ScipySampler(u, v, w, pressure, background)
    else:
        sampler = ExactSampler(u, v, w, pressure, background)
    out = {}
    for label, (verts, faces) in meshes.items():
        if len(faces) == 0:
            continue
        t, water = terms(verts, faces, sampler, viscosity, dx, dy, dz, ft)
        sums = np.empty(len(KEYS), dtype=ft)
        for k, name in enumerate(KEYS):
            sel = water if "water" in name else (~water if "solid" in name else slice(None))
            sums[k] = np.sum(t[k][sel])
        with np.errstate(invalid="ignore"):
            scale = np.array([np.sum(np.abs(np.where(np.isnan(r), 0, r))) for r in t], dtype=np.float64)
        out[label] = (sums, scale)
    return out


# ---- inputs ----
def make_fields(shape, seed, dtype=np.float64, pressure=True):
    """A smooth flow with a tenth of noise on it, O(1) values; u, v, w and the pressure."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    out = []
    for k in range(4):
        ph = rng.uniform(0, 2 * np.pi, 3)
        kk = rng.uniform(0.2, 0.7, 3)
        f = np.sin(kk[0] * z + ph[0]) * np.cos(kk[1] * y + ph[1]) + 0.5 * np.sin(kk[2] * x + ph[2]) + 0.3 * (k + 1)
        out.append((f + 0.1 * rng.standard_normal(shape)).astype(dtype))
    return out if pressure else out[:3] + [None]
