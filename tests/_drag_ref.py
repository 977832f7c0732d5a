"""A numpy restatement of the reference's staircase interface drag (velocity_analysis.py:332-511)
that keeps every face's term instead of its sum, and the bounds the drag tests hold sums to.

``face_terms`` returns, per given label and key, the list of the float64 terms that enter the key,
with the sign they enter it with (the reference subtracts the viscous sums, adds the pressure sums).
A test then has the exact value ``E = math.fsum(terms)`` and ``S = math.fsum(|terms|)``: any order of
summing n float64 numbers lies within ``gamma(n) * S`` of E.  test_drag_oracle.py holds this module
to the reference's fixtures.

``records`` reduces the same faces to the device's layout, one record per (label, axis, direction),
for the host assembly to be tested without a device.
"""
import math

import numpy as np

KEYS = ("Fx_v", "Fy_v", "Fz_v", "Fx_v_tan", "Fy_v_tan", "Fz_v_tan", "Fx_v_nor", "Fy_v_nor", "Fz_v_nor",
        "Fx_p", "Fy_p", "Fz_p", "Area")
FORCE_KEYS = KEYS[:-1]
RECORD = np.dtype([("count", np.int64), ("sum_p", np.float64), ("sum_u", np.float64), ("sum_v", np.float64),
                   ("sum_w", np.float64)])
U64 = 2.0**-53
U32 = 2.0**-24


def gamma(n, u=U64):
    """(n - 1) u / (1 - (n - 1) u): the relative bound, in units of sum|x|, of any summation order."""
    n = max(int(n), 1)
    return (n - 1) * u / (1.0 - (n - 1) * u)


def _faces(mask, axis, label, direction):
    """Index arrays (curr cells, next cells) of the faces of `label` along `axis` in one direction,
    in C order of the curr cell."""
    s_curr = [slice(None)] * 3
    s_next = [slice(None)] * 3
    s_curr[axis] = slice(0, -1)
    s_next[axis] = slice(1, None)
    mc, mn = mask[tuple(s_curr)], mask[tuple(s_next)]
    idx = (mc == 0) & (mn == label) if direction == 0 else (mc == label) & (mn == 0)
    curr = np.argwhere(idx)
    nxt = curr.copy()
    nxt[:, axis] += 1
    return tuple(curr.T), tuple(nxt.T)


def _terms_of(fields, pressure, viscosity, spacing, mask, axis, label, direction):
    """(count, pressure terms, u terms, v terms, w terms) of one (label, axis, direction), float64
    arrays in face order, as the device evaluates them (float32 inputs widened first)."""
    dx, dy, dz = spacing
    area = [dy * dx, dz * dx, dz * dy][axis]
    step = [dz, dy, dx][axis]
    curr, nxt = _faces(mask, axis, label, direction)
    fluid = curr if direction == 0 else nxt
    n = len(curr[0])
    if pressure is None:
        tp = np.zeros(n)
    else:
        p_face = 0.5 * (pressure[curr].astype(np.float64) + pressure[nxt].astype(np.float64))
        tp = p_face * area if direction == 0 else (-p_face) * area
    out = [n, tp]
    for comp, f in zip((2, 1, 0), fields):  # u is normal to x faces (axis 2), v to y, w to z
        d = (-2.0 * f[fluid].astype(np.float64)) / step
        out.append(((viscosity * 2) * d) * area if comp == axis else (viscosity * d) * area)
    return out


def records(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels):
    """One RECORD per (given label, axis, direction), summed with math.fsum."""
    mask = np.asarray(mask)
    rec = np.zeros((len(labels), 3, 2), dtype=RECORD)
    for i, label in enumerate(labels):
        for axis in range(3):
            for direction in range(2):
                n, tp, tu, tv, tw = _terms_of((u, v, w), pressure, viscosity, (dx, dy, dz), mask, axis, label, direction)
                rec[i, axis, direction] = (n, math.fsum(tp), math.fsum(tu), math.fsum(tv), math.fsum(tw))
    return rec


def face_terms(u, v, w, pressure, viscosity, dx, dy, dz, mask, labels):
    """{label: {key: [terms]}} for the 12 force keys, and ``Area`` as the reference accumulates it (a
    value, not a list: counts are integers, so it is exact).  A label given twice has its terms
    twice, as the reference sums it twice."""
    mask = np.asarray(mask)
    out = {}
    for label in labels:
        out[label] = {k: [] for k in FORCE_KEYS}
        out[label]["Area"] = 0.0
    dA = [dy * dx, dz * dx, dz * dy]
    for axis in range(3):
        normal = "zyx"[axis]
        for label in labels:
            r = out[label]
            for direction in range(2):
                n, tp, tu, tv, tw = _terms_of((u, v, w), pressure, viscosity, (dx, dy, dz), mask, axis, label, direction)
                if n == 0:
                    continue
                r["Area"] += np.int64(n) * dA[axis]
                if pressure is not None:
                    r[f"F{normal}_p"].extend(tp.tolist())
                for comp, t in (("x", tu), ("y", tv), ("z", tw)):
                    neg = (-t).tolist()
                    r[f"F{comp}_v"].extend(neg)
                    r[f"F{comp}_v_" + ("nor" if comp == normal else "tan")].extend(neg)
    return out


def exact(terms):
    """(E, S, n) of a list of terms."""
    return math.fsum(terms), math.fsum(abs(t) for t in terms), len(terms)


def bound64(terms, extra=12):
    """|any float64 summation of the terms, combined on the host from at most `extra` partial sums, - E|"""
    _, s, n = exact(terms)
    return gamma(n + extra) * s


def bound32(terms):
    """|the reference's float32 result - E64|: each term rounded at most 4 times in float32, then a
    float32 sum of n terms: (n + 4) 2^-24 S, the second-order terms inside a factor (1 + 2^-10)."""
    _, s, n = exact(terms)
    return (n + 4) * U32 * s * (1.0 + 2.0**-10)


# ---- seeded cases shared by the fixture script and the tests ----
SPACING = (0.3, 1.1, 0.7)  # dx, dy, dz as Python floats: anisotropic
VISCOSITY = 1.5e-3

# name: (shape, field dtype, labels in the mask, coarse cell of the blobs, what is special)
CASES = {
    "f64_222": ((2, 2, 2), np.float64, 2, (1, 1, 1), None),
    "f64_159": ((1, 5, 9), np.float64, 3, (1, 1, 2), None),
    "f32_519": ((5, 1, 9), np.float32, 3, (1, 1, 2), None),
    "f64_579": ((5, 7, 9), np.float64, 4, (1, 2, 2), None),
    "f32_579": ((5, 7, 9), np.float32, 4, (1, 2, 2), None),
    "f64_579_nop": ((5, 7, 9), np.float64, 4, (1, 2, 2), "no_pressure"),
    "f64_579_bool": ((5, 7, 9), np.float64, 1, (1, 2, 2), "bool"),
    "f64_579_dup": ((5, 7, 9), np.float64, 4, (1, 2, 2), "dup"),
    "f64_70": ((12, 20, 33), np.float64, 70, (2, 2, 3), None),
    "f32_70": ((12, 20, 33), np.float32, 70, (2, 2, 3), None),
    "f64_big": ((40, 48, 130), np.float64, 8, (6, 7, 9), None),
    "f32_big": ((40, 48, 130), np.float32, 8, (6, 7, 9), None),
}


def make_mask(shape, nlab, cell, rng):
    """Blobs of the labels 1..nlab on a coarse grid (so label-label faces exist), about half of it
    fluid; solid voxels on the first and the last plane, row and column (a wrap-around into the next
    row or plane would find them); a few negative voxels; the label nlab + 1 present in a few voxels
    (never asked for)."""
    coarse = tuple(-(-n // c) for n, c in zip(shape, cell))
    lab = rng.integers(1, nlab + 1, size=coarse)
    lab[rng.random(coarse) < 0.5] = 0
    m = lab
    for ax, c in enumerate(cell):
        m = np.repeat(m, c, axis=ax)
    m = np.ascontiguousarray(m[:shape[0], :shape[1], :shape[2]]).astype(np.int64)
    m[0, 0, :] = 1
    m[-1, -1, :] = nlab
    m[:, -1, -1] = 1
    m[-1, :, 0] = nlab
    m[0, :, -1] = 0
    flat = m.reshape(-1)
    pick = rng.choice(flat.size, size=max(2, flat.size // 50), replace=False)
    flat[pick[::2]] = -1
    flat[pick[1::2]] = nlab + 1
    return m


def make_case(name, seed=None):
    """dict(u, v, w, pressure, mask, labels, spacing, viscosity) of a named case.  The requested
    labels are 1..nlab and one absent label; nlab + 1 is in the mask and not requested."""
    shape, dtype, nlab, cell, special = CASES[name]
    return make_inputs(shape, dtype, nlab, cell, special, 1000 + list(CASES).index(name) if seed is None else seed)


def make_inputs(shape, dtype, nlab, cell, special, seed):
    rng = np.random.default_rng(seed)
    u, v, w = (rng.standard_normal(shape).astype(dtype) for _ in range(3))
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    pressure = (rng.standard_normal(shape) + 0.5 * x - 0.25 * z).astype(dtype)
    mask = make_mask(shape, nlab, cell, rng)
    labels = list(range(1, nlab + 1)) + [nlab + 50]
    if special == "no_pressure":
        pressure = None
    elif special == "bool":
        mask = mask == 1
        labels = None
    elif special == "dup":
        labels = [3, 1, 3, 2]
    return dict(u=u, v=v, w=w, pressure=pressure, mask=mask, labels=labels, spacing=SPACING, viscosity=VISCOSITY)


def make_perm_case(dtype, shape=(12, 20, 33), seed=77):
    """A pressure ramp plus noise and velocities with a mean: every one of the six sums has a
    condition S / |E| below 10 (the ramp's slopes and the means are well above the noise)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    dx, dy, dz = SPACING
    pressure = (-3.0 * x * dx + 2.0 * y * dy + 1.5 * z * dz + 0.05 * rng.standard_normal(shape)).astype(dtype)
    u = (1.0 + 0.3 * rng.standard_normal(shape)).astype(dtype)
    v = (-0.5 + 0.3 * rng.standard_normal(shape)).astype(dtype)
    w = (0.4 + 0.3 * rng.standard_normal(shape)).astype(dtype)
    return dict(u=u, v=v, w=w, pressure=pressure, spacing=SPACING, viscosity=VISCOSITY)


def checksum(case):
    """A fingerprint of the seeded inputs: a fixture made from other numbers must not pass."""
    tot = 0.0
    for k in ("u", "v", "w", "pressure"):
        if case.get(k) is not None:
            tot += math.fsum(np.asarray(case[k], dtype=np.float64).ravel())
    if "mask" in case:
        tot += float(np.asarray(case["mask"], dtype=np.int64).sum())
    return tot


def permeability_from_pressure(u, v, w, pressure, viscosity, dx, dy, dz):
    """The six exact sums (math.fsum of u, v, w and of np.gradient's x, y, z components), their
    conditions S / |E| and the value of the reference's expression (:673-697) evaluated from them."""
    gz, gy, gx = np.gradient(pressure, dz, dy, dx)
    sums, cond = [], []
    for a in (u, v, w, gx, gy, gz):
        a = np.asarray(a, dtype=np.float64).ravel()
        e, s = math.fsum(a), math.fsum(np.abs(a))
        sums.append(e)
        cond.append(s / abs(e) if e != 0 else (math.inf if s != 0 else 1.0))
    n = np.float64(np.asarray(u).size)
    u0 = np.array(sums[:3]) / n
    g = np.array(sums[3:]) / n
    mag2 = np.sum(g**2)
    k = 0.0 if mag2 == 0 else -viscosity * np.dot(u0, g) / mag2
    return sums, cond, k
