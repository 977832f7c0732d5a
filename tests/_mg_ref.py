"""numpy restatement of the multigrid preconditioner, written the way csrc/ptv_multigrid.hip computes it.

``z = M r`` is one symmetric V-cycle on the active (fluid, not Dirichlet) voxels of the anchored
pressure system.  Every operation below is elementwise float64 arithmetic or a sum of at most eight
terms taken in the kernel's order, so the device result is the same bits (tests/test_gpu_multigrid.py
demands them).  The operation order is stated at the head of ptv_multigrid.hip; in short, per cell

    d        = 0 + w(x-) + w(x+) + w(y-) + w(y+) + w(z-) + w(z+) + e
    (A z)_i  = (0 + w(x-) (z_x- - z_i) + ... + w(z+) (z_z+ - z_i)) - e z_i
    sweep      z_i <- z_i - (omega (r_i - (A z)_i)) / d        (from zero: 0 - (omega r_i) / d)
    restrict   r_C = 0 + the children's residuals, z slowest, x fastest
    prolong    z_i <- z_i + z_C

and a cell with d = 0 is outside the system (z = 0, residual 0, no correction).  A neighbour outside
the domain enters with weight 0, so its value (the device reads a clamped index, this file a zero)
does not matter for finite vectors.
"""
from __future__ import annotations

import numpy as np

NU, COARSE_SWEEPS, OMEGA = 2, 16, 2.0 / 3.0
MAX_LEVELS = 32
TAIL_CELLS = 4096
TAIL_LDS_BYTES = 152 * 1024
AXES = (2, 1, 0)  # the array axis of x, y, z


def _shift(a, step, axis, fill=0):
    """a[i + step] along axis, `fill` past the ends."""
    out = np.roll(a, -step, axis=axis)
    s = [slice(None)] * 3
    s[axis] = -1 if step == 1 else 0
    out[tuple(s)] = fill
    return out


class Level:
    """One level: the +x, +y, +z face weights (0 at the domain edge), the extra diagonal term, the
    diagonal."""

    def __init__(self, w, e):
        self.w = w  # [wx, wy, wz]
        self.e = e
        self.shape = e.shape
        d = np.zeros(self.shape)
        for k in range(3):
            d = d + _shift(w[k], -1, AXES[k])
            d = d + w[k]
        self.d = d + e
        self.inside = self.d != 0.0

    def apply(self, z):
        acc = np.zeros(self.shape)
        for k in range(3):
            ax = AXES[k]
            acc = acc + _shift(self.w[k], -1, ax) * (_shift(z, -1, ax) - z)
            acc = acc + self.w[k] * (_shift(z, 1, ax) - z)
        return acc - self.e * z

    def sweep(self, r, z, omega):
        d = np.where(self.inside, self.d, 1.0)
        if z is None:
            new = 0.0 - (omega * r) / d
        else:
            new = z - (omega * (r - self.apply(z))) / d
        return np.where(self.inside, new, 0.0)

    def residual(self, r, z):
        return np.where(self.inside, r - self.apply(z), 0.0)


def level0(mask, dirichlet, dx, dy, dz):
    mask = np.asarray(mask) != 0
    dirf = mask & (np.asarray(dirichlet) != 0) if dirichlet is not None else np.zeros(mask.shape, bool)
    act = mask & ~dirf
    ih2 = [1.0 / (h * h) for h in (dx, dy, dz)]
    w = []
    e = np.zeros(mask.shape)
    for k in range(3):
        ax = AXES[k]
        w.append(np.where(act & _shift(act, 1, ax, False), ih2[k], 0.0))
        for step in (-1, 1):
            e = e + np.where(act & _shift(dirf, step, ax, False), ih2[k], 0.0)
    return Level(w, e)


def _pad_even(a):
    return np.pad(a, [(0, n % 2) for n in a.shape])


def _children(a, c, b, x):
    return _pad_even(a)[c::2, b::2, x::2]


def coarsen(fine):
    """The Galerkin operator P^T A P of piecewise-constant 2 x 2 x 2 aggregation, in the kernel's
    summation order."""
    cshape = tuple((n + 1) // 2 for n in fine.shape)
    w = [np.zeros(cshape) for _ in range(3)]
    e = np.zeros(cshape)
    for c in range(2):
        for b in range(2):
            for a in range(2):
                if a == 1:
                    w[0] = w[0] + _children(fine.w[0], c, b, a)
                if b == 1:
                    w[1] = w[1] + _children(fine.w[1], c, b, a)
                if c == 1:
                    w[2] = w[2] + _children(fine.w[2], c, b, a)
                e = e + _children(fine.e, c, b, a)
    return Level(w, e)


def restrict(res):
    out = np.zeros(tuple((n + 1) // 2 for n in res.shape))
    for c in range(2):
        for b in range(2):
            for a in range(2):
                out = out + _children(res, c, b, a)
    return out


def prolong(level, z, zc):
    up = np.repeat(np.repeat(np.repeat(zc, 2, 0), 2, 1), 2, 2)[:z.shape[0], :z.shape[1], :z.shape[2]]
    return np.where(level.inside, z + up, z)


class Hierarchy:
    def __init__(self, mask, dirichlet, dx, dy, dz, max_levels=0, nu=0, coarse_sweeps=0, omega=0.0):
        self.nu = nu or NU
        self.coarse_sweeps = coarse_sweeps or COARSE_SWEEPS
        self.omega = omega or OMEGA
        cap = min(max_levels, MAX_LEVELS) if max_levels > 0 else MAX_LEVELS
        self.levels = [level0(mask, dirichlet, dx, dy, dz)]
        while max(self.levels[-1].shape) > 2 and len(self.levels) < cap:
            self.levels.append(coarsen(self.levels[-1]))
        self.shape = self.levels[0].shape

    # what the device reports in ptv_mg_stats
    def cells(self):
        return [int(np.prod(l.shape)) for l in self.levels]

    def active(self):
        return [int(l.inside.sum()) for l in self.levels]

    def tail_level(self):
        cells = [c + c % 2 for c in self.cells()]
        for l, c in enumerate(cells):
            if self.cells()[l] <= TAIL_CELLS and 8 * (c + 2 * sum(cells[l:])) <= TAIL_LDS_BYTES:
                return l
        return len(cells)

    def _sweeps(self, level, r, z, count):
        for _ in range(count):
            z = level.sweep(r, z, self.omega)
        return z

    def cycle(self, r, l=0):
        level = self.levels[l]
        if l == len(self.levels) - 1:
            return self._sweeps(level, r, None, self.coarse_sweeps)
        z = self._sweeps(level, r, None, self.nu)
        zc = self.cycle(restrict(level.residual(r, z)), l + 1)
        return self._sweeps(level, r, prolong(level, z, zc), self.nu)

    def apply(self, r):
        """z = M r on the grid."""
        return self.cycle(np.asarray(r, dtype=np.float64).reshape(self.shape))

    def operator(self, mask):
        """M on the compact fluid vector (the layout of _pressure_ref.laplacian_matrix), for scipy's
        cg(A, b, M=...); Dirichlet entries map to 0."""
        from scipy.sparse.linalg import LinearOperator

        mask = np.asarray(mask) != 0
        n = int(mask.sum())

        def matvec(rc):
            g = np.zeros(self.shape)
            g[mask] = np.asarray(rc, dtype=np.float64).ravel()
            return self.apply(g)[mask]

        return LinearOperator((n, n), matvec=matvec, dtype=np.float64)


def aggregation_matrix(fine_shape):
    """P (fine cells x coarse cells) of the 2 x 2 x 2 piecewise-constant aggregation, CSR."""
    from scipy import sparse

    cshape = tuple((n + 1) // 2 for n in fine_shape)
    Z, Y, X = np.meshgrid(*(np.arange(n) for n in fine_shape), indexing="ij")
    parent = ((Z // 2) * cshape[1] + (Y // 2)) * cshape[2] + (X // 2)
    nf = int(np.prod(fine_shape))
    return sparse.csr_matrix((np.ones(nf), (np.arange(nf), parent.ravel())), shape=(nf, int(np.prod(cshape))))


def level_matrix(level):
    """A level's operator as an explicit CSR matrix over all its cells (rows of cells with d = 0 are
    empty)."""
    from scipy import sparse

    n = int(np.prod(level.shape))
    idx = np.arange(n).reshape(level.shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [-level.d.ravel()]
    for k in range(3):
        ax = AXES[k]
        nb = _shift(idx, 1, ax, -1)
        ok = (nb >= 0) & (level.w[k] != 0.0)
        rows += [idx[ok], nb[ok]]
        cols += [nb[ok], idx[ok]]
        vals += [level.w[k][ok], level.w[k][ok]]
    A = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.eliminate_zeros()
    return A


def pcg(rhs, mask, dirichlet, dx, dy, dz, rtol=1e-10, maxiter=3000, dot=None, **mg):
    """The oracle: scipy's cg(A, b, M=V-cycle) on the explicit symmetric matrix with the Dirichlet rows
    and columns eliminated.  ``dot``: None for scipy's own (np.dot), or a function that replaces both
    inner products' summation (the recurrence restated, for the order gap).  Returns (p, itn, info)."""
    from scipy.sparse.linalg import cg

    import _pressure_ref as pref
    from _variational_ref import single_threaded_blas

    A = pref.laplacian_matrix(mask, dx, dy, dz, dirichlet, symmetric=True)
    b = rhs[mask].copy()
    b[dirichlet[mask]] = 0.0
    M = Hierarchy(mask, dirichlet, dx, dy, dz, **mg).operator(mask)
    p = np.zeros(mask.shape)
    if dot is None:
        itn = [0]

        def callback(_x):
            itn[0] += 1

        with single_threaded_blas():
            x, info = cg(A, b, rtol=rtol, atol=0.0, maxiter=maxiter, M=M, callback=callback)
        p[mask] = x
        return p, itn[0], int(info)
    # scipy's recurrence (_isolve/iterative.py, cg) with the inner products summed by `dot`
    x = np.zeros_like(b)
    r = b.copy()
    bnrm2 = np.sqrt(dot(b, b))
    if bnrm2 == 0:
        return p, 0, 0
    atol = rtol * bnrm2
    pvec = None
    rho_prev = None
    for it in range(maxiter):
        if np.sqrt(dot(r, r)) < atol:
            p[mask] = x
            return p, it, 0
        z = M.matvec(r)
        rho = dot(r, z)
        pvec = z.copy() if it == 0 else z + (rho / rho_prev) * pvec
        q = A @ pvec
        alpha = rho / dot(pvec, q)
        x = x + alpha * pvec
        r = r - alpha * q
        rho_prev = rho
    p[mask] = x
    return p, maxiter, maxiter


def chunked_dot(a, b, chunk=1000):
    """An inner product summed in another fixed order: numpy's sum within chunks of `chunk`
    products, then the chunk sums left to right."""
    prod = a * b
    total = 0.0
    for i in range(0, prod.size, chunk):
        total += float(np.sum(prod[i:i + chunk]))
    return total


# ---- the grids the CPU and GPU tests share ----
def os_path_golden(name):
    import os

    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"pressure_{name}.npz")


def _golden(name):
    g = np.load(os_path_golden(name), allow_pickle=False)
    return g["mask"], g["dirichlet"], (float(g["dx"]), float(g["dy"]), float(g["dz"])), g["rhs"]


def case(name):
    """(mask, dirichlet, (dx, dy, dz)) of a named test grid; arrays are (nz, ny, nx) bool."""
    sp = (1.0, 1.25, 0.8)
    rng = np.random.default_rng(11)
    if name in ("odd", "g12", "g20"):  # 7 x 9 x 33, 12 x 10 x 14, 20 x 18 x 24 blob masks of the pressure fixtures
        return _golden(name)[:3]
    if name == "half":  # 40 x 36 x 44, half filled at random, a Dirichlet plane: two levels above the tail
        mask = rng.uniform(size=(40, 36, 44)) > 0.5
        d = np.zeros_like(mask)
        d[-1] = True
        return mask, d & mask, sp
    if name == "half_unit":  # the same with unit spacings: every weight is an integer, every sum exact
        mask, d, _ = case("half")
        return mask, d, (1.0, 1.0, 1.0)
    if name in ("line5", "cube2", "col6"):  # extents of 1 and 2
        shape = {"line5": (1, 1, 5), "cube2": (2, 2, 2), "col6": (1, 6, 1)}[name]
        mask = np.ones(shape, bool)
        d = np.zeros(shape, bool)
        d.flat[0] = True
        return mask, d, sp
    if name == "pockets":  # an isolated active voxel and a fluid pocket with no path to a Dirichlet voxel
        mask = np.zeros((9, 8, 10), bool)
        mask[5:, :, :] = True          # the main body, anchored at its last plane
        mask[1, 1, 1] = True           # isolated: no fluid neighbour at all (zero diagonal)
        mask[1:3, 4:7, 5:9] = True     # a pocket: fluid, connected to nothing anchored
        mask[4] = False
        d = np.zeros_like(mask)
        d[-1] = True
        return mask, d & mask, sp
    if name == "plane":  # one plane, all of it Dirichlet: no active cell
        mask = np.random.default_rng(3).uniform(size=(1, 9, 12)) > 0.3
        return mask, mask.copy(), sp
    raise KeyError(name)


CASES = ["odd", "g20", "half", "line5", "cube2", "col6", "pockets", "plane"]
