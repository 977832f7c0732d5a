"""CPU oracle of the variational divergence cleaning (the project's own restatement of the
reference's physics.py:356-514; nothing here imports the reference).

Two forms of the same system (I + lambda D^T D) x = (u, v, w)[fluid]:

* ``csr``: the three divergence operators as CSR matrices, the six products and the 3 x 3 block
  matrix, built by the same sequence of scipy operations as the reference, so that scipy stores and
  sums the entries in the same order: bit-identical to the reference (tests/test_variational_oracle.py
  pins that against the fixtures);
* ``stencil``: the operator applied matrix-free with numpy slices, as the GPU kernels apply it.  Only
  the matvec's rounding order differs; the normwise difference of the two forms' results is the
  unit (``order_gap``) in which the GPU tests measure the device's difference from the oracle.

Both run scipy's ``cg(A, b, rtol=rtol, atol=0.0, maxiter=maxiter)`` and count iterations through
``callback``, with the BLAS library held to one thread (``single_threaded_blas``): cg's dot products
go through BLAS, whose threaded ddot (vectors of more than 10^4 entries) sums in an order that
depends on the thread count, so a fixture recorded with one thread count could not be reproduced
bit for bit under another.  Per axis with spacing h, for a fluid voxel i with neighbours i+ and i-: n+ = 1 if i+
is inside the grid and fluid, e+ = 1 if i+ is outside the grid (n-, e- likewise), and
    c_i = n+ (0.5/h) + e+ (1.0/h) - n- (0.5/h) - e- (1.0/h)
    (D v)_i   = c_i v_i + n+ (0.5/h) v_{i+} - n- (0.5/h) v_{i-}
    (D^T d)_j = c_j d_j + n- (0.5/h) d_{j-} - n+ (0.5/h) d_{j+}
"""
from __future__ import annotations

import numpy as np
from scipy import sparse
from scipy.sparse.linalg import LinearOperator, cg
from threadpoolctl import threadpool_limits

AXES = (2, 1, 0)  # x, y, z as array axes of a (nz, ny, nx) grid


def _shifted(mask, axis, step):
    """(inside, fluid): whether each voxel's neighbour at ``step`` along ``axis`` is inside the grid,
    and whether it is inside and fluid."""
    inside = np.ones(mask.shape, bool)
    fluid = np.zeros(mask.shape, bool)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
        edge = [slice(None)] * 3
        edge[axis] = slice(-1, None)
    else:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
        edge = [slice(None)] * 3
        edge[axis] = slice(0, 1)
    inside[tuple(edge)] = False
    fluid[tuple(dst)] = mask[tuple(src)]
    return inside, fluid


def diagonal(mask, axis, h):
    """c on the grid (0 at solid voxels), accumulated in the reference's order."""
    in_p, fl_p = _shifted(mask, axis, +1)
    in_m, fl_m = _shifted(mask, axis, -1)
    c = np.zeros(mask.shape)
    c += np.where(fl_p, 0.5 / h, 0.0)
    c += np.where(~in_p, 1.0 / h, 0.0)
    c -= np.where(fl_m, 0.5 / h, 0.0)
    c -= np.where(~in_m, 1.0 / h, 0.0)
    return np.where(mask, c, 0.0), fl_p & mask, fl_m & mask


def single_threaded_blas():
    """Context manager: BLAS on one thread, so that cg's dot products sum in one fixed order."""
    return threadpool_limits(limits=1, user_api="blas")


# ---- the CSR form ----------------------------------------------------------------------------
def csr_operators(mask, dx, dy, dz):
    """Dx, Dy, Dz over the fluid voxels in C order: per operator the diagonal entries, then the
    plus-neighbour entries, then the minus-neighbour entries, as one COO matrix turned into CSR."""
    n = int(mask.sum())
    index = np.full(mask.shape, -1, dtype=np.int32)
    index[mask] = np.arange(n)
    here = index[mask]
    ops = []
    for axis, h in zip(AXES, (dx, dy, dz)):
        c, fl_p, fl_m = diagonal(mask, axis, h)
        nb_p = np.roll(index, -1, axis=axis)[mask]
        nb_m = np.roll(index, +1, axis=axis)[mask]
        has_p, has_m = fl_p[mask], fl_m[mask]
        rows = np.concatenate([here, here[has_p], here[has_m]])
        cols = np.concatenate([here, nb_p[has_p], nb_m[has_m]])
        vals = np.concatenate([c[mask], np.full(int(has_p.sum()), 0.5 / h), np.full(int(has_m.sum()), -0.5 / h)])
        ops.append(sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr())
    return ops


def csr_system(mask, dx, dy, dz, lambda_reg):
    Dx, Dy, Dz = csr_operators(mask, dx, dy, dz)
    n = Dx.shape[0]
    eye = sparse.eye(n)
    xx, xy, xz = Dx.T @ Dx, Dx.T @ Dy, Dx.T @ Dz
    yy, yz, zz = Dy.T @ Dy, Dy.T @ Dz, Dz.T @ Dz
    return sparse.bmat([[eye + lambda_reg * xx, lambda_reg * xy, lambda_reg * xz],
                        [lambda_reg * xy.T, eye + lambda_reg * yy, lambda_reg * yz],
                        [lambda_reg * xz.T, lambda_reg * yz.T, eye + lambda_reg * zz]], format="csr")


# ---- the stencil form ------------------------------------------------------------------------
class Stencil:
    """absolute=True: the operators |Dx|, |Dy|, |Dz| (entrywise), for error bounds.  Arrays of
    np.longdouble are carried through in that precision (the coefficients stay the rounded doubles)."""

    def __init__(self, mask, dx, dy, dz, absolute=False):
        self.mask = mask
        self.h = (dx, dy, dz)
        self.neg = 1.0 if absolute else -1.0
        self.c, self.pairs = [], []
        for axis, h in zip(AXES, self.h):
            c, _, _ = diagonal(mask, axis, h)
            c = np.abs(c) if absolute else c
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            self.c.append(c)
            self.pairs.append((lo, hi, mask[lo] & mask[hi]))

    def div(self, grids):
        """Dx u + Dy v + Dz w on the grid (0 at solid voxels); grids: three (nz, ny, nx) arrays."""
        total = None
        for k, g in enumerate(grids):
            g = np.where(self.mask, g, 0.0)
            lo, hi, both = self.pairs[k]
            ch = 0.5 / self.h[k]
            out = self.c[k] * g
            out[lo] += np.where(both, ch * g[hi], 0.0)
            out[hi] += self.neg * np.where(both, ch * g[lo], 0.0)
            total = out if total is None else total + out
        return total

    def adjoint(self, d):
        """(Dx^T d, Dy^T d, Dz^T d) on the grid."""
        outs = []
        for k in range(3):
            lo, hi, both = self.pairs[k]
            ch = 0.5 / self.h[k]
            out = self.c[k] * d
            out[hi] += np.where(both, ch * d[lo], 0.0)
            out[lo] += self.neg * np.where(both, ch * d[hi], 0.0)
            outs.append(out)
        return outs

    def apply(self, grids, lambda_reg):
        """A x on the grid."""
        g = [np.where(self.mask, a, 0.0) for a in grids]
        t = self.adjoint(self.div(g))
        return [np.where(self.mask, a + lambda_reg * b, 0.0) for a, b in zip(g, t)]

    def operator(self, lambda_reg):
        mask = self.mask
        n = int(mask.sum())

        def matvec(x):
            x = np.asarray(x).ravel()
            grids = []
            for k in range(3):
                g = np.zeros(mask.shape)
                g[mask] = x[k * n:(k + 1) * n]
                grids.append(g)
            return np.concatenate([a[mask] for a in self.apply(grids, lambda_reg)])

        return LinearOperator((3 * n, 3 * n), matvec=matvec, rmatvec=matvec, dtype=np.float64)


def exact_products(x, mask, dx, dy, dz, lambda_reg):
    """In np.longdouble: d = D x, y = A x, and the magnitudes |D| |x| and |x| + lambda |D^T| |D| |x|
    that scale their rounding-error bounds (all on the grid; x: three grids)."""
    xl = [np.where(mask, a, 0.0).astype(np.longdouble) for a in x]
    st, sa = Stencil(mask, dx, dy, dz), Stencil(mask, dx, dy, dz, absolute=True)
    d = st.div(xl)
    y = [a + lambda_reg * b for a, b in zip(xl, st.adjoint(d))]
    ax = [np.abs(a) for a in xl]
    d_mag = sa.div(ax)
    y_mag = [a + lambda_reg * b for a, b in zip(ax, sa.adjoint(d_mag))]
    return d, y, d_mag, y_mag


# ---- the solve -------------------------------------------------------------------------------
def solve(u, v, w, mask, dx, dy, dz, lambda_reg=1e3, rtol=1e-8, maxiter=2000, form="csr"):
    """The cleaned fields (0 at solid voxels), the iterations completed and scipy's info."""
    mask = np.asarray(mask, bool)
    n = int(mask.sum())
    A = csr_system(mask, dx, dy, dz, lambda_reg) if form == "csr" else Stencil(mask, dx, dy, dz).operator(lambda_reg)
    b = np.concatenate([u[mask], v[mask], w[mask]])
    count = [0]

    def callback(_x):
        count[0] += 1

    with single_threaded_blas():
        sol, info = cg(A, b, rtol=rtol, atol=0.0, maxiter=maxiter, callback=callback)
    outs = []
    for k, a in enumerate((u, v, w)):
        g = np.zeros_like(a)
        g[mask] = sol[k * n:(k + 1) * n]
        outs.append(g)
    return outs, count[0], int(info)


def order_gap(a, b):
    """Normwise difference of two results (three fields each), relative to the first."""
    a, b = np.stack(a), np.stack(b)
    den = float(np.linalg.norm(a.ravel()))
    return float(np.linalg.norm((a - b).ravel())) / (den if den > 0 else 1.0)
