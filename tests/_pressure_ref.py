"""numpy restatement of the pressure recovery, written the way csrc/ptv_pressure.hip computes it.

The force field (velocity_analysis.py:210-289) and the force divergence (physics.py:211-262) are
elementwise chains, restated here operation for operation: the fixtures hold the reference's own
results and ``test_pressure_oracle.py`` demands the same bits.  The anchored Poisson solve is
scipy's ``cg`` on the matrix-free operator of the symmetric system whose Dirichlet rows and columns
are eliminated; ``laplacian_matrix`` builds the explicit CSR matrices the identity test compares.
"""
from __future__ import annotations

import numpy as np

SOLID, BULK, FILL1, FILL2, OPEN = 0, 1, 2, 3, 4
RTOL, MAXITER = 1e-10, 3000
LSQR = dict(damp=1e-8, atol=1e-10, btol=1e-10, iter_lim=3000)


def _shift(a, step, axis, wrap, fill):
    """a[i + step] along axis: wrapped around the domain, or `fill` past the ends."""
    out = np.roll(a, -step, axis=axis)
    if not wrap:
        s = [slice(None)] * 3
        s[axis] = -1 if step == 1 else 0
        out[tuple(s)] = fill
    return out


def _clamped(f, step, axis):
    out = np.roll(f, -step, axis=axis)
    s = [slice(None)] * 3
    s[axis] = -1 if step == 1 else 0
    out[tuple(s)] = f[tuple(s)]
    return out


def raw_laplacian(f, dx, dy, dz):
    lap = np.zeros_like(f)
    for axis, h in ((0, dz), (1, dy), (2, dx)):
        lap = lap + ((_clamped(f, 1, axis) - 2 * f) + _clamped(f, -1, axis)) / (h * h)
    return lap


def voxel_codes(mask):
    """0 solid, 1 bulk (fluid with six fluid neighbours inside the domain), 4 fluid not bulk."""
    bulk = mask.copy()
    for axis in range(3):
        for step in (1, -1):
            bulk &= _shift(mask, step, axis, False, False)
    code = np.where(mask, OPEN, SOLID).astype(np.uint8)
    code[bulk] = BULK
    return code


def fill_round(laps, code, top, wrap=True):
    """One fill round on the three Laplacians: OPEN voxels average their neighbours of code 1..top in
    the order z+1, z-1, y+1, y-1, x+1, x-1.  Returns (new laps, which voxels were filled)."""
    sums = [np.zeros_like(laps[0]) for _ in laps]
    count = np.zeros_like(laps[0])
    for axis in range(3):
        for step in (1, -1):
            cn = _shift(code, step, axis, wrap, SOLID)
            ok = (code == OPEN) & (cn >= BULK) & (cn <= top)
            for k, lap in enumerate(laps):
                sums[k][ok] += _shift(lap, step, axis, wrap, 0.0)[ok]
            count[ok] += 1
    hit = count > 0
    out = []
    for k, lap in enumerate(laps):
        new = lap.copy()
        new[hit] = sums[k][hit] / count[hit]
        out.append(new)
    return out, hit


def filled_laplacians(u, v, w, dx, dy, dz, mask, wrap=True):
    laps = [raw_laplacian(f, dx, dy, dz) for f in (u, v, w)]
    code = voxel_codes(mask)
    if not (code == BULK).any():
        return laps
    laps, hit = fill_round(laps, code, BULK, wrap)
    code[hit] = FILL1
    laps, _ = fill_round(laps, code, FILL1, wrap)
    return laps


def force_field(u, v, w, dx, dy, dz, mu, rho, mask, wrap=True):
    laps = filled_laplacians(u, v, w, dx, dy, dz, mask, wrap)
    f = [mu * lap for lap in laps]
    if rho > 0:
        for k, c in enumerate((u, v, w)):
            gz, gy, gx = np.gradient(c, dz, dy, dx)
            f[k] = f[k] - rho * ((u * gx + v * gy) + w * gz)
    return tuple(f)


def _flux_term(f, mask, axis, h, inhom):
    n = f.shape[axis]
    cur = [slice(None)] * 3
    nxt = [slice(None)] * 3
    cur[axis] = slice(0, n - 1)
    nxt[axis] = slice(1, n)
    cur, nxt = tuple(cur), tuple(nxt)
    fc, fn, mc, mn = f[cur], f[nxt], mask[cur], mask[nxt]
    face = np.where(mc & mn, 0.5 * (fc + fn), 0.0)
    if inhom:
        face = np.where(mc & ~mn, fc, face)
        face = np.where(mn & ~mc, fn, face)
    hi = np.zeros_like(f)
    lo = np.zeros_like(f)
    hi[cur] = face
    lo[nxt] = face
    return (hi - lo) / h


def force_divergence(fx, fy, fz, mask, dx, dy, dz, wall_bc="zero-neumann"):
    inhom = wall_bc == "inhomogeneous"
    return (_flux_term(fx, mask, 2, dx, inhom) + _flux_term(fy, mask, 1, dy, inhom)) + _flux_term(fz, mask, 0, dz, inhom)


def laplacian_apply(x, mask, dx, dy, dz):
    """(A x)_i = sum over fluid face neighbours inside the domain of (x_j - x_i) / h**2 on the grid,
    in the kernel's term order x-, x+, y-, y+, z-, z+; 0 at solid voxels."""
    acc = np.zeros_like(x)
    for axis, h in ((2, dx), (1, dy), (0, dz)):
        ih2 = 1.0 / (h * h)
        for step in (-1, 1):
            ok = mask & _shift(mask, step, axis, False, False)
            acc[ok] += ((_shift(x, step, axis, False, 0.0) - x) * ih2)[ok]
    return acc


def slice_operator(mask, dirichlet, dx, dy, dz):
    """The eliminated system as a LinearOperator on the compact fluid vector: the Laplacian on the
    active (fluid, not Dirichlet) entries, the identity on the Dirichlet ones."""
    from scipy.sparse.linalg import LinearOperator

    n = int(mask.sum())
    d = dirichlet[mask]

    def matvec(xc):
        g = np.zeros(mask.shape)
        xc = np.asarray(xc, dtype=np.float64).ravel()
        g[mask] = np.where(d, 0.0, xc)
        y = laplacian_apply(g, mask, dx, dy, dz)[mask]
        return np.where(d, xc, y)

    return LinearOperator((n, n), matvec=matvec, dtype=np.float64)


def cg_solve(rhs, mask, dirichlet, dx, dy, dz, rtol=RTOL, maxiter=MAXITER):
    """scipy's cg on the slice operator; returns (p grid, itn, info)."""
    from scipy.sparse.linalg import cg

    from _variational_ref import single_threaded_blas

    b = rhs[mask].copy()
    b[dirichlet[mask]] = 0.0
    itn = [0]

    def callback(_x):
        itn[0] += 1

    with single_threaded_blas():
        x, info = cg(slice_operator(mask, dirichlet, dx, dy, dz), b, rtol=rtol, atol=0.0, maxiter=maxiter,
                     callback=callback)
    p = np.zeros(mask.shape)
    p[mask] = x
    return p, itn[0], int(info)


def anchor_plane(shape, anchor, flow_direction, w, mask):
    """The z index of the Dirichlet plane (velocity_analysis.py:304-321), None for anchor='none'."""
    if anchor == "none":
        return None
    if flow_direction == "positive":
        positive = True
    elif flow_direction == "negative":
        positive = False
    else:
        positive = bool(np.mean(w[mask]) >= 0)
    last = (anchor == "outlet") == positive
    return shape[0] - 1 if last else 0


def dirichlet_grid(mask, plane):
    d = np.zeros(mask.shape, dtype=bool)
    if plane is not None:
        d[plane] = True
    return d & mask


def laplacian_matrix(mask, dx, dy, dz, dirichlet=None, symmetric=False):
    """The explicit CSR Laplacian over the fluid voxels.  With a Dirichlet set: its rows become the
    identity (what the reference builds); symmetric=True clears its columns too."""
    from scipy import sparse

    n = int(mask.sum())
    idx = np.full(mask.shape, -1, dtype=np.int64)
    idx[mask] = np.arange(n)
    rows, cols, vals = [], [], []
    for axis, h in ((2, dx), (1, dy), (0, dz)):
        ih2 = 1.0 / (h ** 2)
        for step in (-1, 1):
            nb = _shift(idx, step, axis, False, -1)
            ok = mask & (nb >= 0)
            rows += [idx[ok], idx[ok]]
            cols += [nb[ok], idx[ok]]
            vals += [np.full(int(ok.sum()), ih2), np.full(int(ok.sum()), -ih2)]
    A = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    if dirichlet is not None and dirichlet[mask].any():
        d = dirichlet[mask]
        keep = sparse.diags((~d).astype(np.float64))
        A = keep @ A @ keep if symmetric else keep @ A
        A = (A + sparse.diags(d.astype(np.float64))).tocsr()
        A.eliminate_zeros()
    return A


def normwise(a, b):
    den = np.linalg.norm(b.ravel())
    return float(np.linalg.norm((a - b).ravel()) / den) if den > 0 else float(np.linalg.norm((a - b).ravel()))
