"""The calls of the grid-field families whose host entry points stage through the context's pool,
each through its host entry point (numpy arrays) and through its ``_dev`` entry point (torch
tensors).  Shared by tests/test_gpu_host_staging.py and tools/host_staging_hash.py.

``CASES`` maps a name to ``(dtypes, fn)``; ``fn(ctx, inputs, on_dev)`` returns ``(arrays, stats)``,
the output arrays and the stats dict (or None) of the one call.  ``same(a, b)`` compares two such
results bit for bit, leaving the timings out of the stats."""
import numpy as np

H = (0.7, 1.1, 1.3)  # dx, dy, dz
SHAPES = [(5, 4, 2), (7, 9, 13)]  # (nz, ny, nx): even nx takes the two-wide path, odd nx the one-wide
TABLE = [1, 2]  # labels of the drag and the marching cubes
ITERS = 40


class Inputs:
    def __init__(self, shape, dtype=np.float64):
        from ptv_interpolation_amd import _lib

        rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2])
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.code = _lib.F32 if self.dtype == np.float32 else _lib.F64
        self.nz, self.ny, self.nx = shape
        self.mask = rng.random(shape) < 0.8
        self.mask.flat[0] = True
        self.f = [rng.standard_normal(shape).astype(dtype) for _ in range(4)]  # u, v, w, p / phi
        self.dirichlet = (rng.random(shape) < 0.1) & self.mask
        self.labels = rng.integers(0, 3, shape).astype(np.int32)
        self.solid = (rng.random(shape) < 0.7).astype(np.uint8)
        self.solid.flat[-1] = 0
        self.dt = np.abs(rng.standard_normal(shape))
        self.points = rng.random((20, 3)) * np.array(shape[::-1], dtype=np.float64)
        self.offsets = rng.standard_normal((5, 3))
        self.coords = rng.random((3, 17)) * (np.array(shape, dtype=np.float64)[:, None] + 1.0) - 0.5


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(shape, like):
    import torch

    return torch.empty(shape, dtype=torch.from_numpy(np.zeros(1, dtype=like)).dtype, device="cuda")


def _back(*ts):
    import torch

    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def divergence(ctx, d, on_dev):
    if not on_dev:
        return [ctx.divergence(*d.f[:3], d.mask, *H)], dict(ctx.stats)
    t, m, o = [_t(a) for a in d.f[:3]], _t(d.mask.view(np.uint8)), _empty(d.shape, d.dtype)
    st = ctx.divergence_dev(d.nx, d.ny, d.nz, _ptrs(t), m.data_ptr(), o.data_ptr(), *H, field_dtype=d.code,
                            result_dtype=d.code)
    return _back(o), st


def _solver(host, dev, n_out, **kw):
    """A call of three float64 fields and the mask into n_out grids."""
    def fn(ctx, d, on_dev):
        if not on_dev:
            res = getattr(ctx, host)(*d.f[:3], d.mask, *H, **kw)
            arrays, st = res if isinstance(res, tuple) and isinstance(res[1], dict) else (res, None)
            return list(arrays) if isinstance(arrays, (tuple, list)) else [arrays], st
        t, m = [_t(a) for a in d.f[:3]], _t(d.mask.view(np.uint8))
        o = [_empty(d.shape, np.float64) for _ in range(n_out)]
        st = getattr(ctx, dev)(d.nx, d.ny, d.nz, _ptrs(t), m.data_ptr(), _ptrs(o) if n_out > 1 else o[0].data_ptr(),
                               *H, **kw)
        return _back(*o), st
    return fn


def _poisson(**kw):
    def fn(ctx, d, on_dev):
        use_rhs, use_dir = kw.get("rhs", True), kw.get("dirichlet", True)
        solver = {k: v for k, v in kw.items() if k not in ("rhs", "dirichlet")}
        if not on_dev:
            x, st = ctx.poisson_solve(d.mask, *H, rhs=d.f[3] if use_rhs else None,
                                      force_field=None if use_rhs else d.f[:3],
                                      dirichlet=d.dirichlet if use_dir else None, **solver)
            return [x], st
        m, o, dr = _t(d.mask.view(np.uint8)), _empty(d.shape, np.float64), _t(d.dirichlet.view(np.uint8))
        src = [_t(d.f[3])] if use_rhs else [_t(a) for a in d.f[:3]]
        st = ctx.poisson_solve_dev(d.nx, d.ny, d.nz, m.data_ptr(), o.data_ptr(), *H,
                                   rhs_ptr=src[0].data_ptr() if use_rhs else 0,
                                   force_ptrs=None if use_rhs else _ptrs(src),
                                   dirichlet_ptr=dr.data_ptr() if use_dir else 0, **solver)
        return _back(o), st
    return fn


def flow_analysis(ctx, d, on_dev):
    from ptv_interpolation_amd import _lib

    if not on_dev:
        out, st = ctx.flow_analysis(*d.f[:3], *H, viscosity=1e-3, fluid_mask=d.mask)
        return [out[n] for n in _lib.FLOW_OUTPUTS], st
    t, m = [_t(a) for a in d.f[:3]], _t(d.mask.view(np.uint8))
    o = [_empty(d.shape, d.dtype) for _ in _lib.FLOW_OUTPUTS]
    st = ctx.flow_analysis_dev(d.nx, d.ny, d.nz, _ptrs(t), _ptrs(o), *H, viscosity=1e-3, mask_ptr=m.data_ptr(),
                               field_dtype=d.code)
    return _back(*o), st


def flow_derived(ctx, d, on_dev):
    s, o = np.abs(d.f[0]).reshape(-1), np.abs(d.f[1]).reshape(-1)  # a flat list: one shape for both entry points
    mk = d.mask.reshape(-1)
    if not on_dev:
        out, st = ctx.flow_derived(s, o, viscosity=1e-3, fluid_mask=mk)
        return [out["dissipation"], out["flow_type"]], st
    ts, to, m = _t(s), _t(o), _t(mk.view(np.uint8))
    r = [_empty(s.shape, d.dtype) for _ in range(2)]
    st = ctx.flow_derived_dev(s.size, ts.data_ptr(), to.data_ptr(), r[0].data_ptr(), r[1].data_ptr(), viscosity=1e-3,
                              mask_ptr=m.data_ptr(), field_dtype=d.code)
    return _back(*r), st


def interface_drag(ctx, d, on_dev):
    if not on_dev:
        return [ctx.interface_drag(d.labels, *d.f[:3], d.f[3], 1e-3, *H, TABLE)[0]], None
    t, m = [_t(a) for a in d.f], _t(d.labels)
    rec, _ = ctx.interface_drag_dev(d.nx, d.ny, d.nz, m.data_ptr(), _ptrs(t[:3]), t[3].data_ptr(), 1e-3, *H, TABLE,
                                    field_dtype=d.code)
    return [rec], None


def gradient_sums(ctx, d, on_dev):
    if not on_dev:
        return [np.array(ctx.gradient_sums(d.f[3], *H))], None
    t = _t(d.f[3])
    return [np.array(ctx.gradient_sums_dev(d.nx, d.ny, d.nz, t.data_ptr(), *H, field_dtype=d.code))], None


def edt(ctx, d, on_dev):
    if not on_dev:
        d2, dist, st = ctx.edt(d.solid)
        return [d2, dist], st
    m, d2, dist = _t(d.solid), _empty(d.shape, np.int32), _empty(d.shape, np.float64)
    st = ctx.edt_dev(d.nx, d.ny, d.nz, m.data_ptr(), d2.data_ptr(), dist.data_ptr())
    return _back(d2, dist), st


def align_score(ctx, d, on_dev):
    if not on_dev:
        return [ctx.align_score(d.shape, len(d.points), d.offsets, points=d.points, dt=d.dt)[0]], None
    p, f = _t(d.points), _t(d.dt)
    return [ctx.align_score_dev(d.shape, len(d.points), p.data_ptr(), f.data_ptr(), d.offsets)[0]], None


def label(ctx, d, on_dev):
    from ptv_interpolation_amd import _lib

    if not on_dev:
        lab, sizes, st = ctx.label(d.solid, connectivity=18, want_sizes=True)
        return [lab, sizes], st
    m, lab = _t(d.solid), _empty(d.shape, np.int32)
    sizes = _empty((_lib.label_sizes_room(d.solid.size),), np.int64)
    st = ctx.label_dev(d.nx, d.ny, d.nz, m.data_ptr(), lab.data_ptr(), connectivity=18, sizes_ptr=sizes.data_ptr())
    lab, sizes = _back(lab, sizes)
    return [lab, sizes[:st["n_components"] + 1]], st


def marching_cubes(ctx, d, on_dev):
    if not on_dev:
        nv, nt, _ = ctx.marching_cubes(d.labels, TABLE)
    else:
        m = _t(d.labels)
        nv, nt, _ = ctx.marching_cubes_dev(d.nx, d.ny, d.nz, m.data_ptr(), TABLE)
    return [nv, nt] + [a for pair in ctx.surface_fetch(nv, nt) for a in pair], None


def spline_prefilter(ctx, d, on_dev):
    from ptv_interpolation_amd import _lib

    if not on_dev:
        return [ctx.spline_prefilter(d.f[0])[0]], None
    t = _t(d.f[0])
    coef = _empty(tuple(n + 2 * _lib.SPLINE_PAD for n in d.shape), np.float64)
    ctx.spline_prefilter_dev(d.nx, d.ny, d.nz, t.data_ptr(), coef.data_ptr(), field_dtype=d.code)
    return _back(coef), None


def _map_coordinates(order):
    def fn(ctx, d, on_dev):
        if not on_dev:
            return [ctx.map_coordinates(d.f[0], d.coords, order=order)[0]], None
        t, co, o = _t(d.f[0]), _t(d.coords), _empty((d.coords.shape[1],), np.float64)
        ctx.map_coordinates_dev(d.nx, d.ny, d.nz, t.data_ptr(), co.data_ptr(), d.coords.shape[1], o.data_ptr(),
                                order=order, field_dtype=d.code)
        return _back(o), None
    return fn


BOTH, F64 = (np.float32, np.float64), (np.float64,)
CASES = {
    "divergence": (BOTH, divergence),
    "clean": (F64, _solver("clean_divergence", "clean_divergence_dev", 3, iterations=2, iter_lim=ITERS)),
    "variational": (F64, _solver("clean_variational", "clean_variational_dev", 3, lambda_reg=200.0, maxiter=ITERS)),
    "force field": (F64, _solver("force_field", "force_field_dev", 3, mu=1e-3, rho=1.2)),
    "force divergence": (F64, _solver("force_divergence", "force_divergence_dev", 1, wall_bc="inhomogeneous")),
    "poisson cg rhs": (F64, _poisson(maxiter=ITERS)),
    "poisson cg force": (F64, _poisson(rhs=False, maxiter=ITERS)),
    "poisson lsqr rhs": (F64, _poisson(dirichlet=False, iter_lim=ITERS)),
    "pressure": (F64, _solver("pressure_recover", "pressure_recover_dev", 1, mu=1e-3, maxiter=ITERS)),
    "flow analysis": (BOTH, flow_analysis),
    "flow derived": (BOTH, flow_derived),
    "interface drag": (BOTH, interface_drag),
    "gradient sums": (BOTH, gradient_sums),
    "edt": (F64, edt),
    "align score": (F64, align_score),
    "label": (F64, label),
    "marching cubes": (F64, marching_cubes),
    "spline prefilter": (BOTH, spline_prefilter),
    "map_coordinates order 0": (BOTH, _map_coordinates(0)),
    "map_coordinates order 1": (BOTH, _map_coordinates(1)),
    "map_coordinates order 3": (BOTH, _map_coordinates(3)),
}


def untimed(st):
    """The stats without the timings."""
    return {k: v for k, v in (st or {}).items() if k != "ms" and not k.startswith("ms_")}


def same(a, b):
    """Two results of a case: the same arrays, byte for byte, and the same stats but for the timings."""
    (xa, sa), (xb, sb) = a, b
    return (len(xa) == len(xb) and
            all(p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(xa, xb)) and
            repr(untimed(sa)) == repr(untimed(sb)))
