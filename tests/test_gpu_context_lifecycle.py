"""Context lifecycle: one call of every family on a fresh context, close(), and the same again.

The context owns every device buffer, event, pinned block and its stream through the owning types
of csrc/ptv_own.hpp, and ptv_free only deletes it.  This is the test that walks every owning member
through allocation and destruction: the second cycle's outputs must equal the first cycle's bit for
bit, and closing a closed context stays harmless."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 40          # 40^3 = 64000 points > 50000 with every axis >= 9: a coarse lattice is built
SLAB = (4, 40)  # 36 planes = 57600 points: the slab gets a lattice too (the slab culls need one)


def _one_cycle():
    from scipy.spatial import Delaunay

    from ptv_interpolation_amd import _lib, synth

    P, Q = synth.sphere_pack(5000, G, values="normal")
    ax = np.linspace(0.0, G - 1.0, G)
    small = np.linspace(0.0, G - 1.0, 16)
    rng = np.random.default_rng(5)
    out = {}
    ctx = _lib.Context(0)  # a fresh one, not the shared cached context
    try:
        out["idw8"] = ctx.interp_knn(P, Q, axes=(ax, ax, ax), k=8)
        # the cached cull map: built by the cold call, used and proven by the warm one, reused
        # without a host synchronisation by the speculative one
        for phase in ("cold", "warm", "speculative"):
            out["auto " + phase] = ctx.interp_knn(P, Q, axes=(ax, ax, ax), k=8, z_range=SLAB,
                                                  flags=_lib.FLAG_SLAB_CULL_AUTO)
            assert ctx.stats["halo_required"] == (-1.0 if phase == "cold" else 0.0), phase
            assert np.array_equal(out["auto " + phase][0], out["idw8"][0][SLAB[0]:SLAB[1]]), phase
        out["halo"] = ctx.interp_knn(P, Q, axes=(ax, ax, ax), k=8, z_range=SLAB, slab_halo=float(G))
        assert 0.0 <= ctx.stats["halo_required"] <= G
        out["k130"] = ctx.interp_knn(P, Q, axes=(small, small, small), k=130)
        out["rbf16"] = ctx.interp_rbf(P, Q, axes=(small, small, small), k=16)
        out["linear"] = ctx.interp_linear(P[:1500], Q[:1500], _lib.Triangulation(Delaunay(P[:1500])),
                                          axes=(small, small, small))
        out["filter"] = ctx.filter_outliers_knn(P, Q, k=25)
        f = [rng.standard_normal((12, 12, 12)) for _ in range(3)]
        fluid = rng.random((12, 12, 12)) > 0.2
        out["divergence"] = (ctx.divergence(*f, fluid, 1.0, 1.0, 1.0),)
        raw_axes = [np.arange(12.0)] * 3
        coarse = np.linspace(0.0, 11.0, 7)
        out["sample_mask"] = (ctx.sample_mask(fluid.view(np.uint8), raw_axes, axes=(coarse, coarse, coarse)),)
        out["boundary"] = ctx.boundary_particles(fluid.view(np.uint8), _lib.MASK_BOOL, 2, 3, [0.0] * 3, [11.0] * 3,
                                                 [11.0] * 3)
        assert len(out["boundary"][0]) > 0
        out["clean"], _ = ctx.clean_divergence(*f, fluid, 1.0, 1.0, 1.0, iterations=2)
        out["variational"], _ = ctx.clean_variational(*f, fluid, 1.0, 1.0, 1.0, lambda_reg=200.0, maxiter=20)
        out["pressure"] = (ctx.pressure_recover(*f, fluid, 1.0, 1.0, 1.0, 1e-3, maxiter=20)[0],)
        flow, _ = ctx.flow_analysis(*f, 1.0, 1.0, 1.0, viscosity=1e-3, fluid_mask=fluid)
        out["flow"] = tuple(flow[name] for name in _lib.FLOW_OUTPUTS)
        grains = rng.integers(0, 3, (12, 12, 12)).astype(np.int32)
        as_bytes = lambda rec: np.frombuffer(rec.tobytes(), dtype=np.uint8)  # noqa: E731  (record arrays)
        out["drag"] = (as_bytes(ctx.interface_drag(grains, *f, None, 1e-3, 1.0, 1.0, 1.0, [1, 2])[0]),)
        d2, dist, _ = ctx.edt(fluid.view(np.uint8), keep_distance=True)
        out["edt"] = (d2, dist)
        out["align"] = (as_bytes(ctx.align_score((12, 12, 12), 30, rng.standard_normal((4, 3)),
                                                 points=rng.random((30, 3)) * 11.0)[0]),)  # against the kept field
        coords = rng.random((3, 25)) * 11.0
        out["spline"] = (ctx.spline_prefilter(f[0])[0], ctx.map_coordinates(f[0], coords)[0],
                         ctx.map_coordinates(None, coords, shape=(12, 12, 12))[0])  # the resident coefficients
        labels, sizes, _ = ctx.label(fluid.view(np.uint8), connectivity=26, want_sizes=True)
        out["label"] = (labels, sizes)
        nv, nt, _ = ctx.marching_cubes(grains, [1, 2])
        out["marching cubes"] = (nv, nt) + tuple(a for pair in ctx.surface_fetch(nv, nt) for a in pair)
    finally:
        ctx.close()
    ctx.close()  # already closed
    ctx.close()
    assert ctx.h is None
    return out


def test_two_context_lifetimes_give_the_same_bits():
    first = _one_cycle()
    second = _one_cycle()
    assert first.keys() == second.keys()
    for name in first:
        for a, b in zip(first[name], second[name]):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name
