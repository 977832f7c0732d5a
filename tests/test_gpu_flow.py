"""GPU parity of the flow analysis (csrc/ptv_flow.hip behind ``ptv_flow_analysis`` /
``ptv_flow_derived``): the shear-rate magnitude, the viscous dissipation, the vorticity magnitude and
the Astarita flow type, bit for bit against the reference's fixtures (tests/golden/flow_*.npz) and,
off their shapes, against the numpy restatement that test_flow_oracle.py holds to those fixtures;
and the statistics of the same pass.

Shapes are the smallest that reach every path of the kernel: a lane owns 2 (float64) or 4 (float32)
consecutive x when nx allows and every buffer is 16-byte aligned, else 1; a block covers 64 lanes x 4
rows; a thread column marches kFlowPlanes = 32 planes, loading kFlowBatch = 2 at a time.
"""
import glob
import itertools
import math
import os
import warnings

import numpy as np
import pytest

import _flow_ref as fref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "flow_*.npz")))
OUTPUTS = fref.OUTPUTS
PLANES, BATCH = 32, 2  # kFlowPlanes, kFlowBatch of ptv_flow.hip
H = (0.3, 1.1, 0.7)    # dx, dy, dz: anisotropic, none a float32 value (the two division rules differ)
VISC = 1.5e-3


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


@pytest.fixture(scope="module")
def va():
    from ptv_interpolation_amd import velocity_analysis

    return velocity_analysis


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _random_case(shape, dtype, seed, mask=True):
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(shape).astype(dtype) for _ in range(3)]
    return f, (rng.random(shape) < 0.7 if mask else None)


def _spacings(strong):
    return tuple((np.float64 if strong else float)(h) for h in H)


def _check_stats(st, fields, mask, uvw=None):
    """max, min and the counts exactly; every sum within n 2^-53 sum|x| of math.fsum, a bound that
    holds for every order of summation: it catches a voxel missed or counted twice at a seam."""
    any_field = next(iter(fields.values())) if fields else uvw[0]
    n = any_field.size
    assert st["n_voxels"] == n
    assert st["n_fluid"] == (n if mask is None else int(np.count_nonzero(mask)))

    def bound_ok(got, x):
        x = np.asarray(x, dtype=np.float64).ravel()
        if not np.isfinite(x).all():
            return
        assert abs(got - math.fsum(x)) <= x.size * 2.0**-53 * math.fsum(np.abs(x)), (got, math.fsum(x))

    if uvw is not None:
        for name, a in zip(("sum_u", "sum_v", "sum_w"), uvw):
            bound_ok(st[name], a)
    for name in OUTPUTS:
        if name not in fields:
            assert st["sum"][name] == 0.0 and st["max"][name] == 0.0 and st["min"][name] == 0.0, name
            continue
        x = fields[name]
        assert np.array_equal(np.float64(st["max"][name]), np.float64(_quiet(np.max, x)), equal_nan=True), name
        assert np.array_equal(np.float64(st["min"][name]), np.float64(_quiet(np.min, x)), equal_nan=True), name
        bound_ok(st["sum"][name], x)
        bound_ok(st["sum_fluid"][name], x if mask is None else x[mask])


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", CASES)
def test_fixture_fused_call(va, name):
    """The host entry through the fused call: one pass, four fields."""
    c = fref.load_case(os.path.join(GOLDEN, f"flow_{name}.npz"))
    got = _quiet(va.analyze, c["u"], c["v"], c["w"], c["dx"], c["dy"], c["dz"], c["viscosity"], c["mask"])
    for out in OUTPUTS:
        assert fref.same(got[out], c[out]), (name, out)
    uvw = [np.asarray(c[k], dtype=np.float64) for k in "uvw"]
    _check_stats(got["stats"], {k: got[k] for k in OUTPUTS}, c["mask"], uvw)


@pytest.mark.parametrize("name", CASES)
def test_fixture_per_function_wrappers(va, name):
    c = fref.load_case(os.path.join(GOLDEN, f"flow_{name}.npz"))
    args = (c["u"], c["v"], c["w"], c["dx"], c["dy"], c["dz"])
    assert fref.same(_quiet(va.compute_strain_rate, *args, mask=c["mask"]), c["strain_rate"])
    assert fref.same(_quiet(va.compute_vorticity, *args, mask=c["mask"]), c["vorticity"])
    assert fref.same(_quiet(va.compute_viscous_dissipation, c["strain_rate"], c["viscosity"], *args[3:],
                            mask=c["mask"]), c["dissipation"])
    assert fref.same(_quiet(va.compute_astarita_flow_type, c["strain_rate"], c["vorticity"], mask=c["mask"]),
                     c["flow_type"])


# ---------------------------------------------------------------- seams
SEAMS = [
    # dtype, (nz, ny, nx), np.float64 spacings
    (np.float64, (BATCH + 1, 5, 130), False),   # two x tiles of 2-wide lanes; one row past a block; batch + 1 planes
    (np.float64, (BATCH + 1, 5, 131), False),   # odd nx: the scalar path, three x tiles
    (np.float64, (PLANES + 1, 3, 6), False),    # one plane past a thread column
    (np.float32, (BATCH + 1, 5, 260), False),   # two x tiles of 4-wide lanes
    (np.float32, (BATCH + 1, 5, 262), True),    # nx % 4 != 0: the scalar path; float64 division
    (np.float32, (PLANES + 1, 9, 8), True),
    (np.float32, (2 * PLANES + 1, 2, 4), False),
]


@pytest.mark.parametrize("dtype, shape, strong", SEAMS)
@pytest.mark.parametrize("masked", [True, False])
def test_seams_against_the_restatement(ctx, dtype, shape, strong, masked):
    f, m = _random_case(shape, dtype, sum(shape), masked)
    h = _spacings(strong)
    want = fref.analyze(*f, *h, VISC, m)
    got, st = ctx.flow_analysis(*f, *h, viscosity=VISC, fluid_mask=m, spacing_strong=strong)
    for out in OUTPUTS:
        assert fref.same(got[out], want[out]), out
    _check_stats(st, got, m, f)


def test_unaligned_device_pointers_take_the_scalar_path(ctx):
    """Device buffers that start one element past a 16-byte boundary, on an even nx."""
    import torch

    from ptv_interpolation_amd import _lib

    for dtype, tdt, code in ((np.float64, torch.float64, _lib.F64), (np.float32, torch.float32, _lib.F32)):
        shape = (5, 6, 136)
        n = int(np.prod(shape))
        f, m = _random_case(shape, dtype, 11)
        want = fref.analyze(*f, *H, VISC, m)
        flat = [torch.zeros(n + 4, dtype=tdt, device="cuda") for _ in range(7)]
        for t, a in zip(flat, f):
            t[1:n + 1] = torch.from_numpy(a.ravel()).cuda()
        views = [t[1:n + 1] for t in flat]
        assert all(v.data_ptr() % 16 != 0 for v in views)
        dm = torch.from_numpy(m.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        st = ctx.flow_analysis_dev(shape[2], shape[1], shape[0], [v.data_ptr() for v in views[:3]],
                                   [v.data_ptr() for v in views[3:]], *H, viscosity=VISC, mask_ptr=dm.data_ptr(),
                                   field_dtype=code, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy().reshape(shape) for k, v in zip(OUTPUTS, views[3:])}
        for out in OUTPUTS:
            assert fref.same(got[out], want[out]), (dtype, out)
        for t in flat[3:]:  # nothing written before or after the views
            assert float(t[0]) == 0.0 and not t[n + 1:].any()
        _check_stats(st, got, m, f)


# ---------------------------------------------------------------- z-slabs
def test_zslabs_with_halos_equal_the_whole(ctx):
    """A (12, 6, 16) grid cut at every z into two slabs, each with a one-plane halo on its interior
    side: the fields equal the whole-grid result and the counts add up."""
    shape = (12, 6, 16)
    f, m = _random_case(shape, np.float64, 5)
    whole, sw = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m)
    for out in OUTPUTS:
        assert fref.same(whole[out], fref.analyze(*f, *H, VISC, m)[out])
    for cut in range(1, shape[0]):
        flo, slo = ctx.flow_analysis(*(a[:cut + 1] for a in f), *H, viscosity=VISC, fluid_mask=m[:cut + 1],
                                     z_range=(0, cut), edges=(True, False))
        fhi, shi = ctx.flow_analysis(*(a[cut - 1:] for a in f), *H, viscosity=VISC, fluid_mask=m[cut - 1:],
                                     z_range=(1, shape[0] - cut + 1), edges=(False, True))
        for out in OUTPUTS:
            assert np.array_equal(np.concatenate([flo[out], fhi[out]]), whole[out]), (cut, out)
        assert slo["n_voxels"] + shi["n_voxels"] == sw["n_voxels"] == m.size
        assert slo["n_fluid"] + shi["n_fluid"] == sw["n_fluid"] == int(m.sum())
        _check_stats(slo, flo, m[:cut], [a[:cut] for a in f])
        _check_stats(shi, fhi, m[cut:], [a[cut:] for a in f])


def test_rejects_a_missing_halo_and_short_axes(ctx):
    u = np.zeros((6, 4, 4))
    with pytest.raises(ValueError, match="halo"):
        ctx.flow_analysis(u, u, u, 1.0, 1.0, 1.0, z_range=(0, 6), edges=(False, True))
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):  # below the wrapper's validation: PTV_E_ARG
        z = np.zeros(shape)
        with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
            ctx.flow_analysis(z, z, z, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="positive and finite"):
        ctx.flow_analysis(u, u, u, 1.0, 0.0, 1.0)


def test_an_empty_plane_range_gives_zero_statistics(ctx):
    f, m = _random_case((4, 3, 4), np.float64, 2)
    got, st = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m, z_range=(2, 2))
    assert all(got[k].shape == (0, 3, 4) for k in OUTPUTS)
    assert st["n_voxels"] == 0 and st["n_fluid"] == 0 and st["sum_u"] == 0.0
    assert all(v == 0.0 for k in ("sum", "sum_fluid", "max", "min") for v in st[k].values())


# ---------------------------------------------------------------- optional outputs
def test_every_subset_of_the_outputs_gives_the_same_bits(ctx):
    import torch

    shape = (BATCH + 1, 5, 130)
    n = int(np.prod(shape))
    f, m = _random_case(shape, np.float64, 21)
    dev = [torch.from_numpy(a).cuda() for a in f]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    sentinel = -12345.0

    def run(subset):
        outs = [torch.full((n,), sentinel, dtype=torch.float64, device="cuda") for _ in OUTPUTS]
        torch.cuda.synchronize()
        st = ctx.flow_analysis_dev(shape[2], shape[1], shape[0], [t.data_ptr() for t in dev],
                                   [o.data_ptr() if k in subset else 0 for k, o in zip(OUTPUTS, outs)], *H,
                                   viscosity=VISC, mask_ptr=dm.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {k: o.cpu().numpy() for k, o in zip(OUTPUTS, outs)}, st

    full, sf = run(OUTPUTS)
    want = fref.analyze(*f, *H, VISC, m)
    for k in OUTPUTS:
        assert np.array_equal(full[k].reshape(shape), want[k]), k
    subsets = [s for r in range(1, 5) for s in itertools.combinations(OUTPUTS, r)]
    assert len(subsets) == 15
    for subset in subsets:
        got, st = run(subset)
        for k in OUTPUTS:
            if k in subset:
                assert got[k].tobytes() == full[k].tobytes(), (subset, k)
                for stat in ("sum", "sum_fluid", "max", "min"):
                    assert st[stat][k] == sf[stat][k], (subset, k, stat)
            else:
                assert (got[k] == sentinel).all(), (subset, k)
                assert st["sum"][k] == 0.0 and st["max"][k] == 0.0 and st["min"][k] == 0.0
        assert (st["sum_u"], st["sum_v"], st["sum_w"], st["n_fluid"]) == \
            (sf["sum_u"], sf["sum_v"], sf["sum_w"], sf["n_fluid"])


# ---------------------------------------------------------------- elementwise mode
@pytest.mark.parametrize("dtype, shape", [(np.float64, (5, 7, 130)), (np.float64, (3, 5, 131)),
                                          (np.float32, (33, 9, 8)), (np.float32, (3, 5, 263))])
@pytest.mark.parametrize("masked", [True, False])
def test_elementwise_mode_equals_the_fused_call(ctx, dtype, shape, masked):
    f, m = _random_case(shape, dtype, 31 + sum(shape), masked)
    fused, _ = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m)
    # the reference chains masked S and O into the derived fields; so does the caller of this mode
    got, st = ctx.flow_derived(fused["strain_rate"], fused["vorticity"], viscosity=VISC, fluid_mask=m)
    for k in ("dissipation", "flow_type"):
        assert fref.same(got[k], fused[k]), k
    _check_stats(st, got, m)
    only_d, _ = ctx.flow_derived(fused["strain_rate"], None, viscosity=VISC, fluid_mask=m, outputs=("dissipation",))
    assert fref.same(only_d["dissipation"], fused["dissipation"]) and "flow_type" not in only_d


def test_elementwise_mode_device_pointers(ctx):
    import torch

    shape = (4, 6, 64)
    f, m = _random_case(shape, np.float64, 77)
    want = fref.analyze(*f, *H, VISC, m)
    s, o = (torch.from_numpy(want[k]).cuda() for k in ("strain_rate", "vorticity"))
    d, t = torch.empty_like(s), torch.empty_like(s)
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    st = ctx.flow_derived_dev(s.numel(), s.data_ptr(), o.data_ptr(), d.data_ptr(), t.data_ptr(), viscosity=VISC,
                              mask_ptr=dm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), want["dissipation"])
    assert np.array_equal(t.cpu().numpy(), want["flow_type"])
    assert st["n_fluid"] == int(m.sum())


# ---------------------------------------------------------------- statistics
def test_dyadic_inputs_sum_exactly(ctx):
    """Small integers times 2^-6: every partial sum is exact in any order, so the sums of u, v, w
    equal np.sum bit for bit (several blocks in x, y and z)."""
    shape = (PLANES + 3, 9, 130)
    rng = np.random.default_rng(41)
    for dtype in (np.float64, np.float32):
        f = [(rng.integers(-64, 65, size=shape) * 2.0**-6).astype(dtype) for _ in range(3)]
        m = rng.random(shape) < 0.6
        got, st = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m)
        for name, a in zip(("sum_u", "sum_v", "sum_w"), f):
            assert st[name] == float(np.sum(a, dtype=np.float64)) == math.fsum(a.ravel()), name
        _check_stats(st, got, m, f)


def test_extrema_propagate_nan_as_numpy_does(ctx):
    f, m = _random_case((4, 5, 6), np.float64, 51)
    f[0][2, 2, 2] = np.nan
    m[1:4, 1:4, 1:4] = True  # its stencil neighbours are fluid
    got, st = _quiet(ctx.flow_analysis, *f, *H, viscosity=VISC, fluid_mask=m)
    assert np.isnan(got["strain_rate"]).any()
    for k in ("strain_rate", "dissipation", "vorticity"):
        assert math.isnan(st["max"][k]) and math.isnan(st["min"][k]) and math.isnan(st["sum"][k]), k
    assert not np.isnan(got["flow_type"]).any()  # a NaN denominator gives 0
    _check_stats(st, got, m)


def test_permeability_is_the_references_expression_on_the_device_sums(ctx, va):
    shape = (PLANES + 1, 6, 20)
    for dtype in (np.float64, np.float32):
        f, m = _random_case(shape, dtype, 61)
        f[2] += dtype(0.5)  # a mean flow
        res = va.analyze(*f, *H, VISC, m)
        st, n = res["stats"], res["stats"]["n_voxels"]
        want = fref.permeability_from_means(*(np.float64(st[k]) / np.float64(n) for k in ("sum_u", "sum_v", "sum_w")),
                                            np.float64(st["sum"]["dissipation"]) / np.float64(n), VISC)
        assert res["permeability"] == want and isinstance(res["permeability"], np.float64)
        # the per-function wrapper: its own two passes' sums through the same expression
        _, s1 = ctx.flow_analysis(*f, 1.0, 1.0, 1.0, outputs=())
        _, s2 = ctx.flow_derived(res["dissipation"], None, outputs=())
        k = va.compute_permeability(*f, res["dissipation"], VISC, *H, mask=m)
        assert k == fref.permeability_from_means(*(np.float64(s1[q]) / np.float64(n) for q in ("sum_u", "sum_v", "sum_w")),
                                                 np.float64(s2["sum_u"]) / np.float64(n), VISC)
        assert (s1["sum_u"], s1["sum_v"], s1["sum_w"]) == (st["sum_u"], st["sum_v"], st["sum_w"])
        # and it is the reference's number to rounding (np.mean sums in another order, float32 in float32)
        ref = fref.compute_permeability(*f, res["dissipation"], VISC, *H, m)
        assert abs(k - ref) <= (1e-12 if dtype is np.float64 else 1e-4) * abs(ref)
        assert va.compute_permeability(*f, np.zeros(shape, dtype), VISC, *H) == 0.0


def test_two_calls_return_the_same_bits(ctx):
    f, m = _random_case((PLANES + 1, 9, 130), np.float64, 71)
    a, sa = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m)
    b, sb = ctx.flow_analysis(*f, *H, viscosity=VISC, fluid_mask=m)
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    sa.pop("ms_stencil"), sb.pop("ms_stencil")
    assert sa == sb
