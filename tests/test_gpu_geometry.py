"""GPU parity of every k-NN consumer off the unit grid and in flat clouds (tests/_geometry.py):
coordinates scaled by 2^-80 .. 2^80, offset by 1e6 and 2^40, anisotropic; planar, collinear,
nearly planar and fully coincident clouds; descending and uneven axes; a grid away from the
particles or inside a gap of them; n = k and n = 1; and five of these again on a grid large
enough for the coarse lattice (``@dense``).  Runs only on an MI355X (``-m gpu``).

These are the regimes of the bounding box, the cell grid's dimension count, the margins
(``cg.mg``, ``sqrtf_up``, the fp32 prefilters, the packed keys' truncation) and the tile boxes
(DESIGN.md "Supported coordinate envelope").  Every comparison is against ``oracle.cpu_ref`` on
the same arrays, with the bar the suite already uses for the method: IDW p = 2 and nearest bit for
bit outside value-heterogeneous ties (tests/test_geometry_cases.py holds their share at 0),
Sibson normwise 1e-10, radius IDW NaN pattern + 1e-12, local RBF against the extended-precision
solve, linear bit for bit.  The metamorphic checks need no oracle: a power-of-two scaling and a
reversed axis change no voxel's value.
"""
import numpy as np
import pytest

from oracle import cpu_ref
from tests import _geometry as G
from tests._util import normwise

pytestmark = pytest.mark.gpu

TOL_SIBSON = 1e-10  # tests/test_gpu_keys.py
TOL_RADIUS = 1e-12  # tests/test_gpu_radius.py
TOL_RBF = 1e-10     # tests/test_gpu_rbf.py: gpu-vs-exact <= max(TOL, lapack-vs-exact)
TOL_LINEAR = 1e-12  # tests/test_gpu_linear.py, voxels on simplex faces


@pytest.fixture(scope="module")
def ctx():
    from ptv_interpolation_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    return _lib.Context.get(0)


def _method(k):
    from ptv_interpolation_amd import _lib

    return {"nearest": _lib.METHOD_NEAREST, "sibson": _lib.METHOD_SIBSON, "idw": _lib.METHOD_IDW}[G.method_of(k)]


def _knn(ctx, name, k, **kw):
    (P, Q, ax, ay, az), k = G.get(name, k)
    return ctx.interp_knn(P, Q, axes=(ax, ay, az), method=_method(k), k=k, **kw)


# ---------------------------------------------------------------------------------------------
# k-NN interpolation against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", G.runs())
def test_knn_vs_oracle(ctx, name, k):
    """k = 8 (fill-then-sort) and 20 (packed keys) on every case; nearest, k = 7 (insert path), 12,
    50, 130 (large-k path) and Sibson k = 30 on the wide cases; k = 8 and 20 on the lattice-sized
    grid, where the coarse lattice's count bounds and ``lattice_ub`` run (ms_lattice > 0)."""
    got = _knn(ctx, name, k)
    print(f"{name} k={k} {G.method_of(k)}: n_repair_tiles {ctx.stats['n_repair_tiles']}, "
          f"cells {ctx.stats['cells']}, r0 {ctx.stats['r0']:.3e}")
    ref = G.oracle_knn(name, k)
    keep = ~G.hetero(name, k)
    assert keep.mean() >= 1.0 - G.TIE_CAP.get(name.split("@")[0], 0.0)
    for a, b in zip(got, ref):
        if k == G.K_SIBSON:
            assert normwise(a, b) <= TOL_SIBSON
        else:
            assert np.array_equal(a[keep], b[keep]), f"{np.sum(a[keep] != b[keep])} of {keep.sum()} voxels differ"


# ---------------------------------------------------------------------------------------------
# metamorphic checks (no oracle)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", G.SCALE_EXPONENTS)
def test_nearest_is_scale_invariant(ctx, e):
    """The nearest particle of a voxel is the same under an exact scaling, and the output is its
    value: bit-identical to the base case."""
    base = _knn(ctx, "base", 1)
    scaled = _knn(ctx, f"scale_2^{e}", 1)
    for a, b in zip(base, scaled):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("grid", ["", "@dense"])
@pytest.mark.parametrize("k", G.K_ALL)
def test_descending_axes_do_not_change_a_voxel(ctx, k, grid):
    """axes_irregular with its x and z axes sorted ascending, flipped back along x and z, equals the
    run on the descending axes bit for bit; on the lattice-sized grid the lattice's every-4th-point
    axes are then subsampled from a descending, uneven axis."""
    P, Q, ax, ay, az = G.case("axes_irregular" + grid)
    assert ax[0] > ax[-1] and az[0] > az[-1]
    desc = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k)
    asc = ctx.interp_knn(P, Q, axes=(ax[::-1].copy(), ay, az[::-1].copy()), k=k)
    for a, b in zip(desc, asc):
        assert np.array_equal(a, b[::-1, :, ::-1])


# ---------------------------------------------------------------------------------------------
# call modes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.MODE_CASES)
@pytest.mark.parametrize("k", G.K_ALL)
def test_modes_equal_the_separable_grid(ctx, name, k):
    """Point-list grid, a z-slab and the slab under PTV_FLAG_SLAB_CULL_AUTO all equal the whole
    separable grid bit for bit.  (This grid builds no lattice, so the flag falls through to the
    plain slab call here; test_slab_cull_map_on_the_lattice_grid runs the map.)"""
    from ptv_interpolation_amd import _lib

    P, Q, ax, ay, az = G.case(name)
    whole = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k)
    Z, Y, X = np.meshgrid(az, ay, ax, indexing="ij")
    pl = ctx.interp_knn(P, Q, grid_points=(X, Y, Z), shape=X.shape, k=k)
    slab = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k, z_range=(3, 7))
    cull = [ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k, z_range=(3, 7), flags=_lib.FLAG_SLAB_CULL_AUTO)
            for _ in range(2)]
    for c in range(3):
        assert np.array_equal(whole[c], pl[c])
        assert np.array_equal(whole[c][3:7], slab[c])
        assert np.array_equal(whole[c][3:7], cull[0][c]) and np.array_equal(whole[c][3:7], cull[1][c])


@pytest.mark.parametrize("name", G.DENSE_CULL_CASES)
@pytest.mark.parametrize("k", G.K_ALL)
def test_slab_cull_map_on_the_lattice_grid(ctx, name, k):
    """PTV_FLAG_SLAB_CULL_AUTO on a slab that builds the lattice, three calls: the first bins every
    particle and caches the per-column map, the second culls with it and proves the cull on the device,
    the third runs speculatively from the cached count and box.  Each equals the oracle's rows bit for
    bit.  The second and third calls must have run the proven cull (halo_required is 0 there and -1
    when every particle was binned without a map), and on G.DENSE_MUST_CULL must have dropped particles."""
    from ptv_interpolation_amd import _lib

    P, Q, ax, ay, az = G.case(name + "@dense")
    z0, z1 = G.DENSE_SLAB
    ref = G.oracle_knn(name + "@dense", k)
    keep = ~G.hetero(name + "@dense", k)[z0:z1]
    binned, proven = [], []
    for call in range(3):
        got = ctx.interp_knn(P, Q, axes=(ax, ay, az), k=k, z_range=(z0, z1), flags=_lib.FLAG_SLAB_CULL_AUTO)
        binned.append(ctx.stats["n_binned"])
        proven.append(ctx.stats["halo_required"])
        for a, b in zip(got, ref):
            assert np.array_equal(a[keep], b[z0:z1][keep]), f"call {call}: {np.sum(a[keep] != b[z0:z1][keep])} differ"
    print(f"{name}@dense k={k} slab {z0}:{z1}: particles binned per call {binned} of {len(P)}")
    assert binned[0] == len(P) and proven[0] == -1.0
    assert proven[1:] == [0.0, 0.0] and k <= binned[1] <= len(P) and binned[2] == binned[1]
    if name in G.DENSE_MUST_CULL:
        assert binned[1] < len(P)


# ---------------------------------------------------------------------------------------------
# fixed-radius IDW
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.RADIUS_CASES)
def test_radius_idw_vs_oracle(ctx, name):
    """r = 1.5 base units, scaled with the case.  Bar of tests/test_gpu_radius.py: NaN pattern equal,
    normwise <= 1e-12, voxels with a particle within 1e-9 (base units) of the ball surface excluded."""
    from ptv_interpolation_amd import _lib
    from scipy.spatial import KDTree

    P, Q, ax, ay, az = G.case(name)
    s = G.scale_of(name)
    r = G.RADIUS * s
    U, V, W = ctx.interp_knn(P, Q, axes=(ax, ay, az), method=_lib.METHOD_IDW_RADIUS, radius=r)
    q = G.queries(name)
    ref = cpu_ref.idw_radius_points(P, Q, q, r)
    t = KDTree(P)
    skip = (t.query_ball_point(q, r + 1e-9 * s, return_length=True) !=
            t.query_ball_point(q, r - 1e-9 * s, return_length=True))
    print(f"{name}: empty balls {np.isnan(ref[:, 0]).mean():.1%}, surface voxels excluded {skip.mean():.2%}")
    assert skip.mean() < 0.01
    if name == "grid_far":
        assert np.isnan(ref).all()
    for c, got in enumerate((U, V, W)):
        a, b = got.reshape(-1)[~skip], ref[:, c][~skip]
        assert np.array_equal(np.isnan(a), np.isnan(b)), "empty-ball (NaN) pattern differs"
        assert normwise(a, b) <= TOL_RADIUS


# ---------------------------------------------------------------------------------------------
# outlier filter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.FILTER_CASES)
@pytest.mark.parametrize("k", G.FILTER_K)
def test_filter_vs_oracle(ctx, name, k):
    """keep and the (k+1)-th neighbour distance equal the oracle's for every particle
    (tests/test_geometry_cases.py: no particle of these cases is tie-order dependent)."""
    from scipy.spatial import KDTree

    P, Q, *_ = G.case(name)
    keep, kth = ctx.filter_outliers_knn(P, Q, k=k, threshold=3.0)
    ref_keep, ref_radius = cpu_ref.outlier_filter(P, Q, k, 3.0)
    d, _ = KDTree(P).query(P, k=k + 1)
    assert np.array_equal(keep.view(bool), ref_keep), f"{np.sum(keep.view(bool) != ref_keep)} decisions differ"
    assert np.array_equal(kth, d[:, -1])
    assert np.median(kth) == ref_radius


# ---------------------------------------------------------------------------------------------
# local RBF
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.RBF_CASES)
@pytest.mark.parametrize("kernel,k,eps,degree", [("thin_plate_spline", 20, None, None), ("gaussian", 32, 1.5, -1)])
def test_rbf_vs_extended_precision(ctx, name, kernel, k, eps, degree):
    """TPS k = 20 and Gaussian epsilon = 1.5 / scale, degree -1, k = 32.  Bar per component:
    gpu-vs-exact <= max(1e-10, lapack-vs-exact), exact = the extended-precision solve of the same
    systems."""
    from ptv_interpolation_amd.rbf import LocalRBFInterpolator

    P, Q, ax, ay, az = G.case(name)
    if eps is not None:
        eps = eps / G.scale_of(name)
    U, V, W = LocalRBFInterpolator(P, Q, neighbors=k, kernel=kernel, epsilon=eps, degree=degree).evaluate_grid(
        ax, ay, az, ctx=ctx)
    q = G.queries(name)
    lap = cpu_ref.rbf_local_points(P, Q, q, k, kernel, eps, degree)
    ext = cpu_ref.rbf_local_points(P, Q, q, k, kernel, eps, degree, solver="extended")
    for c, a in enumerate((U, V, W)):
        e_ref = normwise(a.ravel(), lap[:, c])
        e_exact = normwise(a.ravel(), ext[:, c])
        gap = normwise(lap[:, c], ext[:, c])
        print(f"{name} {kernel} k={k} {'UVW'[c]}: gpu-vs-lapack {e_ref:.3e}  gpu-vs-exact {e_exact:.3e}  "
              f"lapack-vs-exact {gap:.3e}")
        assert e_exact <= max(TOL_RBF, gap)


def test_rbf_planar_is_singular_everywhere(ctx):
    """A planar cloud leaves the TPS polynomial block rank deficient at every voxel: LinAlgError as
    scipy, and the count of singular systems is the voxel count."""
    from ptv_interpolation_amd.rbf import LocalRBFInterpolator

    P, Q, ax, ay, az = G.case("planar")
    with pytest.raises(np.linalg.LinAlgError):
        cpu_ref.rbf_local_points(P, Q, G.queries("planar")[:8], 20)
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        LocalRBFInterpolator(P, Q, neighbors=20).evaluate_grid(ax, ay, az, ctx=ctx)
    st = ctx.last_stats()
    print("planar TPS k=20: n_singular", st["n_singular"], "n_rbf_pivoted", st["n_rbf_pivoted"])
    assert st["n_singular"] == len(ax) * len(ay) * len(az)


# ---------------------------------------------------------------------------------------------
# linear (Delaunay)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.LINEAR_CASES)
def test_linear_vs_oracle(ctx, name):
    """One Delaunay object for the GPU and the oracle; bit for bit, grid_far all fill_value."""
    from ptv_interpolation_amd import _lib
    from scipy.spatial import Delaunay

    P, Q, ax, ay, az = G.case(name)
    d = Delaunay(P)
    got = ctx.interp_linear(P, Q, _lib.Triangulation(d), axes=(ax, ay, az), fill_value=-7.5)
    ref = cpu_ref.linear_points(P, Q, G.queries(name), fill_value=-7.5, tri=d)
    print(f"{name}: outside the hull {np.mean(ref[:, 0] == -7.5):.1%}, brute-force voxels {ctx.stats['n_singular']}")
    for c, a in enumerate(got):
        assert np.array_equal(a.ravel(), ref[:, c]), f"{np.sum(a.ravel() != ref[:, c])} voxels differ"
        if name == "grid_far":
            assert (a == -7.5).all()


def test_linear_voxels_on_vertices_and_bounds(ctx):
    """A grid whose axes are the coordinates of 5 particles plus tri.min_bound / tri.max_bound: voxels
    exactly on vertices (where every incident simplex is a valid answer) and exactly on the bounding
    box test of the point location.  Normwise <= 1e-12 (any incident simplex interpolates the vertex
    to rounding); the share of differing voxels is printed.  Every voxel carries the bits of a simplex
    that scipy's rule accepts (tests/_linear_ref.py)."""
    from ptv_interpolation_amd import _lib
    from scipy.spatial import Delaunay
    from tests import _linear_ref as R

    P, Q, *_ = G.case("base")
    d = Delaunay(P)
    pick = np.argsort(np.linalg.norm(P - P.mean(axis=0), axis=1))[[0, 300, 900, 1800, 2700]]
    axes = [np.sort(np.concatenate([[d.min_bound[c]], P[pick, c], [d.max_bound[c]]])) for c in range(3)]
    got = ctx.interp_linear(P, Q, _lib.Triangulation(d), axes=tuple(axes), fill_value=-7.5)
    q = cpu_ref.grid_queries(*axes)
    ref = cpu_ref.linear_points(P, Q, q, fill_value=-7.5, tri=d)
    hit = (q[:, None, :] == P[pick][None, :, :]).all(axis=2)  # (voxel, picked particle)
    assert (hit.sum(axis=0) == 1).all()
    on_vertex = hit.argmax(axis=0)  # the voxel that sits on each picked particle
    for c, a in enumerate(got):
        print(f"{'UVW'[c]}: differing voxels {np.mean(a.ravel() != ref[:, c]):.2%} of {len(q)}, "
              f"normwise {normwise(a.ravel(), ref[:, c]):.2e}")
        assert normwise(a.ravel(), ref[:, c]) <= TOL_LINEAR
        assert normwise(a.ravel()[on_vertex], Q[pick, c]) <= TOL_LINEAR  # a vertex takes its own value
    assert len(R.unexplained(got, R.admissible(d, Q, q, -7.5, R.EPS_BROAD))) == 0


# ---------------------------------------------------------------------------------------------
# non-finite coordinates: ValueError, as the oracle (cKDTree) raises
# ---------------------------------------------------------------------------------------------
def _calls(ctx, P, Q, axes=None, grid_points=None, shape=None, tri=None):
    grid = dict(axes=axes) if axes is not None else dict(grid_points=grid_points, shape=shape)
    calls = {
        "interp_knn": lambda: ctx.interp_knn(P, Q, k=8, **grid),
        "interp_knn_k20": lambda: ctx.interp_knn(P, Q, k=20, **grid),
        "interp_rbf": lambda: ctx.interp_rbf(P, Q, k=20, **grid),
        "interp_linear": lambda: ctx.interp_linear(P, Q, tri, **grid),
    }
    return calls


def _all_raise(calls, what, exc=ValueError, match="non-finite"):
    for name, call in calls.items():
        try:
            call()
        except Exception as e:
            assert isinstance(e, exc) and match in str(e), f"{name} on {what}: {type(e).__name__}: {e}"
        else:
            raise AssertionError(f"{name} accepted {what}")


@pytest.fixture(scope="module")
def base_tri():
    from ptv_interpolation_amd import _lib
    from scipy.spatial import Delaunay

    return _lib.Triangulation(Delaunay(G.case("base")[0]))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", ["particle", "axis", "query"])
def test_non_finite_coordinates_raise(ctx, base_tri, bad, where):
    """One non-finite value in a particle coordinate (the last particle's z: no reduction order
    hides it), in an axis, or in a point-list query: ValueError from every entry point, never a
    number.  (The triangulation is the clean cloud's: scipy's Delaunay refuses the value itself.)"""
    P, Q, ax, ay, az = (a.copy() for a in G.case("base"))
    Z, Y, X = (a.copy() for a in np.meshgrid(az, ay, ax, indexing="ij"))
    if where == "particle":
        P[-1, 2] = bad
        calls = _calls(ctx, P, Q, axes=(ax, ay, az), tri=base_tri)
        calls["filter_outliers_knn"] = lambda: ctx.filter_outliers_knn(P, Q, k=10)
    elif where == "axis":
        ay[4] = bad
        calls = _calls(ctx, P, Q, axes=(ax, ay, az), tri=base_tri)
    else:
        X[5, 3, 7] = bad
        calls = _calls(ctx, P, Q, grid_points=(X, Y, Z), shape=X.shape, tri=base_tri)
    _all_raise(calls, f"a {bad} {where} coordinate")
    # the context still serves a clean call afterwards
    P, Q, ax, ay, az = G.case("base")
    for a, b in zip(ctx.interp_knn(P, Q, axes=(ax, ay, az), k=8), G.oracle_knn("base", 8)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_particle_through_the_slab_culls(ctx, bad):
    """The slab culls bin only the particles near the slab, and reduce the bounding box over those:
    a particle with a non-finite coordinate is kept by every cull, so the call raises as it does
    without one.  slab_halo > 0 first; then PTV_FLAG_SLAB_CULL_AUTO on its cached-map and speculative
    calls, with the value put in after the map was built."""
    from ptv_interpolation_amd import _lib

    P, Q, ax, ay, az = G.case("offset_1e6@dense")
    z0, z1 = G.DENSE_SLAB
    zlo, zhi = min(az[z0], az[z1 - 1]), max(az[z0], az[z1 - 1])
    # 200 more particles 20 to 30 units above the slab: no halo the proof asks for reaches them
    rng = np.random.default_rng(5)
    F = P[:200].copy()
    F[:, 2] = zhi + rng.uniform(20.0, 30.0, 200)
    far = len(P)
    P, Q = np.concatenate([P, F]), np.concatenate([Q, Q[:200]])
    inside = int(np.argmin(np.abs(P[:, 2] - 0.5 * (zlo + zhi))))
    halo = 8.0
    ctx.interp_knn(P, Q, axes=(ax, ay, az), k=8, z_range=(z0, z1), slab_halo=halo)
    print(f"slab_halo {halo}: halo_required {ctx.stats['halo_required']:.3f}, binned {ctx.stats['n_binned']} of {len(P)}")
    assert ctx.stats["n_binned"] <= len(P) - 200 and P[far, 2] > zhi + halo  # the cull is active and drops `far`
    variants = {}
    for label, row, col in (("z of a culled particle", far, 2), ("x of a culled particle", far, 0),
                            ("y of a kept particle", inside, 1)):
        B = P.copy()
        B[row, col] = bad
        variants[label] = B
    _all_raise({f"slab_halo, {bad} in {label}": (lambda B=B: ctx.interp_knn(
        B, Q, axes=(ax, ay, az), k=8, z_range=(z0, z1), slab_halo=halo)) for label, B in variants.items()}, "the slab")
    auto = dict(axes=(ax, ay, az), k=8, z_range=(z0, z1), flags=_lib.FLAG_SLAB_CULL_AUTO)
    for label, B in variants.items():
        for clean_calls in (1, 2):  # then the bad call is the cached-map call / the speculative call
            for _ in range(clean_calls):
                ctx.interp_knn(P, Q, **auto)
            assert clean_calls == 1 or ctx.stats["n_binned"] < len(P)
            _all_raise({f"cull map after {clean_calls} clean call(s), {bad} in {label}":
                        lambda B=B: ctx.interp_knn(B, Q, **auto)}, "the slab")


@pytest.mark.parametrize("e", [-600, 600])
def test_coordinates_outside_the_float64_range_are_refused(ctx, e):
    """Squared distances of coordinates scaled by 2^600 overflow float64, those of 2^-600 are
    subnormal or 0: PTV_E_UNSUPPORTED (NotImplementedError), never a number."""
    P, Q, ax, ay, az = G.case("base")
    s = 2.0 ** e
    calls = {
        "interp_knn": lambda: ctx.interp_knn(P * s, Q, axes=(ax * s, ay * s, az * s), k=8),
        "interp_knn_k20": lambda: ctx.interp_knn(P * s, Q, axes=(ax * s, ay * s, az * s), k=20),
        "interp_rbf": lambda: ctx.interp_rbf(P * s, Q, axes=(ax * s, ay * s, az * s), k=20),
        "filter_outliers_knn": lambda: ctx.filter_outliers_knn(P * s, Q, k=10),
    }
    _all_raise(calls, f"coordinates scaled by 2^{e}", exc=NotImplementedError, match="supported range")
