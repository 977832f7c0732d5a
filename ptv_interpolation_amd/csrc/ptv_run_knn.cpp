// ptv_run_knn.cpp — the k-NN interpolation call on device pointers (run_knn: the register-list
// kernels with the optional slab cull, the cached cull map of PTV_FLAG_SLAB_CULL_AUTO, the large-k
// path) and the outlier filter's particle queries (run_filter).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptv_ctx.hpp"

namespace ptv {

namespace {

// the outlier filter's particle queries (5M, k = 25): 23.3 ms at 1.2, 22.6 at 2.5, 22.4 at 5,
// 24.1 at 8 / 4, 28.4 at 16 / 12
constexpr double kFilterOccupancy = 5.0;
// the filter's first gather radius, in units of the expected (k+1)-NN radius: its queries sit on
// the particles (the pack's sphere shells), so the mean-density radius overshoots.  Same-box sweep
// (5M particles, k = 25, search ms): 1.0 19.79, 0.75 19.51, 0.6 19.45, 0.45 19.42, 0.3 23.25
constexpr double kFilterR0Scale = 0.6;
// relative widening of the cached slab cull map over the need it was built from
constexpr double kCullMapSlack = 1e-6;

SearchParams knn_search(const ptv_knn_params *prm) {
    return SearchParams{prm->method, prm->k, prm->power, prm->eps, prm->flags, prm->cell_occupancy, prm->r0_scale,
                        prm->lattice_bounds};
}

// The main launch of a call, with what every path does after it.
int launch_main(ptv_ctx *c, const KnnLaunch &kl, const Prepared &pr, const ptv_grid *g, const uint8_t *mask, double *U,
                double *V, double *W, hipStream_t s) {
    PTV_TRY(launch_knn(kl, pr.b, queries_of(g), mask, U, V, W, s));
    PTV_TRY(c->ev_knn1.record(s));
    c->timed_pending = true;
    return PTV_OK;
}

// ---- PTV_FLAG_SLAB_CULL_AUTO (see ptv_api.h): the per-column cull map, cached per context ----
// A call whose key matches the cached map culls with it and proves the cull on the device (the need
// map of the kept particles' lattice inside the used map everywhere) before the gated main launch; a
// call without a cached map (or whose proof fails) bins every particle and builds the map from its
// own lattice.  Key: the particle arrays, n, a 96-value fingerprint, the axis values, the grid, the
// slab, k, method.

// This call's key: the data part gathered into c->cfp on the device (ndev doubles), the host part,
// and, once read(), the whole key as the cache stores it.
struct CullKey {
    size_t ndev = 0;
    std::vector<double> host, full;

    // the fingerprint, then the grid's axis values: the map and the cached lattice bounds belong to
    // lattice positions, and a reused axis buffer (the host path's c->axes, a recycled torch
    // allocation) can hold other coordinates under the same pointer.  Gathered on the device and
    // read back in one copy (one copy per array cost ~20 us each)
    int build(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, hipStream_t s) {
        const double *src[6] = {p->x, p->y, p->z, p->u, p->v, p->w};
        const size_t nfp = 6 * kFingerprint;
        ndev = nfp + (size_t)(g->nx + g->ny + g->nz);
        PTV_TRY(c->cfp.ensure(ndev));
        PTV_TRY(launch_fingerprint(src, p->n, c->cfp.p, s));
        PTV_TRY(launch_concat3(g->ax, (int)g->nx, g->ay, (int)g->ny, g->az, (int)g->nz, c->cfp.p + nfp, s));
        // the host part of the key: the arrays, n, the grid, the slab, k, method
        for (const void *q : {(const void *)p->x, (const void *)p->y, (const void *)p->z, (const void *)p->u,
                              (const void *)p->v, (const void *)p->w, (const void *)g->ax, (const void *)g->ay,
                              (const void *)g->az}) {
            uint64_t bits = (uint64_t)(uintptr_t)q;
            double d;
            std::memcpy(&d, &bits, sizeof(d));
            host.push_back(d);
        }
        for (int64_t v : {p->n, g->nx, g->ny, g->nz, g->z_begin, g->z_end, (int64_t)prm->k, (int64_t)prm->method,
                          (int64_t)prm->lattice_bounds})
            host.push_back((double)v);
        return PTV_OK;
    }
    int read(ptv_ctx *c, hipStream_t s) {
        full.assign(ndev, 0.0);
        PTV_HIP(hipMemcpyAsync(full.data(), c->cfp.p, ndev * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipStreamSynchronize(s));
        full.insert(full.end(), host.begin(), host.end());
        return PTV_OK;
    }
    // bitwise comparisons (a NaN fingerprint value never matches itself otherwise)
    static bool same(const std::vector<double> &a, const std::vector<double> &b) {
        return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
    }
    bool host_matches(const CullCache &cc) const { return same(cc.key_host, host) && cc.key.size() == ndev + host.size(); }
    bool matches(const CullCache &cc) const { return same(cc.key, full); }
    // the map built by this call is keyed by its data; no culled call has run under it yet
    int store(ptv_ctx *c, hipStream_t s) const {
        CullCache &cc = c->ccache;
        cc.key = full;
        cc.key_host = host;
        PTV_TRY(cc.key_dev.ensure(ndev));
        PTV_HIP(hipMemcpyAsync(cc.key_dev.p, c->cfp.p, ndev * sizeof(double), hipMemcpyDeviceToDevice, s));
        cc.kept_valid = false;
        return PTV_OK;
    }
};

// The culled attempt: cull with the cached map, bin the kept particles, prove on the device that
// their lattice bounds stay within the cached ones, and run the main launch gated by that proof.
// spec: a proven culled call already ran with this host key, so the device also compares the data
// part (fingerprint + axis values) and the kept count, folded into the same gate; the host reads the
// gate once, after the main launch (no synchronisation before it).
// proven = false: no outputs were written.
int knn_auto_culled(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm,
                    const CullKey &key, bool spec, const uint8_t *mask, double *U, double *V, double *W,
                    hipStream_t s, bool &proven) {
    proven = false;
    const SearchParams sp = knn_search(prm);
    CullMap used = c->cmap_geo;
    used.top = c->cmap[0].p;
    used.bot = c->cmap[1].p;
    Culled cu;
    PTV_TRY(cull_slab(c, p, g, prm->k, 0.0, &used, spec ? &c->ccache : nullptr, key.ndev, s, cu));
    if (!cu.ok) return PTV_OK;
    KnnLaunch kl;
    Prepared pr;
    PTV_TRY(prepare(c, &cu.p, g, &sp, s, kl, pr, cu.box, true));
    if (kl.cb.dk == nullptr) return PTV_OK;  // no lattice bounds: nothing to prove the cull with
    PTV_TRY(c->halo_need.ensure(1));
    const long long nlp = (long long)kl.cb.n[0] * kl.cb.n[1] * kl.cb.n[2];
    kl.gate = c->halo_need.p;
    kl.gate_halo = 0.0;
    if (!(kl.cb.n[0] == c->cdk_n[0] && kl.cb.n[1] == c->cdk_n[1] && kl.cb.n[2] == c->cdk_n[2])) {
        // (cannot happen for one key: the lattice follows the grid and the slab) a different
        // lattice proves nothing against the cached bounds: a failing gate, rerun by the caller
        PTV_HIP(hipMemsetAsync(c->halo_need.p, 0xff, sizeof(unsigned long long), s));
    } else {
        // the proof, gating the main launch: the need map grows with the lattice bounds, and the
        // cached map was built from the bounds of the call that binned every particle (widened by
        // kCullMapSlack), so bounds of the kept particles within half that of the cached ones
        // prove that the map holds every particle a slab voxel can need
        PTV_TRY(launch_bounds_within(kl.cb.dk, c->cdk.p, nlp, 1.0 + 0.5 * kCullMapSlack, c->halo_need.p, s, !spec));
        PTV_TRY(c->ev_main0.record(s));
    }
    PTV_TRY(launch_main(c, kl, pr, g, mask, U, V, W, s));
    c->last.n_particles = p->n;
    c->last.n_binned = cu.p.n;
    PTV_HIP(hipMemcpyAsync(c->h_misc.p + 1, c->halo_need.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (dev_knob("PTV_DBG_CULL"))  // dev builds: the cull and its proof
        std::fprintf(stderr, "[cull] slab [%lld, %lld) kept %lld of %lld, map %dx%d, proof %llx\n",
                     (long long)g->z_begin, (long long)g->z_end, (long long)cu.p.n, (long long)p->n, used.mx, used.my,
                     (unsigned long long)c->h_misc.p[1]);
    if (c->h_misc.p[1] != 0ull) return PTV_OK;
    proven = true;  // the gated launch wrote every output
    c->last.halo_required = 0.0;
    if (!spec) {  // later calls with this key may run speculatively
        c->ccache.kept = cu.p.n;
        std::memcpy(c->ccache.bbox, cu.box, sizeof(cu.box));
        c->ccache.kept_valid = true;
    }
    return PTV_OK;
}

// Every particle binned; this call's lattice gives the map later calls cull with, keyed by `key`.
int knn_auto_uncached(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm,
                      const CullKey &key, const uint8_t *mask, double *U, double *V, double *W, hipStream_t s) {
    const SearchParams sp = knn_search(prm);
    KnnLaunch kl;
    Prepared pr;
    c->cull_timed = false;
    PTV_TRY(prepare(c, p, g, &sp, s, kl, pr, nullptr, true));
    if (kl.cb.dk == nullptr)  // no lattice bounds: nothing to build a map from
        return launch_main(c, kl, pr, g, mask, U, V, W, s);
    // the map geometry: cells of two finest-lattice cells per axis over the grid's (x, y) extent
    // (edge cells reach to infinity, so any extent is valid; it only sets the resolution)
    double e[4];
    PTV_HIP(hipMemcpyAsync(&e[0], g->ax, sizeof(double), hipMemcpyDefault, s));
    PTV_HIP(hipMemcpyAsync(&e[1], g->ax + (g->nx - 1), sizeof(double), hipMemcpyDefault, s));
    PTV_HIP(hipMemcpyAsync(&e[2], g->ay, sizeof(double), hipMemcpyDefault, s));
    PTV_HIP(hipMemcpyAsync(&e[3], g->ay + (g->ny - 1), sizeof(double), hipMemcpyDefault, s));
    PTV_HIP(hipStreamSynchronize(s));
    CullMap geo{};
    geo.mx = std::max(1, std::min(256, (kl.cb.n[0] - 1) / 2));
    geo.my = std::max(1, std::min(256, (kl.cb.n[1] - 1) / 2));
    geo.x0 = std::min(e[0], e[1]);
    geo.y0 = std::min(e[2], e[3]);
    const double wx = std::fabs(e[1] - e[0]), wy = std::fabs(e[3] - e[2]);
    geo.cw = wx > 0.0 && std::isfinite(wx) ? wx / geo.mx : 1.0;
    geo.ch = wy > 0.0 && std::isfinite(wy) ? wy / geo.my : 1.0;
    if (!std::isfinite(geo.x0)) geo.x0 = 0.0;
    if (!std::isfinite(geo.y0)) geo.y0 = 0.0;
    geo.icw = 1.0 / geo.cw;
    geo.ich = 1.0 / geo.ch;
    const size_t nm = (size_t)geo.mx * geo.my;
    const size_t ncol = (size_t)std::max(kl.cb.n[0] - 1, 1) * std::max(kl.cb.n[1] - 1, 1);
    const long long nlp = (long long)kl.cb.n[0] * kl.cb.n[1] * kl.cb.n[2];
    PTV_TRY(c->ccols.ensure(7 * ncol));
    PTV_TRY(c->ckeys.ensure(2 * nm));
    PTV_TRY(launch_main(c, kl, pr, g, mask, U, V, W, s));
    c->last.n_particles = p->n;
    c->last.n_binned = p->n;
    for (auto &d : c->cmap) PTV_TRY(d.ensure(nm));
    // (widened by kCullMapSlack: the packed-key lattice bounds of a culled call carry other slots in
    // their low bits, a few 1e-9 relative from this call's)
    PTV_TRY(launch_cull_need(kl.cb.ax, kl.cb.ay, kl.cb.az, kl.cb.n, kl.cb.dk, kl.cg.mg, kCullMapSlack, geo,
                             c->cmap[0].p, c->cmap[1].p, c->ccols.p, c->ckeys.p, nullptr, nullptr, s));
    PTV_TRY(c->cdk.ensure((size_t)nlp));
    PTV_HIP(hipMemcpyAsync(c->cdk.p, kl.cb.dk, (size_t)nlp * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int d = 0; d < 3; ++d) c->cdk_n[d] = kl.cb.n[d];
    c->cmap_geo = geo;
    c->cmap_valid = true;
    return key.store(c, s);
}

// Try culled with the cached map; if there is none for this key, or the cull is not proven (the
// particles changed under the same arrays and fingerprint, or under a speculative reuse the data key
// or kept count differed), run with every particle binned, which refreshes the map.
int run_knn_auto(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm,
                 const uint8_t *mask, double *U, double *V, double *W, hipStream_t s, ptv_stats *st) {
    CullKey key;
    PTV_TRY(key.build(c, p, g, prm, s));
    const bool spec = c->cmap_valid && c->ccache.kept_valid && key.host_matches(c->ccache);
    if (!spec) PTV_TRY(key.read(c, s));
    const bool use_map = spec || (c->cmap_valid && key.matches(c->ccache));
    if (dev_knob("PTV_DBG_CULL"))
        std::fprintf(stderr, "[cull] slab [%lld, %lld) n %lld: cached map %d, key match %d, speculative %d\n",
                     (long long)g->z_begin, (long long)g->z_end, (long long)p->n, (int)c->cmap_valid, (int)use_map,
                     (int)spec);
    int rc = PTV_OK;
    bool proven = false;
    if (use_map) {
        rc = knn_auto_culled(c, p, g, prm, key, spec, mask, U, V, W, s, proven);
        if (rc == PTV_OK && !proven) {
            c->cmap_valid = false;
            c->ccache.kept_valid = false;
            if (spec) rc = key.read(c, s);  // the map built next is keyed by this call's data
        }
    }
    if (rc == PTV_OK && !proven) rc = knn_auto_uncached(c, p, g, prm, key, mask, U, V, W, s);
    if (rc == PTV_OK && st) *st = c->last;
    return rc;
}

// k >= 128 (beyond the register lists): bin every particle (no lattice), then the large-k path --
// per-query ball bound, candidate gather, segmented sort, the reference's epilogue (ptv_knn_big.hip)
int run_knn_big(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, const uint8_t *mask,
                double *U, double *V, double *W, hipStream_t s, ptv_stats *st) {
    SearchParams sp = knn_search(prm);
    sp.lattice_bounds = -1;
    if (!(sp.cell_occupancy > 0.0)) sp.cell_occupancy = std::max(1.0, prm->k / 256.0);
    KnnLaunch kl;
    Prepared pr;
    c->cull_timed = false;
    c->rbf_chunks = 0;
    PTV_TRY(prepare(c, p, g, &sp, s, kl, pr));
    BigEpilogue ep;
    ep.method = prm->method;
    ep.power = prm->power;
    ep.eps = prm->eps;
    ep.flags = prm->flags;
    ep.U = U;
    ep.V = V;
    ep.W = W;
    const int64_t nvox = (g->z_end - g->z_begin) * g->nx * g->ny;
    PTV_TRY(run_big_knn(c->big, big_queries(g, (int)g->z_begin, mask), pr.b, pr.cg, nvox, prm->k, ep, s));
    PTV_TRY(c->ev_knn1.record(s));
    c->timed_pending = true;
    c->last.n_particles = p->n;
    c->last.n_binned = p->n;
    if (st) *st = c->last;
    return PTV_OK;
}

}  // namespace

int run_knn(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, const uint8_t *mask,
            double *U, double *V, double *W, hipStream_t s, ptv_stats *st) {
    const bool radius = prm->method == PTV_METHOD_IDW_RADIUS;
    if (!radius && kmax_for(prm->k) == 0) return run_knn_big(c, p, g, prm, mask, U, V, W, s, st);
    // the slab culls need the lattice bounds (they prove the cull exact)
    const bool can_cull = !radius && queries_of(g).separable() && lattice_built(g, prm->lattice_bounds);
    if ((prm->flags & PTV_FLAG_SLAB_CULL_AUTO) && can_cull && (g->z_begin > 0 || g->z_end < g->nz)) {
        c->rbf_chunks = 0;
        return run_knn_auto(c, p, g, prm, mask, U, V, W, s, st);
    }
    SearchParams sp = knn_search(prm);
    if (radius) {
        // fixed-radius IDW: one pass over the radius ball, no k-th distance bounds or seeds
        sp.k = 1;
        sp.lattice_bounds = -1;
    }
    KnnLaunch kl;
    Prepared pr;
    // slab cull (ptv_knn_params.slab_halo): bin only the particles near this z-slab
    Culled cu;
    c->cull_timed = false;
    if (prm->slab_halo > 0.0 && can_cull)
        PTV_TRY(cull_slab(c, p, g, prm->k, prm->slab_halo, nullptr, nullptr, 0, s, cu));
    PTV_TRY(prepare(c, cu.ok ? &cu.p : p, g, &sp, s, kl, pr, cu.ok ? cu.box : nullptr));
    if (cu.ok && kl.cb.dk == nullptr) {
        // no lattice bounds were built, so nothing proves the cull exact: bin every particle
        // instead (same result as slab_halo = 0), never refuse the call for it
        cu.ok = false;
        c->cull_timed = false;
        PTV_TRY(prepare(c, p, g, &sp, s, kl, pr));
    }
    if (cu.ok) {
        // the exactness proof runs on the device and gates the main launch (it writes nothing
        // unless the halo is proven); the host reads the proof back after it, so no
        // synchronisation stalls the stream between the lattice and the main launch
        PTV_TRY(c->halo_need.ensure(1));
        PTV_TRY(launch_halo_need(kl.cb.ax, kl.cb.ay, kl.cb.az, kl.cb.n[0], kl.cb.n[1], kl.cb.n[2], kl.cb.dk,
                                 c->cull_win.p, kl.cg.mg, c->halo_need.p, s));
        kl.gate = c->halo_need.p;
        kl.gate_halo = prm->slab_halo;
        PTV_TRY(c->ev_main0.record(s));
    }
    c->rbf_chunks = 0;
    if (radius) {
        kl.mode = kModeRadius;
        kl.radius = prm->radius;
    }
    PTV_TRY(launch_main(c, kl, pr, g, mask, U, V, W, s));
    if (cu.ok) {
        PTV_HIP(hipMemcpyAsync(c->h_misc.p + 1, c->halo_need.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipStreamSynchronize(s));
        double need;
        std::memcpy(&need, &c->h_misc.p[1], sizeof(need));
        c->last.n_particles = p->n;
        c->last.n_binned = cu.p.n;
        c->last.halo_required = need;
        if (!(need <= prm->slab_halo)) {
            if (st) *st = c->last;  // halo_required for the caller's retry
            set_error("slab cull not proven exact: slab_halo " + std::to_string(prm->slab_halo) +
                      " < required " + std::to_string(need) + " (retry with >= halo_required, or 0)");
            return PTV_E_INEXACT;
        }
    }
    if (st) *st = c->last;
    return PTV_OK;
}

// (k+1)-NN of every particle among the particles (slot mode, binned query order), then
// the per-particle median / MAD statistics
int run_filter(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep, double *kth,
               hipStream_t s) {
    const int64_t n = p->n;
    const int64_t npad = (n + 255) & ~(int64_t)255;  // 64 queries per wave tile, 4 tiles per block
    for (int i = 0; i < 3; ++i) PTV_TRY(c->qpts[i].ensure(npad));
    PTV_TRY(launch_pad_queries(p->x, p->y, p->z, n, npad, c->qpts[0].p, c->qpts[1].p, c->qpts[2].p, s));
    ptv_grid g{};
    g.nx = 16;  // 4 wave tiles along x per block (ptv_filter.hip pos_of)
    g.ny = 4;
    g.nz = npad / 64;
    g.px = c->qpts[0].p;
    g.py = c->qpts[1].p;
    g.pz = c->qpts[2].p;
    g.z_begin = 0;
    g.z_end = g.nz;
    double r0s = kFilterR0Scale, occ = kFilterOccupancy;
    if (const char *e = dev_knob("PTV_FILTER_R0")) r0s = std::atof(e);       // dev knobs
    if (const char *e = dev_knob("PTV_FILTER_OCC")) occ = std::atof(e);
    KnnLaunch kl;
    Prepared pr;
    c->rbf_chunks = 0;
    if (filter_kmax(prm->k) == 0) {
        // k >= 127: the large-k path on the particles in original order (ptv_knn_big.hip)
        const SearchParams sb{PTV_METHOD_IDW, prm->k + 1, 2.0, 1e-10, 0u, std::max(1.0, (prm->k + 1) / 256.0), 1.0, -1};
        c->cull_timed = false;
        PTV_TRY(prepare(c, p, &g, &sb, s, kl, pr));
        PTV_TRY(c->flt_spd.ensure((size_t)n));
        PTV_TRY(launch_slot_speed(pr.b.pval, n, c->flt_spd.p, s));
        BigQueries q;
        q.particles = 1;
        q.px = p->x;
        q.py = p->y;
        q.pz = p->z;
        q.pu = p->u;
        q.pv = p->v;
        q.pw = p->w;
        BigEpilogue ep;
        ep.filter = 1;
        ep.spd = c->flt_spd.p;
        ep.keep = keep;
        ep.kth = kth;
        ep.threshold = prm->threshold;
        ep.mad_eps = prm->mad_eps;
        PTV_TRY(run_big_knn(c->big, q, pr.b, pr.cg, n, prm->k + 1, ep, s));
        PTV_TRY(c->ev_knn1.record(s));
        c->timed_pending = true;
        c->last.n_voxels = n;
        return PTV_OK;
    }
    const SearchParams sp{PTV_METHOD_IDW, prm->k + 1, 2.0, 1e-10, 0u, occ, r0s, -1};
    PTV_TRY(prepare(c, p, &g, &sp, s, kl, pr));
    // query order: Morton order of the particles over the bounding box prepare() measured (pr.lo,
    // pr.hi), laid out in the k-NN kernel's sub-ball lane pattern (ptv_filter.hip)
    const size_t tb = morton_sort_temp_bytes(n);
    PTV_TRY(c->flt_code.ensure((size_t)npad));  // Morton keys, then the queries' original indices
    PTV_TRY(c->flt_count.ensure(n));
    PTV_TRY(c->flt_start.ensure(n));
    PTV_TRY(c->flt_perm.ensure(n));
    PTV_TRY(c->flt_scanp.ensure(tb / 4 + 1));
    PTV_TRY(launch_morton_order(p->x, p->y, p->z, n, pr.lo, pr.hi, c->flt_code.p, c->flt_count.p, c->flt_start.p,
                                c->flt_perm.p, c->flt_scanp.p, tb, s));
    // q_orig: the original index at each query position (reuses the Morton key buffer, dead
    // after the sort); the speeds of the binned particles in slot order
    uint32_t *q_orig = c->flt_code.p;
    PTV_TRY(launch_query_layout(c->flt_perm.p, p->x, p->y, p->z, n, npad, c->qpts[0].p, c->qpts[1].p, c->qpts[2].p,
                                q_orig, s));
    PTV_TRY(c->flt_spd.ensure((size_t)n));
    PTV_TRY(launch_slot_speed(pr.b.pval, n, c->flt_spd.p, s));
    // the (k+1)-NN search with the statistics fused into its epilogue (no slot list in HBM)
    kl.mode = kModeFilter;
    kl.fe.q_orig = q_orig;
    kl.fe.inv = c->code.p;  // the binning's inverse permutation (launch_bin: code = inv after the scatter)
    kl.fe.spd = c->flt_spd.p;
    kl.fe.keep = keep;
    kl.fe.kth = kth;
    kl.fe.threshold = prm->threshold;
    kl.fe.mad_eps = prm->mad_eps;
    PTV_TRY(launch_main(c, kl, pr, &g, nullptr, nullptr, nullptr, nullptr, s));
    c->last.n_voxels = n;
    return PTV_OK;
}

}  // namespace ptv
