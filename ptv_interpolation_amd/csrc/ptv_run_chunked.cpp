// ptv_run_chunked.cpp — the consumers that take each voxel's neighbour slots from HBM: the local RBF
// (run_rbf) and method='linear' (run_linear).  Both walk the slab in chunks of z planes: a k-NN pass
// in slot mode, then the consumer's kernel.
#include <algorithm>
#include <string>
#include <vector>

#include "ptv_ctx.hpp"

namespace ptv {

namespace {

// method='linear': the walk's step limit, and the voxels the brute-force location can take over
constexpr int kLinearMaxWalk = 4096;
constexpr int kLinearFlagCap = 1 << 20;

// The slab's planes in chunks whose k slots per voxel fit the context's slot buffer.
struct Chunks {
    int64_t z0, z1;
    int planes, count;
    int begin(int ch) const { return (int)(z0 + (int64_t)ch * planes); }
    int end(int ch) const { return (int)std::min<int64_t>(z1, begin(ch) + planes); }
};

// planes per chunk (chunk_planes <= 0: about 512 MB of slots per chunk), the slot buffer, and the
// context's three events per chunk
int plan_chunks(ptv_ctx *c, const ptv_grid *g, int chunk_planes, int k, Chunks &cs) {
    const int64_t plane = g->nx * g->ny;
    cs.z0 = g->z_begin;
    cs.z1 = g->z_end;
    int cp = chunk_planes;
    if (cp <= 0) {
        const int64_t per_plane = plane * (int64_t)k * 4;
        cp = (int)std::max<int64_t>(4, std::min<int64_t>(cs.z1 - cs.z0, ((int64_t)512 << 20) / std::max<int64_t>(per_plane, 1)));
    }
    cp = std::max(4, (cp + 3) & ~3);
    PTV_TRY(c->slots.ensure((size_t)std::min<int64_t>(cp, cs.z1 - cs.z0) * plane * k));
    cs.planes = cp;
    cs.count = (int)((cs.z1 - cs.z0 + cp - 1) / cp);
    if (c->rbf_ev.size() < 3 * (size_t)cs.count) c->rbf_ev.resize(3 * (size_t)cs.count);
    return PTV_OK;
}

// the slot search of chunk ch
KnnLaunch chunk_search(const ptv_ctx *c, const KnnLaunch &kl, const Chunks &cs, int ch) {
    KnnLaunch cl = kl;
    cl.z0 = cs.begin(ch);
    cl.z1 = cs.end(ch);
    cl.lz0 = (int)cs.z0;
    cl.mode = kModeSlots;
    cl.slots = c->slots.p;
    return cl;
}

}  // namespace

// monomial exponents of _monomial_powers(3, degree) (_rbfinterp.py:48-79), packed
std::vector<int> monomial_powers(int degree) {
    std::vector<int> out;
    for (int d = 0; d <= degree; ++d) {
        // combinations_with_replacement(range(3), d) in lexicographic order
        std::vector<int> idx(d, 0);
        while (true) {
            int pw[3] = {0, 0, 0};
            for (int v : idx) ++pw[v];
            out.push_back(pw[0] | (pw[1] << 8) | (pw[2] << 16));
            int i = d - 1;
            while (i >= 0 && idx[i] == 2) --i;
            if (i < 0) break;
            ++idx[i];
            for (int j = i + 1; j < d; ++j) idx[j] = idx[i];
        }
    }
    return out;
}

// Local RBF: per z chunk, a k-NN pass in slot mode, then the per-voxel solve.
int run_rbf(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_rbf_params *prm, int m,
            const double *smooth, const uint8_t *mask, double *U, double *V, double *W, hipStream_t s,
            int64_t *n_singular) {
    // k >= 128: the large-k slot search (ptv_knn_big.hip; no lattice, its own cell occupancy)
    const bool big = kmax_for(prm->k) == 0;
    const SearchParams sp{PTV_METHOD_IDW, prm->k, 2.0, 1e-10, 0u, big ? std::max(1.0, prm->k / 256.0) : 0.0, 0.0,
                          big ? -1 : 0};
    const Queries q = queries_of(g);
    KnnLaunch kl;
    Prepared pr;
    PTV_TRY(prepare(c, p, g, &sp, s, kl, pr));
    const std::vector<int> pw = monomial_powers(prm->degree);
    PTV_TRY(c->rbf_pw.ensure(pw.size() + 1));
    PTV_TRY(c->rbf_status.ensure(6));
    PTV_TRY(c->rbf_nslist.ensure(kRbfNsCap));
    if (!pw.empty())
        PTV_HIP(hipMemcpyAsync(c->rbf_pw.p, pw.data(), pw.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const int st_init[6] = {0, 0x7fffffff, 0, 0, 0, 0};

    const int64_t plane = g->nx * g->ny;
    Chunks cs;
    PTV_TRY(plan_chunks(c, g, prm->chunk_planes, prm->k, cs));
    const int nchunks = cs.count;
    RbfKernelArgs ra{};
    ra.nx = (int)g->nx;
    ra.ny = (int)g->ny;
    ra.out_z0 = (int)cs.z0;
    ra.separable = q.separable() ? 1 : 0;
    ra.k = prm->k;
    ra.m = m;
    ra.kernel = prm->kernel;
    ra.epsilon = prm->epsilon;
    ra.smoothing = prm->smoothing;
    ra.flags = prm->flags;
    if (m > kRbfMaxSystem) {
        // k_rbf_huge: persistent workgroups with a global-memory slice each (about 2 GB in total)
        const size_t slice = rbf_huge_slice_doubles(m, prm->k);
        const long long nb = std::max<long long>(64, std::min<long long>(4096, (2LL << 30) / (long long)(slice * 8)));
        PTV_TRY(c->rbf_huge.ensure((size_t)nb * slice));
        ra.huge_scratch = c->rbf_huge.p;
        ra.huge_blocks = (int)nb;
    }
    int st_out[6] = {0, 0, 0, 0, 0, 0};
    // per chunk: the voxels k_rbf_ns flagged (status[3] of its launch), whether they overflowed the
    // list (status[4]) and the running singular count (status[0]), copied on the device after each chunk
    PTV_TRY(c->rbf_cflag.ensure(3 * (size_t)nchunks));
    std::vector<int> cflag(3 * (size_t)nchunks, 0);
    std::vector<char> rerun((size_t)nchunks, 1);
    int64_t pivoted = 0;
    int64_t singular_redone = 0;  // pass 0's singular counts of the chunks an overflow rerun solves again
    for (int pass = 0; pass < 2; ++pass) {
    // pass 1 (rare): k_rbf_spd16 met a pivot its reciprocal does not serve (every chunk again with the
    // LDS-broadcast SPD kernel: the same arithmetic plus the IEEE division for such pivots), or
    // k_rbf_ns flagged more voxels in a chunk than its list holds (that chunk again, pivoting)
    ra.spd_lds = pass;
    ra.ns_list = pass == 0 ? c->rbf_nslist.p : nullptr;
    ra.ns_cap = kRbfNsCap;
    // (a full SPD rerun starts its counts afresh; an overflow rerun adds to pass 0's)
    if (pass == 0 || st_out[2] != 0)
        PTV_HIP(hipMemcpyAsync(c->rbf_status.p, st_init, sizeof(st_init), hipMemcpyHostToDevice, s));
    for (int ch = 0; ch < nchunks; ++ch) {
        if (!rerun[ch]) continue;
        const int za = cs.begin(ch), zb = cs.end(ch);
        PTV_TRY(c->rbf_ev[3 * ch].record(s));
        if (big) {
            BigEpilogue ep;
            ep.slots = c->slots.p;
            PTV_TRY(run_big_knn(c->big, big_queries(g, za, mask), pr.b, pr.cg, (int64_t)(zb - za) * plane, prm->k, ep, s));
        } else {
            PTV_TRY(launch_knn(chunk_search(c, kl, cs, ch), pr.b, q, mask, nullptr, nullptr, nullptr, s));
        }
        PTV_TRY(c->rbf_ev[3 * ch + 1].record(s));
        ra.z0 = za;
        ra.z1 = zb;
        PTV_TRY(launch_rbf(ra, pr.b, c->slots.p, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, smooth, c->rbf_pw.p, mask, U, V, W,
                           c->rbf_status.p, s));
        if (pass == 0) {
            PTV_HIP(hipMemcpyAsync(c->rbf_cflag.p + 3 * ch, c->rbf_status.p + 3, 2 * sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
            PTV_HIP(hipMemcpyAsync(c->rbf_cflag.p + 3 * ch + 2, c->rbf_status.p, sizeof(int),
                                   hipMemcpyDeviceToDevice, s));
            PTV_HIP(hipMemsetAsync(c->rbf_status.p + 4, 0, sizeof(int), s));
        }
        PTV_TRY(c->rbf_ev[3 * ch + 2].record(s));
    }
    PTV_HIP(hipMemcpyAsync(st_out, c->rbf_status.p, sizeof(st_out), hipMemcpyDeviceToHost, s));
    if (pass == 0)
        PTV_HIP(hipMemcpyAsync(cflag.data(), c->rbf_cflag.p, cflag.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (pass == 1) {
        st_out[0] -= (int)singular_redone;  // each rerun chunk's singular voxels, counted once
        break;
    }
    bool again = false;
    for (int ch = 0; ch < nchunks; ++ch) {
        const bool over = cflag[3 * ch + 1] != 0;
        // voxels the pivoting kernel solved: the flagged ones, or every voxel of an overflowed chunk
        pivoted += over ? (int64_t)(cs.end(ch) - cs.begin(ch)) * plane : cflag[3 * ch];
        rerun[ch] = (st_out[2] != 0 || over) ? 1 : 0;
        again = again || rerun[ch];
        if (over && st_out[2] == 0) singular_redone += cflag[3 * ch + 2] - (ch > 0 ? cflag[3 * ch - 1] : 0);
    }
    if (st_out[2] != 0) pivoted = 0;  // the SPD rerun: no null-space kernel ran
    if (!again) break;
    }
    c->rbf_chunks = nchunks;
    *n_singular = st_out[0];
    c->last.n_singular = st_out[0];
    c->last.n_rbf_pivoted = pivoted;
    if (st_out[0] > 0) {
        set_error("Singular matrix. (" + std::to_string(st_out[0]) + " voxel system(s), first at linear voxel " +
                  std::to_string(st_out[1]) + ")");
        return PTV_E_SINGULAR;
    }
    return PTV_OK;
}

// method='linear' on device pointers: binning + k = 1 slot search per z-chunk (the walk starts),
// the walk / interpolation kernel, then scipy's brute-force location for the flagged voxels.
int run_linear(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_linear_params *prm,
               const int32_t *simp, const int32_t *nbr, const double *tr, const int32_t *v2s, const uint8_t *mask,
               double *U, double *V, double *W, hipStream_t s) {
    const SearchParams sp{PTV_METHOD_NEAREST, 1, 2.0, 1e-10, 0u, 0.0, 0.0, 0};
    const Queries q = queries_of(g);
    KnnLaunch kl;
    Prepared pr;
    PTV_TRY(prepare(c, p, g, &sp, s, kl, pr));
    Chunks cs;
    PTV_TRY(plan_chunks(c, g, prm->chunk_planes, 1, cs));
    PTV_TRY(c->lin_count.ensure(1));
    PTV_TRY(c->lin_flags.ensure(kLinearFlagCap));
    PTV_HIP(hipMemsetAsync(c->lin_count.p, 0, sizeof(int), s));
    LinearKernelArgs la{};
    la.nx = (int)g->nx;
    la.ny = (int)g->ny;
    la.out_z0 = (int)cs.z0;
    la.separable = q.separable() ? 1 : 0;
    la.nsimplex = prm->nsimplex;
    la.simplices = simp;
    la.neighbors = nbr;
    la.transform = tr;
    la.v2s = v2s;
    la.pu = p->u;
    la.pv = p->v;
    la.pw = p->w;
    for (int d = 0; d < 3; ++d) {
        la.lo[d] = prm->min_bound[d];
        la.hi[d] = prm->max_bound[d];
    }
    la.fill = prm->fill_value;
    la.flags = prm->flags;
    la.max_walk = kLinearMaxWalk;
    la.flag_count = c->lin_count.p;
    la.flag_list = c->lin_flags.p;
    la.flag_cap = kLinearFlagCap;
    for (int ch = 0; ch < cs.count; ++ch) {
        PTV_TRY(c->rbf_ev[3 * ch].record(s));
        PTV_TRY(launch_knn(chunk_search(c, kl, cs, ch), pr.b, q, mask, nullptr, nullptr, nullptr, s));
        PTV_TRY(c->rbf_ev[3 * ch + 1].record(s));
        la.z0 = cs.begin(ch);
        la.z1 = cs.end(ch);
        PTV_TRY(launch_linear(la, pr.b.prec, c->slots.p, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, mask, U, V, W, s));
        PTV_TRY(c->rbf_ev[3 * ch + 2].record(s));
    }
    c->rbf_chunks = cs.count;
    int nflag = 0;
    PTV_HIP(hipMemcpyAsync(&nflag, c->lin_count.p, sizeof(int), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (nflag > kLinearFlagCap) {
        set_error("linear: " + std::to_string(nflag) + " voxels need the brute-force point location (limit " +
                  std::to_string(kLinearFlagCap) + "): degenerate triangulation");
        return PTV_E_UNSUPPORTED;
    }
    c->last.n_singular = nflag;  // reported: voxels located by the brute-force scan
    if (nflag > 0) {
        la.z0 = (int)cs.z0;
        la.z1 = (int)cs.z1;
        PTV_TRY(launch_linear_brute(la, nflag, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, U, V, W, s));
    }
    return PTV_OK;
}

}  // namespace ptv
