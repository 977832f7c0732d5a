// ptv_search.cpp — what every k-NN consumer runs first: prepare() (bounding box, binning, coarse
// lattice of k-th distance bounds, launch template), and the slab cull that may run before it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ptv_ctx.hpp"

namespace ptv {

namespace {

// particles per binning cell: the k <= 8 kernels (seeded, sub-ball filtered copy) are fastest
// with coarse cells (fewer, longer runs per row: 512^3 / 5M k=8 main launch 19.1 -> 16.5 ms
// from 1.2 to 5.5); the larger-k kernels prefer fine cells (k=50: 477 ms at 1.2, 493 at 5.5)
// measured on the 512^3 / 5M sphere pack, k = 8 (tools/void_split.py, round 2): per-cell
// occupancy 16 / 12 with cells 12x thinner along x (16 particles per x-column of 12 cells)
// gave k-NN 14.9 ms against 16.3 ms for cubic cells of 5.5, the lattice 2.31 against 2.44
constexpr double kDefaultOccupancySmallK = 16.0;  // particles per (y, z) cell column segment
constexpr double kDefaultXRefSmallK = 12.0;       // x-refinement of the k <= 8 cells
constexpr double kDefaultOccupancy = 1.2;          // k > 8 without lattice seeds (point lists)
// k > 8 with union seeds (round 3, a dev-knob sweep, now tools/gpu_envab.sh, 512^3 / 5M IDW k = 50): the seeded
// gather radius is tight, so coarser cells (fewer runs per row) win again: main launch
// 139.7 ms at 1.2 / cubic, 137.7 at 2.5, 134.8 at 5, 133.5 at 8 with x 4x thinner, 133.4 at 16 / 12
constexpr double kDefaultOccupancyLargeK = 8.0;
constexpr double kDefaultXRefLargeK = 4.0;
constexpr double kDefaultR0Scale = 1.0;     // first gather radius / expected k-NN radius
constexpr long long kMaxCells = 1LL << 28;
constexpr long long kLatticeStopPoints = 50000; // no coarser lattice below this many points
constexpr size_t kSeedBytesMax = 40ULL << 30;    // lattice seed records per level (C5 2048^3, k = 8: 17 GB)
// split lattice launch (k_kdist_merge): the first max(kLatticeSplitMinBlocks, blocks /
// kLatticeSplitDiv) blocks of a lattice level's longest-first order, kLatticeSplit waves per tile.
// Measured (512^3 / 5M sphere pack, k = 8, a dev-knob sweep, now tools/gpu_envab.sh): the share 2/8 lattice 1.81 ->
// 0.88 ms at 64 blocks (1.07 at 32, 2.05 at 8), C2 0.81 -> 0.69; the whole 512^3 grid's lattice
// launch is throughput-bound (35.9k tiles of ~280k cycles each), 1.91 -> 1.86 ms
constexpr int kLatticeSplit = 16;
constexpr long long kLatticeSplitMinBlocks = 64;
constexpr long long kLatticeSplitDiv = 128;
// cap on the split launch's partial-list buffer (split_blocks * 4 * kLatticeSplit * KMAX * 64 slots,
// memset once per level): 64 MiB = 512 blocks at KMAX 8, 32 at 128; the measured win came from the
// first ~64 blocks, while nb / 128 at 2048^3 would be ~4300 blocks (0.56 GB at k = 8, 9 GB at 127)
constexpr size_t kLatticeSplitBytesMax = 64ULL << 20;
// binning: the radix sort above this many particles, the atomic counting sort below (crossover
// ~2.6M from the two measured points, profiles/r06_ab/bin_sort_ab.txt)
constexpr int64_t kBinSortMinParticles = 2500000;

// Cell grid over the union bounding box: ~`occ` particles per cell on average.
CellGrid make_cell_grid(const double lo_in[3], const double hi_in[3], int64_t n, double occ, double xref_in) {
    CellGrid cg{};
    double ext[3];
    double maxext = 0.0, maxabs = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi_in[a] - lo_in[a];
        if (!(ext[a] > 0.0)) ext[a] = 0.0;
        maxext = std::max(maxext, ext[a]);
        maxabs = std::max(maxabs, std::max(std::fabs(lo_in[a]), std::fabs(hi_in[a])));
    }
    if (!(occ > 0.0)) occ = kDefaultOccupancy;
    if (const char *e = dev_knob("PTV_CELL_OCC")) occ = std::atof(e);  // dev override
    double vol = 1.0;
    int dims = 0;
    for (int a = 0; a < 3; ++a)
        if (ext[a] > 1e-9 * maxext) {
            vol *= ext[a];
            ++dims;
        }
    double cs = dims ? std::pow(occ * vol / (double)n, 1.0 / dims) : 1.0;
    // x-refinement: cells `xref` times thinner along x (occupancy / xref per cell).  A gather
    // run is a contiguous x-range of cells whose cost is its two cstart loads whatever its
    // length, so thin x-cells trim the runs' ends (fewer candidates outside the sub-balls)
    // without adding rows.
    double xref = std::max(1.0, xref_in);
    if (const char *e = dev_knob("PTV_CELL_XREF")) xref = std::max(1.0, std::atof(e));  // dev override
    for (int iter = 0; iter < 64; ++iter) {  // cap the cell count (memory) by growing cs
        long long tot = 1;
        for (int a = 0; a < 3; ++a) {
            int nc = 1;
            const double csa = a == 0 ? cs / xref : cs;
            if (ext[a] > 1e-9 * maxext && csa > 0.0) nc = (int)std::max(1.0, std::min(1e6, std::ceil(ext[a] / csa)));
            cg.nc[a] = nc;
            tot *= nc;
        }
        cg.ncells = tot;
        if (tot <= kMaxCells) break;
        cs *= 1.1;
    }
    for (int a = 0; a < 3; ++a) {
        cg.cs[a] = ext[a] > 0.0 ? ext[a] / cg.nc[a] : 1.0;
        cg.ic[a] = 1.0 / cg.cs[a];
        cg.o[a] = lo_in[a];
    }
    cg.mg = 1e-12 * (maxabs + maxext) + 1e-300;
    return cg;
}

// First gather radius: the radius of a ball expected to hold k particles at the mean
// density of the bounding box, times `scale` (every lane's k-th distance usually fits).
double first_radius(const double lo[3], const double hi[3], int64_t n, int k, double scale) {
    if (!(scale > 0.0)) scale = kDefaultR0Scale;
    double vol = 1.0, maxext = 0.0;
    int dims = 0;
    for (int a = 0; a < 3; ++a) maxext = std::max(maxext, hi[a] - lo[a]);
    for (int a = 0; a < 3; ++a)
        if (hi[a] - lo[a] > 1e-9 * maxext) {
            vol *= hi[a] - lo[a];
            ++dims;
        }
    if (dims == 0 || maxext <= 0.0) return 1.0;
    const double unit = dims == 3 ? 4.18879020478639 : (dims == 2 ? 3.14159265358979 : 2.0);
    return scale * std::pow((double)k * vol / ((double)n * unit), 1.0 / dims);
}

// The slab's query coordinates as launch_bbox takes them.
void bbox_queries(const ptv_grid *g, const double *qa[3], int64_t qn[3]) {
    const Queries q = queries_of(g);
    const int64_t plane = g->nx * g->ny, z0 = g->z_begin, nz = g->z_end - g->z_begin;
    if (q.separable()) {
        qa[0] = q.ax;
        qa[1] = q.ay;
        qa[2] = q.az + z0;
        qn[0] = g->nx;
        qn[1] = g->ny;
        qn[2] = nz;
    } else {
        qa[0] = q.qx + z0 * plane;
        qa[1] = q.qy + z0 * plane;
        qa[2] = q.qz + z0 * plane;
        qn[0] = qn[1] = qn[2] = nz * plane;
    }
}

// 1. bounding box of particles + this slab's queries, and the coordinate-range check
int measure_bbox(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, hipStream_t s, const double *box6,
                 Prepared &pr) {
    PTV_TRY(c->bbox_part.ensure(6 * 1024));
    PTV_TRY(c->bbox_out.ensure(8));
    PTV_TRY(c->h_bbox.ensure(kHostWords));
    PTV_TRY(c->h_misc.ensure(kHostWords));
    PTV_TRY(c->ev_bin0.record(s));
    if (box6 == nullptr) {  // (the slab cull reads it back together with its kept count)
        const double *pp[3] = {p->x, p->y, p->z};
        const double *qa[3];
        int64_t qn[3];
        bbox_queries(g, qa, qn);
        PTV_TRY(launch_bbox(pp, p->n, qa, qn, c->bbox_part.p, 1024, c->bbox_out.p, s));
        PTV_HIP(hipMemcpyAsync(c->h_bbox.p, c->bbox_out.p, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipStreamSynchronize(s));
        box6 = c->h_bbox.p;
    }
    for (int a = 0; a < 3; ++a) {
        pr.lo[a] = box6[a];
        pr.hi[a] = box6[3 + a];
        if (!std::isfinite(pr.lo[a]) || !std::isfinite(pr.hi[a])) {
            set_error("non-finite particle or grid coordinates");
            return PTV_E_ARG;
        }
    }
    // squared distances must neither overflow nor lose bits to underflow in float64 (the tested range
    // is 2^-80 .. 2^80 of unit coordinates)
    double maxabs = 0.0, maxext = 0.0;
    for (int a = 0; a < 3; ++a) {
        maxabs = std::max(maxabs, std::max(std::fabs(pr.lo[a]), std::fabs(pr.hi[a])));
        maxext = std::max(maxext, pr.hi[a] - pr.lo[a]);
    }
    if (maxabs > 0x1p500 || (maxext > 0.0 && maxext < 0x1p-500)) {
        set_error("coordinates outside the supported range: |coordinate| <= 2^500 and a bounding box of "
                  "extent 0 or >= 2^-500");
        return PTV_E_UNSUPPORTED;
    }
    return PTV_OK;
}

// 2. binning: the cell grid over the box, the particles sorted into its cells
int bin_particles(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const SearchParams *prm, hipStream_t s,
                  Prepared &pr) {
    const int64_t n = p->n;
    const bool small_k = kmax_for(prm->k) <= 8;
    // union seeds bound the large-k search
    const bool seeded_lattice = queries_of(g).separable() && prm->lattice_bounds >= 0;
    const bool given = prm->cell_occupancy > 0.0;
    const double occ = given ? prm->cell_occupancy
                       : (small_k ? kDefaultOccupancySmallK : (seeded_lattice ? kDefaultOccupancyLargeK : kDefaultOccupancy));
    const double xref = given ? 1.0 : (small_k ? kDefaultXRefSmallK : (seeded_lattice ? kDefaultXRefLargeK : 1.0));
    pr.cg = make_cell_grid(pr.lo, pr.hi, n, occ, xref);
    const size_t m = (size_t)pr.cg.ncells;
    PTV_TRY(c->code.ensure(2 * (size_t)n));  // cell codes + in-cell ranks (launch_bin)
    PTV_TRY(c->perm.ensure(n));
    PTV_TRY(c->prec.ensure(n));
    PTV_TRY(c->pval.ensure(n));
    PTV_TRY(c->count.ensure(m));
    PTV_TRY(c->start.ensure(m + 1));
    PTV_TRY(c->scanp.ensure(scan_partials_needed(m) + 1));
    const double *pp[3] = {p->x, p->y, p->z};
    const double *pv[3] = {p->u, p->v, p->w};
    // sort-based binning (a stable radix sort of (cell, index) pairs) from kBinSortMinParticles:
    // 512^3 / 5M binning 0.81 -> 0.68 ms against the atomic histogram + scatter + in-cell sort,
    // the 0.73M particles of share 2/8 0.134 -> 0.22 ms (profiles/r06_ab/bin_sort_ab.txt)
    BinSortScratch ss;
    const char *bs = dev_knob("PTV_BIN_SORT");  // dev knob: 0 = the atomic counting sort, 1 = the sort
    const bool use_sort = bs ? bs[0] == '1' : n >= kBinSortMinParticles;
    const size_t tb = use_sort ? bin_sort_temp_bytes(n, m) : 0;
    if (tb > 0) {
        PTV_TRY(c->bin_keys.ensure((size_t)n));
        PTV_TRY(c->bin_temp.ensure(std::max<size_t>(tb, 1)));
        ss.keys = c->bin_keys.p;
        ss.temp = c->bin_temp.p;
        ss.temp_bytes = tb;
    }
    PTV_TRY(launch_bin(pr.cg, pp, pv, n, c->code.p, c->perm.p, c->count.p, c->start.p, c->scanp.p, c->prec.p,
                       c->pval.p, s, &ss));
    PTV_TRY(c->ev_bin1.record(s));
    pr.b = Binned{c->prec.p, c->pval.p, c->start.p, n};
    pr.r0 = first_radius(pr.lo, pr.hi, n, prm->k, prm->r0_scale);
    return PTV_OK;
}

// The launch of planes [z_begin, z_end) over the binned particles, before any lattice bound.
KnnLaunch search_launch(const ptv_grid *g, const SearchParams *prm, const Prepared &pr) {
    KnnLaunch kl;
    kl.cg = pr.cg;
    kl.nx = (int)g->nx;
    kl.ny = (int)g->ny;
    kl.nz = (int)g->nz;
    kl.z0 = (int)g->z_begin;
    kl.z1 = (int)g->z_end;
    kl.separable = queries_of(g).separable() ? 1 : 0;
    kl.method = prm->method == PTV_METHOD_NEAREST ? PTV_METHOD_IDW : prm->method;
    kl.k = prm->k;
    kl.power = prm->power;
    kl.eps = prm->eps;
    kl.flags = prm->flags;
    kl.r0 = pr.r0;
    return kl;
}

// Whether a grid of n[0] x n[1] x n[2] points gets a coarser lattice level above it.
bool lattice_level_above(const long long n[3]) {
    long long stop = kLatticeStopPoints;
    if (const char *e = dev_knob("PTV_LAT_STOP")) stop = std::atoll(e);  // dev override
    return n[0] * n[1] * n[2] > stop && std::min(n[0], std::min(n[1], n[2])) >= 9;
}

// dev builds (PTV_DBG_ORDER, PTV_DBG_LATDK): dims, then nd device doubles and ni device ints, to a file
int dump_lattice(const char *path, const int dims[3], const double *dd, size_t nd, const int *di, size_t ni,
                 hipStream_t s) {
    std::vector<double> hd(nd);
    std::vector<int> hi(ni);
    if (ni) PTV_HIP(hipMemcpyAsync(hi.data(), di, ni * sizeof(int), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipMemcpyAsync(hd.data(), dd, nd * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (FILE *f = std::fopen(path, "wb")) {
        std::fwrite(dims, sizeof(int), 3, f);
        std::fwrite(hd.data(), sizeof(double), nd, f);
        std::fwrite(hi.data(), sizeof(int), ni, f);
        std::fclose(f);
    }
    return PTV_OK;
}

// 3. coarse-lattice k-th distance bounds (separable grids): every 4th point of the
//    grid, recursively, down to a few tens of thousands of points; each level is an
//    exact k-NN pass (k-th distance only) bounded by the next coarser level.
//    Leaves the finest level in pr.cb.
int build_lattice(ptv_ctx *c, const ptv_grid *g, const SearchParams *prm, hipStream_t s, bool exact_finest,
                  Prepared &pr) {
    // Seed records for the main launch (the finest level's k-NN lists) pay for the pair lists (k <=
    // 12): headline 22.4 -> 14.1 ms with them, k = 12 33.2 -> 29.4 ms.  For the packed-key lists (k >=
    // 13) the union-seed counting costs more than its tighter bound saves, and the finest level then
    // writes no records either (1.7 GB per launch at k = 50).  Same-box A/B, 512^3 / 5M, main launch
    // + lattice without / with them: k = 16 34.8 + 2.14 / 35.9 + 2.23 ms, Sibson k = 30 54.1 + 2.71 /
    // 55.2 + 2.84, IDW k = 50 102.3 + 5.13 / 104.2 + 5.40, Sibson k = 50 137.9 + 5.09 / 138.8 +
    // 5.38, RBF slot searches k = 20 29.0 / 29.9 and C3 48.4 / 50.0.
    bool main_seeds = kmax_for(prm->k) <= 12;
    if (const char *e = dev_knob("PTV_MAIN_SEEDS")) main_seeds = e[0] == '1';  // dev knob: 1 = always, 0 = never
    struct Lat {
        int n[3];
        double *ax, *ay, *az, *dk;
        float4 *recs;   // NULL on the coarsest (count-bound) level and past kSeedBytesMax
    };
    auto bound_of = [](const Lat &L) { return CoarseBound{L.ax, L.ay, L.az, L.dk, L.recs, {L.n[0], L.n[1], L.n[2]}}; };
    Lat lat[kMaxLattice];
    int nlat = 0;
    const Queries q = queries_of(g);
    if (q.separable() && prm->lattice_bounds >= 0) {
        int n[3] = {(int)g->nx, (int)g->ny, (int)(g->z_end - g->z_begin)};
        // every level's axes from the grid's in one launch (each level takes every 4th point of the
        // one above it, plus the last)
        SubsampleBatch sb{};
        for (int d = 0; d < 3; ++d) sb.n0[d] = n[d];
        sb.base[0] = q.ax;
        sb.base[1] = q.ay;
        sb.base[2] = q.az + g->z_begin;
        while (nlat < kMaxLattice) {
            const long long nl[3] = {n[0], n[1], n[2]};
            const int nmin = std::min(n[0], std::min(n[1], n[2]));
            // exact_finest (the slab cull map): a count-bound level above the finest, which is then an
            // exact k-th distance level (its bounds do not depend on the binning cells)
            if (!lattice_level_above(nl) && !(exact_finest && nlat == 1 && nmin >= 2)) break;
            Lat &L = lat[nlat];
            for (int d = 0; d < 3; ++d) L.n[d] = n[d] <= 1 ? 1 : (n[d] - 1 + kLatticeStep - 1) / kLatticeStep + 1;
            PTV_TRY(c->lat_axes[nlat].ensure((size_t)L.n[0] + L.n[1] + L.n[2]));
            PTV_TRY(c->lat_dk[nlat].ensure((size_t)L.n[0] * L.n[1] * L.n[2]));
            L.ax = c->lat_axes[nlat].p;
            L.ay = L.ax + L.n[0];
            L.az = L.ay + L.n[1];
            L.dk = c->lat_dk[nlat].p;
            L.recs = nullptr;
            double *dst[3] = {L.ax, L.ay, L.az};
            for (int d = 0; d < 3; ++d) {
                sb.n[nlat][d] = L.n[d];
                sb.out[nlat][d] = dst[d];
                n[d] = L.n[d];
            }
            ++nlat;
        }
        sb.nlev = nlat;
        if (nlat > 0) PTV_TRY(launch_subsample_levels(sb, kLatticeStep, s));
    }

    const KnnLaunch kl = search_launch(g, prm, pr);
    PTV_TRY(c->ev_knn0.record(s));
    for (int l = nlat - 1; l >= 0; --l) {  // coarsest first
        if (l == nlat - 1) {
            // coarsest lattice: count-only upper bounds (no candidate is read)
            PTV_TRY(launch_count_bound(pr.cg, c->start.p, lat[l].ax, lat[l].ay, lat[l].az, lat[l].n[0], lat[l].n[1],
                                       lat[l].n[2], prm->k, pr.r0, lat[l].dk, s));
            continue;
        }
        // seed records (each lattice point's k-NN, 16 B each) for the next finer level's tiles,
        // unless they would take more than kSeedBytesMax (then the D(c) + |v - c| bound alone)
        const size_t nrec = (size_t)lat[l].n[0] * lat[l].n[1] * lat[l].n[2] * prm->k;
        if ((l > 0 || main_seeds) && nrec * sizeof(float4) <= kSeedBytesMax) {
            PTV_TRY(c->lat_recs[l].ensure(nrec));
            lat[l].recs = c->lat_recs[l].p;
        }
        KnnLaunch ll = kl;
        const char *no_order = dev_knob("PTV_NO_LAT_ORDER");  // dev knob: 1 = XCD-contiguous order
        if (!(no_order && no_order[0] == '1')) {
            const long long nb = (long long)(((lat[l].n[0] + 3) / 4 + 3) / 4) * ((lat[l].n[1] + 3) / 4) *
                                 ((lat[l].n[2] + 3) / 4);
            PTV_TRY(c->lat_order[l].ensure((size_t)nb));
            PTV_TRY(c->lat_okeys.ensure((size_t)nb + 1));
            PTV_TRY(launch_block_order(lat[l + 1].dk, lat[l + 1].n, lat[l].n[0], lat[l].n[1], lat[l].n[2], pr.r0,
                                       c->lat_order[l].p, c->lat_okeys.p, s));
            ll.order = c->lat_order[l].p;
            if (const char *e = dev_knob("PTV_DBG_ORDER"))  // dev builds: the order and the coarser bounds
                if (l == 0)
                    PTV_TRY(dump_lattice(e, lat[1].n, lat[1].dk, (size_t)lat[1].n[0] * lat[1].n[1] * lat[1].n[2],
                                         ll.order, (size_t)nb, s));
            // the first blocks of the order (the void tiles) as a split launch (k_kdist_merge)
            int split = kLatticeSplit;
            long long sblk = std::min<long long>(nb, std::max<long long>(kLatticeSplitMinBlocks, nb / kLatticeSplitDiv));
            if (const char *e = dev_knob("PTV_LAT_SPLIT")) split = std::atoi(e);          // dev: 0 = off
            if (const char *e = dev_knob("PTV_LAT_SPLIT_BLOCKS")) sblk = std::min<long long>(nb, std::atoll(e));
            if (split > 1)
                sblk = std::min<long long>(sblk, (long long)(kLatticeSplitBytesMax / sizeof(uint32_t) /
                                                             kdist_split_slots(split, 1, kmax_for(prm->k))));
            if (split > 1 && sblk > 0) {
                PTV_TRY(c->lat_split.ensure(kdist_split_slots(split, (int)sblk, kmax_for(prm->k))));
                ll.split = split;
                ll.split_blocks = (int)sblk;
                ll.split_out = c->lat_split.p;
            }
        }
        ll.kd_recs = lat[l].recs;
        ll.nx = lat[l].n[0];
        ll.ny = lat[l].n[1];
        ll.nz = lat[l].n[2];
        ll.z0 = 0;
        ll.z1 = lat[l].n[2];
        ll.mode = kModeKDist;
        ll.flags = 0;
        ll.cb = bound_of(lat[l + 1]);
        if (const char *e = dev_knob("PTV_LAT_SEEDS"))  // dev knob: 0 = lattice levels unseeded
            if (e[0] == '0') ll.cb.recs = nullptr;
        PTV_TRY(launch_knn(ll, pr.b, lat[l].ax, lat[l].ay, lat[l].az, nullptr, nullptr, nullptr, nullptr, lat[l].dk,
                           lat[l].dk, lat[l].dk, s));
    }
    pr.cb = nlat > 0 ? bound_of(lat[0]) : CoarseBound{};  // (recs: NULL unless main_seeds)
    PTV_TRY(c->ev_lat1.record(s));
    if (const char *e = dev_knob("PTV_DBG_LATDK"))  // dev builds: the finest lattice bounds to a file
        if (nlat > 0)
            PTV_TRY(dump_lattice(e, lat[0].n, lat[0].dk, (size_t)lat[0].n[0] * lat[0].n[1] * lat[0].n[2], nullptr, 0, s));
    return PTV_OK;
}

// 4. launch template (k-NN search + consumer), the call's stats, the near-tie repair list
int fill_launch(ptv_ctx *c, const ptv_grid *g, const SearchParams *prm, hipStream_t s, const Prepared &pr,
                KnnLaunch &kl) {
    kl = search_launch(g, prm, pr);
    kl.cb = pr.cb;
    PTV_TRY(c->ev_main0.record(s));  // moved to the main launch when a check runs in between
    const int64_t nz = g->z_end - g->z_begin;
    ptv_stats &ls = c->last;
    ls = ptv_stats{};
    ls.n_particles = pr.b.n;
    ls.n_voxels = nz * g->nx * g->ny;
    ls.n_cells = (int64_t)pr.cg.nc[0] * pr.cg.nc[1] * pr.cg.nc[2];
    for (int a = 0; a < 3; ++a) {
        ls.cells[a] = pr.cg.nc[a];
        ls.cell_size[a] = pr.cg.cs[a];
    }
    ls.r0 = pr.r0;
    ls.n_binned = pr.b.n;
    ls.halo_required = -1.0;
    if (kmax_for(prm->k) >= 16) {
        // packed-key lists: the near-tie repair list (tiles whose order the keys did not prove;
        // a handful per launch: past the cap the whole launch reruns exact)
        const long long tiles = (long long)((g->nx + 3) / 4) * ((g->ny + 3) / 4) * ((nz + 3) / 4);
        // (PTV_FLAG_KNN_REPAIR_ALL: a one-entry list, so any second listed tile reruns the whole launch)
        const int cap = (prm->flags & PTV_FLAG_KNN_REPAIR_ALL)
                            ? 1
                            : (int)std::max<long long>(1, std::min<long long>(tiles, 1LL << 22));
        PTV_TRY(c->rep_cnt.ensure(1));
        PTV_TRY(c->rep_list.ensure((size_t)cap));
        kl.rep_cnt = c->rep_cnt.p;
        kl.rep_list = c->rep_list.p;
        kl.rep_cap = cap;
        kl.h_rep = reinterpret_cast<unsigned int *>(c->h_misc.p + 2);
        kl.n_repair = &ls.n_repair_tiles;
    }
    return PTV_OK;
}

}  // namespace

int prepare(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const SearchParams *prm, hipStream_t s,
            KnnLaunch &kl, Prepared &pr, const double *box6, bool exact_finest) {
    PTV_TRY(measure_bbox(c, p, g, s, box6, pr));
    PTV_TRY(bin_particles(c, p, g, prm, s, pr));
    PTV_TRY(build_lattice(c, g, prm, s, exact_finest, pr));
    return fill_launch(c, g, prm, s, pr, kl);
}

bool lattice_built(const ptv_grid *g, int lattice_bounds) {
    const long long n[3] = {g->nx, g->ny, g->z_end - g->z_begin};
    return lattice_bounds >= 0 && lattice_level_above(n);
}

// Cull the particles to those a slab can need: within `halo` of its z extent, or, with `map`, by the
// per-column map.  The kept particles' bounding box (with the slab's query planes) is reduced from
// the count on the device and read back with the count: one host synchronisation for the cull and
// the cell grid.  With `spec` (the speculative reuse of the cached map) nothing is read back: the
// device checks this call's data key (c->cfp, nkey doubles) and kept count against the cache's,
// failing the gate c->halo_need, and the cache's count and box stand in.
int cull_slab(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, int k, double halo, const CullMap *map,
              const CullCache *spec, size_t nkey, hipStream_t s, Culled &out) {
    const int64_t n = p->n;
    const size_t nb = cull_blocks(n);
    for (auto &d : c->cull) PTV_TRY(d.ensure(n));
    PTV_TRY(c->cull_win.ensure(4));
    PTV_TRY(c->cull_cnt.ensure(nb + 1));
    PTV_TRY(c->cull_mask.ensure(cull_mask_words(n)));
    PTV_TRY(c->h_bbox.ensure(kHostWords));
    PTV_TRY(c->h_misc.ensure(kHostWords));
    const double *src[6] = {p->x, p->y, p->z, p->u, p->v, p->w};
    double *dst[6];
    for (int a = 0; a < 6; ++a) dst[a] = c->cull[a].p;
    const double *az = queries_of(g).az;
    out.ok = false;
    c->cull_timed = false;
    PTV_TRY(c->ev_cull0.record(s));
    int64_t kept;
    if (spec) {  // the gate: a kept particle with a non-finite coordinate fails it too (no box is reduced)
        PTV_TRY(c->halo_need.ensure(1));
        PTV_HIP(hipMemsetAsync(c->halo_need.p, 0, sizeof(unsigned long long), s));
    }
    PTV_TRY(launch_cull(src, n, az, (int)g->z_begin, (int)g->z_end, halo, c->cull_win.p, c->cull_cnt.p,
                        c->cull_mask.p, dst, nullptr, s, map, spec ? c->halo_need.p : nullptr));
    if (spec) {
        // the cached kept count and bounding box (the same particles give the same), checked on
        // the device: a mismatch fails the gate and the call reruns with every particle binned
        PTV_TRY(launch_key_check(c->cfp.p, spec->key_dev.p, (int)nkey, c->cull_cnt.p + nb, (uint32_t)spec->kept,
                                 c->halo_need.p, s));
        PTV_TRY(c->ev_cull1.record(s));
        kept = spec->kept;
        std::memcpy(out.box, spec->bbox, sizeof(out.box));
    } else {
        PTV_TRY(c->bbox_part.ensure(6 * 1024));
        PTV_TRY(c->bbox_out.ensure(8));
        const double *kp[3] = {dst[0], dst[1], dst[2]};
        const double *qa[3];
        int64_t qn[3];
        bbox_queries(g, qa, qn);
        uint32_t *h_total = reinterpret_cast<uint32_t *>(c->h_misc.p);
        PTV_TRY(launch_bbox(kp, n, qa, qn, c->bbox_part.p, 1024, c->bbox_out.p, s, c->cull_cnt.p + nb));
        PTV_HIP(hipMemcpyAsync(c->h_bbox.p, c->bbox_out.p, 6 * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipMemcpyAsync(h_total, c->cull_cnt.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        PTV_TRY(c->ev_cull1.record(s));
        PTV_HIP(hipStreamSynchronize(s));
        kept = (int64_t)*h_total;
        std::memcpy(out.box, c->h_bbox.p, sizeof(out.box));
        if (kept < k) return PTV_OK;  // fewer than k could never be proven exact: bin everything
    }
    out.p = ptv_particles{kept, dst[0], dst[1], dst[2], dst[3], dst[4], dst[5]};
    out.ok = true;
    c->cull_timed = true;
    return PTV_OK;
}

}  // namespace ptv
