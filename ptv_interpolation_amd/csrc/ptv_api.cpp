// ptv_api.cpp — the C ABI (include/ptv_api.h) of the context and the interpolation: version and ABI
// sizes, ptv_init / ptv_free, argument validation, the host-buffer call of the interpolators (H2D,
// the device call, D2H, timings) and their entry points on device pointers, the debug stamps and the
// last call's statistics.
//
// The Python drop-in (ptv_interpolation_amd/interpolator.py) binds these symbols with
// ctypes; nothing here depends on torch.  The context is in ptv_ctx.hpp; the search preparation and
// the per-method runners the entry points call are in ptv_search.cpp, ptv_run_knn.cpp and
// ptv_run_chunked.cpp; the grid-field families are in ptv_grid_api.cpp, ptv_flow_api.cpp,
// ptv_mask_api.cpp, ptv_mesh_api.cpp, ptv_surface_api.cpp and ptv_label_api.cpp.
#include <cstdio>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <thread>

#include <sys/mman.h>
#include <vector>

#include "ptv_ctx.hpp"
#include "ptv_xcd_map.hpp"

namespace ptv {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

}  // namespace ptv

using namespace ptv;

extern "C" {

int ptv_version(void) { return PTV_API_VERSION; }

int ptv_abi_sizes(int64_t out6[6]) {
    if (!out6) {
        set_error("ptv_abi_sizes: out is NULL");
        return PTV_E_ARG;
    }
    out6[0] = (int64_t)sizeof(ptv_particles);
    out6[1] = (int64_t)sizeof(ptv_grid);
    out6[2] = (int64_t)sizeof(ptv_knn_params);
    out6[3] = (int64_t)sizeof(ptv_stats);
    out6[4] = (int64_t)sizeof(ptv_rbf_params);
    out6[5] = (int64_t)sizeof(ptv_div_params);
    return PTV_OK;
}

int ptv_abi_sizes2(int64_t out3[3]) {
    if (!out3) {
        set_error("ptv_abi_sizes2: out is NULL");
        return PTV_E_ARG;
    }
    out3[0] = (int64_t)sizeof(ptv_mask_grid);
    out3[1] = (int64_t)sizeof(ptv_boundary_params);
    out3[2] = (int64_t)sizeof(ptv_filter_params);
    return PTV_OK;
}

int ptv_abi_sizes3(int64_t out1[1]) {
    if (!out1) {
        set_error("ptv_abi_sizes3: out is NULL");
        return PTV_E_ARG;
    }
    out1[0] = (int64_t)sizeof(ptv_linear_params);
    return PTV_OK;
}

int ptv_abi_sizes4(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes4: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_clean_params);
    out2[1] = (int64_t)sizeof(ptv_clean_stats);
    return PTV_OK;
}

int ptv_abi_sizes5(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes5: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_variational_params);
    out2[1] = (int64_t)sizeof(ptv_variational_stats);
    return PTV_OK;
}

int ptv_abi_sizes6(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes6: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_flow_params);
    out2[1] = (int64_t)sizeof(ptv_flow_stats);
    return PTV_OK;
}

int ptv_abi_sizes7(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes7: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_drag_params);
    out2[1] = (int64_t)sizeof(ptv_drag_stats);
    return PTV_OK;
}

int ptv_abi_sizes8(int64_t out4[4]) {
    if (!out4) {
        set_error("ptv_abi_sizes8: out is NULL");
        return PTV_E_ARG;
    }
    out4[0] = (int64_t)sizeof(ptv_edt_params);
    out4[1] = (int64_t)sizeof(ptv_edt_stats);
    out4[2] = (int64_t)sizeof(ptv_align_params);
    out4[3] = (int64_t)sizeof(ptv_align_record);
    return PTV_OK;
}

int ptv_abi_sizes9(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes9: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_pressure_params);
    out2[1] = (int64_t)sizeof(ptv_pressure_stats);
    return PTV_OK;
}

int ptv_abi_sizes10(int64_t out3[3]) {
    if (!out3) {
        set_error("ptv_abi_sizes10: out is NULL");
        return PTV_E_ARG;
    }
    out3[0] = (int64_t)sizeof(ptv_spline_params);
    out3[1] = (int64_t)sizeof(ptv_mesh_params);
    out3[2] = (int64_t)sizeof(ptv_mesh_record);
    return PTV_OK;
}

int ptv_abi_sizes11(int64_t out1[1]) {
    if (!out1) {
        set_error("ptv_abi_sizes11: out is NULL");
        return PTV_E_ARG;
    }
    out1[0] = (int64_t)sizeof(ptv_surface_params);
    return PTV_OK;
}

int ptv_abi_sizes12(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes12: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_label_params);
    out2[1] = (int64_t)sizeof(ptv_label_stats);
    return PTV_OK;
}

int ptv_abi_sizes13(int64_t out2[2]) {
    if (!out2) {
        set_error("ptv_abi_sizes13: out is NULL");
        return PTV_E_ARG;
    }
    out2[0] = (int64_t)sizeof(ptv_mg_params);
    out2[1] = (int64_t)sizeof(ptv_mg_stats);
    return PTV_OK;
}

const char *ptv_last_error(void) { return g_last_error.c_str(); }

int ptv_device_count(int *out) {
    if (!out) {
        set_error("ptv_device_count: out is NULL");
        return PTV_E_ARG;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return PTV_OK;
}

int ptv_init(int device, ptv_ctx **out) {
    if (!out) {
        set_error("ptv_init: out is NULL");
        return PTV_E_ARG;
    }
    *out = nullptr;
    int n = 0;
    PTV_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("ptv_init: device " + std::to_string(device) + " out of range (" + std::to_string(n) + " visible)");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(device));
    std::unique_ptr<ptv_ctx> c(new ptv_ctx());
    c->device = device;
    PTV_TRY(c->stream.create());
    *out = c.release();
    return PTV_OK;
}

int ptv_free(ptv_ctx *c) {
    if (!c) return PTV_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (ptv::g_dbg == c->dbg.p) ptv::g_dbg = nullptr;
    delete c;  // every member frees what it owns; the stream goes last
    return PTV_OK;
}

}  // extern "C"

namespace {

int validate(const ptv_particles *p, const ptv_grid *g, const void *prm) {
    if (!p || !g || !prm) {
        set_error("NULL particles/grid/params");
        return PTV_E_ARG;
    }
    if (p->n <= 0 || !p->x || !p->y || !p->z || !p->u || !p->v || !p->w) {
        set_error("particles: need n > 0 and six non-NULL arrays");
        return PTV_E_ARG;
    }
    if (p->n >= (int64_t)1 << 31) {
        set_error("particles: n must be < 2^31");
        return PTV_E_ARG;
    }
    if (g->nx <= 0 || g->ny <= 0 || g->nz <= 0 || g->nx > (1 << 30) || g->ny > (1 << 30)) {
        set_error("grid: dimensions must be positive");
        return PTV_E_ARG;
    }
    const bool sep = g->ax && g->ay && g->az;
    const bool pts = g->px && g->py && g->pz;
    if (!sep && !pts) {
        set_error("grid: give either the three axes or the three point arrays");
        return PTV_E_ARG;
    }
    if (g->z_begin < 0 || g->z_end > g->nz || g->z_begin > g->z_end) {
        set_error("grid: bad z slab [" + std::to_string(g->z_begin) + ", " + std::to_string(g->z_end) + ")");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int validate_knn(const ptv_particles *p, const ptv_knn_params *prm) {
    if (prm->method != PTV_METHOD_IDW && prm->method != PTV_METHOD_SIBSON && prm->method != PTV_METHOD_NEAREST &&
        prm->method != PTV_METHOD_IDW_RADIUS) {
        set_error("unknown method " + std::to_string(prm->method));
        return PTV_E_ARG;
    }
    if (prm->method == PTV_METHOD_IDW_RADIUS) {
        if (!(prm->radius > 0.0 && std::isfinite(prm->radius))) {
            set_error("PTV_METHOD_IDW_RADIUS needs a positive finite radius");
            return PTV_E_ARG;
        }
        return PTV_OK;  // k is not used
    }
    if (prm->k < 1) {
        set_error("k must be >= 1");
        return PTV_E_ARG;
    }
    if ((int64_t)prm->k > p->n) {
        set_error("k=" + std::to_string(prm->k) + " exceeds the number of particles " + std::to_string(p->n));
        return PTV_E_ARG;
    }
    // k beyond the register lists (kmax_for(k) == 0, k >= 128) takes the large-k path (run_knn_big)
    return PTV_OK;
}

int validate_rbf(const ptv_particles *p, const ptv_rbf_params *prm, int *m_out) {
    if (prm->flags & PTV_FLAG_OUT_F32) {
        set_error("local RBF: PTV_FLAG_OUT_F32 is supported by the k-NN methods only");
        return PTV_E_UNSUPPORTED;
    }
    if (prm->kernel < PTV_RBF_LINEAR || prm->kernel > PTV_RBF_GAUSSIAN) {
        set_error("unknown RBF kernel " + std::to_string(prm->kernel));
        return PTV_E_ARG;
    }
    if (prm->k < 1 || (int64_t)prm->k > p->n) {
        set_error("k must be in [1, n]");
        return PTV_E_ARG;
    }
    if (prm->degree < -1 || prm->degree > 8) {
        set_error("degree must be in [-1, 8]");
        return PTV_E_ARG;
    }
    if (!std::isfinite(prm->epsilon)) {
        set_error("epsilon must be finite");
        return PTV_E_ARG;
    }
    const int nm = (int)monomial_powers(prm->degree).size();
    if (nm > prm->k) {
        set_error("At least " + std::to_string(nm) + " data points are required when `degree` is " +
                  std::to_string(prm->degree) + " and the number of dimensions is 3.");
        return PTV_E_ARG;
    }
    const int m = prm->k + nm;
    if (rbf_system_size(m) == 0) {
        set_error("local RBF system of size " + std::to_string(m) + " (k=" + std::to_string(prm->k) +
                  ") exceeds the GPU limit (" + std::to_string(kRbfMaxSystem) + ")");
        return PTV_E_UNSUPPORTED;
    }
    *m_out = m;
    return PTV_OK;
}

}  // namespace

namespace ptv {

int finish_timing(ptv_ctx *c) {
    float ms = 0.f;
    if (c->div_pending) {
        PTV_HIP(hipEventSynchronize(c->ev_div1));
        PTV_HIP(hipEventElapsedTime(&ms, c->ev_div0, c->ev_div1));
        c->last.ms_stencil = ms;
        c->div_pending = false;
    }
    if (!c->timed_pending) return PTV_OK;
    if (c->rbf_chunks > 0) {
        PTV_HIP(hipEventSynchronize(c->rbf_ev[3 * c->rbf_chunks - 1]));
        double knn = 0.0, solve = 0.0;
        for (int ch = 0; ch < c->rbf_chunks; ++ch) {
            PTV_HIP(hipEventElapsedTime(&ms, c->rbf_ev[3 * ch], c->rbf_ev[3 * ch + 1]));
            knn += ms;
            PTV_HIP(hipEventElapsedTime(&ms, c->rbf_ev[3 * ch + 1], c->rbf_ev[3 * ch + 2]));
            solve += ms;
        }
        c->last.ms_knn = knn;
        c->last.ms_solve = solve;
    } else {
        PTV_HIP(hipEventSynchronize(c->ev_knn1));
        PTV_HIP(hipEventElapsedTime(&ms, c->ev_main0, c->ev_knn1));
        c->last.ms_knn = ms;
    }
    if (c->cull_timed) {
        float a = 0.f, b = 0.f;
        PTV_HIP(hipEventElapsedTime(&a, c->ev_cull0, c->ev_cull1));
        PTV_HIP(hipEventElapsedTime(&b, c->ev_lat1, c->ev_main0));
        c->last.ms_cull = (double)a + (double)b;
    }
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_knn0, c->ev_lat1));
    c->last.ms_lattice = ms;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_bin0, c->ev_bin1));
    c->last.ms_bin = ms;
    c->timed_pending = false;
    return PTV_OK;
}

// finish_timing, and a host-buffer call's own legs: ev = call start, H2D end, D2H start, call end
int finish_host_timing(ptv_ctx *c, const Event ev[4]) {
    PTV_TRY(finish_timing(c));
    float h2d = 0.f, d2h = 0.f, tot = 0.f;
    PTV_HIP(hipEventElapsedTime(&h2d, ev[0], ev[1]));
    PTV_HIP(hipEventElapsedTime(&d2h, ev[2], ev[3]));
    PTV_HIP(hipEventElapsedTime(&tot, ev[0], ev[3]));
    c->last.ms_h2d = h2d;
    c->last.ms_d2h = d2h;
    c->last.ms_total = tot;
    return PTV_OK;
}

// The six particle columns -> the context's buffers.
int upload_particles(ptv_ctx *c, const ptv_particles *p, hipStream_t s, ptv_particles &dp) {
    const double *src[6] = {p->x, p->y, p->z, p->u, p->v, p->w};
    for (int i = 0; i < 6; ++i) {
        PTV_TRY(c->pin[i].ensure(p->n));
        PTV_HIP(hipMemcpyAsync(c->pin[i].p, src[i], p->n * sizeof(double), hipMemcpyHostToDevice, s));
    }
    dp = ptv_particles{p->n, c->pin[0].p, c->pin[1].p, c->pin[2].p, c->pin[3].p, c->pin[4].p, c->pin[5].p};
    return PTV_OK;
}

// The grid's axes (separable) or point lists -> the context's buffers; dg = the grid on the device.
int upload_grid(ptv_ctx *c, const ptv_grid *g, hipStream_t s, ptv_grid &dg) {
    dg = *g;
    if (queries_of(g).separable()) {
        PTV_TRY(c->axes.ensure(g->nx + g->ny + g->nz));
        PTV_HIP(hipMemcpyAsync(c->axes.p, g->ax, g->nx * sizeof(double), hipMemcpyHostToDevice, s));
        PTV_HIP(hipMemcpyAsync(c->axes.p + g->nx, g->ay, g->ny * sizeof(double), hipMemcpyHostToDevice, s));
        PTV_HIP(hipMemcpyAsync(c->axes.p + g->nx + g->ny, g->az, g->nz * sizeof(double), hipMemcpyHostToDevice, s));
        dg.ax = c->axes.p;
        dg.ay = c->axes.p + g->nx;
        dg.az = c->axes.p + g->nx + g->ny;
        dg.px = dg.py = dg.pz = nullptr;
    } else {
        const int64_t nfull = g->nz * g->nx * g->ny;
        const double *q[3] = {g->px, g->py, g->pz};
        for (int i = 0; i < 3; ++i) {
            PTV_TRY(c->qpts[i].ensure(nfull));
            PTV_HIP(hipMemcpyAsync(c->qpts[i].p, q[i], nfull * sizeof(double), hipMemcpyHostToDevice, s));
        }
        dg.ax = dg.ay = dg.az = nullptr;
        dg.px = c->qpts[0].p;
        dg.py = c->qpts[1].p;
        dg.pz = c->qpts[2].p;
    }
    return PTV_OK;
}

}  // namespace ptv

namespace {

// First-touch of the caller's output pages on host threads while the device works.  A fresh
// (never written) host buffer pays a page fault per 4 KiB page inside the D2H copy: measured
// on the MI355X box, 1 GiB into fresh pageable memory 65-72 ms against 19 ms (52 GiB/s) into
// touched memory, and pinning (hipHostMalloc / hipHostRegister) costs the same ~45 ms/GiB.  The
// faults are taken in parallel here (a write per page; the D2H then overwrites every byte), so
// only the copy remains on the critical path.  Joined before the D2H is enqueued, and on every
// early return.
constexpr int kMadvPopulateWrite = 23;  // MADV_POPULATE_WRITE (Linux 5.14), absent from older headers

struct PageToucher {
    std::vector<std::thread> th;
    void start(void *const *bufs, int nbuf, size_t bytes) {
        constexpr size_t kPage = 4096, kMin = (size_t)32 << 20;
        if (bytes < kMin) return;
        const unsigned hw = std::thread::hardware_concurrency();
        const int nt = (int)std::max(1u, std::min(16u, hw ? hw : 1u));
        const size_t pages = (bytes + kPage - 1) / kPage;
        for (int t = 0; t < nt; ++t) {
            const size_t p0 = pages * t / nt, p1 = pages * (t + 1) / nt;
            std::vector<char *> b(nbuf);
            for (int i = 0; i < nbuf; ++i) b[i] = static_cast<char *>(bufs[i]);
            th.emplace_back([b, p0, p1, bytes]() {
                // fault the pages in writable WITHOUT changing them (a failed call must leave the
                // caller's arrays as they were): MADV_POPULATE_WRITE where the kernel has it, else a
                // volatile read-modify-write of one byte per page
                for (char *base : b) {
                    const uintptr_t lo = (reinterpret_cast<uintptr_t>(base) + p0 * kPage) & ~(uintptr_t)(kPage - 1);
                    const uintptr_t hi = reinterpret_cast<uintptr_t>(base) + std::min(p1 * kPage, bytes);
                    if (hi > lo && madvise(reinterpret_cast<void *>(lo), hi - lo, kMadvPopulateWrite) == 0) continue;
                    for (size_t pg = p0; pg < p1; ++pg) {
                        volatile char *q = base + std::min(pg * kPage, bytes - 1);
                        *q = *q;
                    }
                }
            });
        }
    }
    void join() {
        for (auto &t : th) t.join();
        th.clear();
    }
    ~PageToucher() { join(); }
};

// Host-buffer call: H2D into the context's buffers, `compute` on device pointers, D2H of
// the slab's three output planes, timings.  compute(dp, dg, dmask, dsmooth, U, V, W, s).
template <typename F>
int host_call(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const uint8_t *mask_h, const double *smooth_h,
              double *U, double *V, double *W, F &&compute, size_t out_elem = sizeof(double)) {
    hipStream_t s = c->stream;
    Event ev[4];
    const int64_t n = p->n;
    const int64_t plane = g->nx * g->ny;
    const int64_t nvox = (g->z_end - g->z_begin) * plane;
    const int64_t nfull = g->nz * plane;
    PageToucher touch;
    {
        void *outs[3] = {U, V, W};
        touch.start(outs, 3, (size_t)nvox * out_elem);
    }
    PTV_TRY(ev[0].record(s));
    ptv_particles dp;
    PTV_TRY(upload_particles(c, p, s, dp));
    ptv_grid dg;
    PTV_TRY(upload_grid(c, g, s, dg));
    const uint8_t *dmask = nullptr;
    if (mask_h) {
        PTV_TRY(c->mask.ensure(nfull));
        PTV_HIP(hipMemcpyAsync(c->mask.p, mask_h, nfull, hipMemcpyHostToDevice, s));
        dmask = c->mask.p;
    }
    const double *dsmooth = nullptr;
    if (smooth_h) {
        PTV_TRY(c->smooth.ensure(n));
        PTV_HIP(hipMemcpyAsync(c->smooth.p, smooth_h, n * sizeof(double), hipMemcpyHostToDevice, s));
        dsmooth = c->smooth.p;
    }
    for (int i = 0; i < 3; ++i) PTV_TRY(c->out[i].ensure(nvox));
    PTV_TRY(ev[1].record(s));
    PTV_TRY(compute(&dp, &dg, dmask, dsmooth, c->out[0].p, c->out[1].p, c->out[2].p, s));
    PTV_TRY(ev[2].record(s));
    touch.join();
    double *dst[3] = {U, V, W};
    for (int i = 0; i < 3; ++i)
        PTV_HIP(hipMemcpyAsync(dst[i], c->out[i].p, nvox * out_elem, hipMemcpyDeviceToHost, s));
    PTV_TRY(ev[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    PTV_TRY(finish_host_timing(c, ev));
    return PTV_OK;
}

int check_call(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const void *prm, double *U, double *V,
               double *W) {
    if (!c) {
        set_error("NULL context");
        return PTV_E_ARG;
    }
    PTV_TRY(validate(p, g, prm));
    if (!U || !V || !W) {
        set_error("NULL output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_interp_knn_dev(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, double *U,
                       double *V, double *W, void *stream, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    PTV_TRY(validate_knn(p, prm));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return run_knn(c, p, g, prm, prm->fluid_mask, U, V, W, s, st);
}

int ptv_interp_knn(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_knn_params *prm, double *U,
                   double *V, double *W, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    PTV_TRY(validate_knn(p, prm));
    PTV_TRY(host_call(c, p, g, prm->fluid_mask, nullptr, U, V, W,
                      [&](const ptv_particles *dp, const ptv_grid *dg, const uint8_t *dmask, const double *,
                          double *dU, double *dV, double *dW, hipStream_t s) {
                          // st: on PTV_E_INEXACT the caller gets halo_required (host_call returns early)
                          return run_knn(c, dp, dg, prm, dmask, dU, dV, dW, s, st);
                      },
                      (prm->flags & PTV_FLAG_OUT_F32) ? sizeof(float) : sizeof(double)));
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_interp_rbf_local_dev(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_rbf_params *prm,
                             double *U, double *V, double *W, void *stream, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    int m = 0;
    PTV_TRY(validate_rbf(p, prm, &m));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    int64_t nsing = 0;
    const int rc = run_rbf(c, p, g, prm, m, prm->smoothing_per_point, prm->fluid_mask, U, V, W, s, &nsing);
    c->timed_pending = true;
    if (st) *st = c->last;
    return rc;
}

int ptv_interp_rbf_local(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_rbf_params *prm,
                         double *U, double *V, double *W, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    int m = 0;
    PTV_TRY(validate_rbf(p, prm, &m));
    PTV_TRY(host_call(c, p, g, prm->fluid_mask, prm->smoothing_per_point, U, V, W,
                      [&](const ptv_particles *dp, const ptv_grid *dg, const uint8_t *dmask, const double *dsmooth,
                          double *dU, double *dV, double *dW, hipStream_t s) {
                          int64_t nsing = 0;
                          const int rc = run_rbf(c, dp, dg, prm, m, dsmooth, dmask, dU, dV, dW, s, &nsing);
                          c->timed_pending = true;
                          return rc;
                      }));
    if (st) *st = c->last;
    return PTV_OK;
}

static int validate_linear(const ptv_particles *p, const ptv_linear_params *prm) {
    if (!prm || !prm->simplices || !prm->neighbors || !prm->transform || !prm->vertex_to_simplex) {
        set_error("linear: NULL parameters or triangulation array");
        return PTV_E_ARG;
    }
    if (prm->nsimplex < 1 || prm->nsimplex > 0x7fffffffLL) {
        set_error("linear: nsimplex must be in [1, 2^31)");
        return PTV_E_ARG;
    }
    if (p->n > 0x7fffffffLL) {
        set_error("linear: more than 2^31 particles");
        return PTV_E_ARG;
    }
    if (prm->flags & ~PTV_FLAG_NAN_TO_NUM) {
        set_error("linear: only PTV_FLAG_NAN_TO_NUM is supported");
        return PTV_E_UNSUPPORTED;
    }
    return PTV_OK;
}

int ptv_interp_linear_dev(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_linear_params *prm,
                          double *U, double *V, double *W, void *stream, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    PTV_TRY(validate_linear(p, prm));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int rc = run_linear(c, p, g, prm, prm->simplices, prm->neighbors, prm->transform, prm->vertex_to_simplex,
                              prm->fluid_mask, U, V, W, s);
    c->timed_pending = true;
    if (st) *st = c->last;
    return rc;
}

int ptv_interp_linear(ptv_ctx *c, const ptv_particles *p, const ptv_grid *g, const ptv_linear_params *prm,
                      double *U, double *V, double *W, ptv_stats *st) {
    PTV_TRY(check_call(c, p, g, prm, U, V, W));
    PTV_TRY(validate_linear(p, prm));
    PTV_TRY(host_call(c, p, g, prm->fluid_mask, nullptr, U, V, W,
                      [&](const ptv_particles *dp, const ptv_grid *dg, const uint8_t *dmask, const double *,
                          double *dU, double *dV, double *dW, hipStream_t s) {
                          const size_t ns = (size_t)prm->nsimplex, n = (size_t)p->n;
                          PTV_TRY(c->lin_simp.ensure(4 * ns));
                          PTV_TRY(c->lin_nbr.ensure(4 * ns));
                          PTV_TRY(c->lin_tr.ensure(12 * ns));
                          PTV_TRY(c->lin_v2s.ensure(n));
                          PTV_HIP(hipMemcpyAsync(c->lin_simp.p, prm->simplices, 4 * ns * sizeof(int), hipMemcpyHostToDevice, s));
                          PTV_HIP(hipMemcpyAsync(c->lin_nbr.p, prm->neighbors, 4 * ns * sizeof(int), hipMemcpyHostToDevice, s));
                          PTV_HIP(hipMemcpyAsync(c->lin_tr.p, prm->transform, 12 * ns * sizeof(double), hipMemcpyHostToDevice, s));
                          PTV_HIP(hipMemcpyAsync(c->lin_v2s.p, prm->vertex_to_simplex, n * sizeof(int), hipMemcpyHostToDevice, s));
                          const int rc = run_linear(c, dp, dg, prm, c->lin_simp.p, c->lin_nbr.p, c->lin_tr.p, c->lin_v2s.p,
                                                    dmask, dU, dV, dW, s);
                          c->timed_pending = true;
                          return rc;
                      }));
    if (st) *st = c->last;
    return PTV_OK;
}

constexpr long long kStampCap = 1LL << 21;  // waves recorded
constexpr int kXcdStampFields = 3;          // ptv_knn_impl.hpp: kStampXcdFields

int ptv_debug_xcd_stamps(ptv_ctx *c, unsigned long long *out, long long cap, long long *n_out) {
    if (!c || !out || !n_out || cap < 0) {
        set_error("NULL argument");
        return PTV_E_ARG;
    }
    *n_out = 0;
    if (!c->dbg.p) return PTV_OK;
    PTV_HIP(hipSetDevice(c->device));
    PTV_HIP(hipDeviceSynchronize());
    const long long n = std::min(cap, kStampCap);
    PTV_HIP(hipMemcpy(out, c->dbg.p + (size_t)kStampCap * 8, (size_t)n * kXcdStampFields * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    *n_out = n;
    return PTV_OK;
}

int ptv_debug_xcd_chunk(int blocks) {
    ptv::g_xcd_chunk = blocks < 0 ? -1 : blocks;
    return PTV_OK;
}

int ptv_xcd_chunk_map(int nblocks, int chunk, int *out) {
    if (nblocks < 0 || (nblocks > 0 && !out)) {
        set_error("ptv_xcd_chunk_map: bad arguments");
        return PTV_E_ARG;
    }
    for (int lb = 0; lb < nblocks; ++lb) out[lb] = ptv::xcd_chunk_block(lb, nblocks, chunk);
    return PTV_OK;
}

int ptv_debug_stamps(ptv_ctx *c, int mode, double *out) {
    if (!c) {
        set_error("NULL context");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    constexpr long long cap = kStampCap;  // modulo-free: later waves dropped
    constexpr int nf = 8;
    if (mode == 1) {  // enable + zero: the phase records, then the plane of XCD records
        PTV_TRY(c->dbg.ensure((size_t)cap * (nf + kXcdStampFields)));
        PTV_HIP(hipMemsetAsync(c->dbg.p, 0, (size_t)cap * (nf + kXcdStampFields) * sizeof(unsigned long long), c->stream));
        PTV_HIP(hipStreamSynchronize(c->stream));
        ptv::g_dbg = c->dbg.p;
        ptv::g_dbg_cap = cap;
    } else if (mode == 0) {
        ptv::g_dbg = nullptr;
        ptv::g_dbg_cap = 0;
    }
    if (out && c->dbg.p) {
        PTV_HIP(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)cap * nf);
        PTV_HIP(hipMemcpy(h.data(), c->dbg.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (const char *dump = dev_knob("PTV_STAMPS_DUMP")) {  // raw per-wave records (dev tool)
            if (FILE *f = std::fopen(dump, "wb")) {
                std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
                std::fclose(f);
            }
        }
        // out: [records, mean of 11 fields, max of 11 fields]: 6 phase cycle counts, then
        // gathered candidates, merge iterations, rounds, passes, candidates kept by the
        // sub-ball filter (packed two or three to a u64 in fields 6 and 7)
        constexpr int nv = 11;
        double sum[nv] = {0}, mx[nv] = {0};
        long long nrec = 0;
        for (long long w = 0; w < cap; ++w) {
            const unsigned long long *r = &h[(size_t)w * nf];
            if (r[0] == 0 && r[2] == 0 && r[5] == 0) continue;
            ++nrec;
            double v[nv];
            for (int f = 0; f < 6; ++f) v[f] = (double)r[f];
            v[6] = (double)(r[6] & 0xffffffffULL);
            v[7] = (double)(r[6] >> 32);
            v[8] = (double)(r[7] & 0xffffULL);
            v[9] = (double)((r[7] >> 16) & 0xffffULL);
            v[10] = (double)(r[7] >> 32);
            for (int f = 0; f < nv; ++f) {
                sum[f] += v[f];
                mx[f] = std::max(mx[f], v[f]);
            }
        }
        out[0] = (double)nrec;
        for (int f = 0; f < nv; ++f) {
            out[1 + f] = nrec ? sum[f] / (double)nrec : 0.0;
            out[1 + nv + f] = mx[f];
        }
    }
    return PTV_OK;
}

int ptv_last_stats(ptv_ctx *c, ptv_stats *st) {
    if (!c || !st) {
        set_error("NULL argument");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    PTV_TRY(finish_timing(c));
    *st = c->last;
    return PTV_OK;
}

}  // extern "C"
