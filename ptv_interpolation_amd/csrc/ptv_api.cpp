// ptv_api.cpp — the C ABI (include/ptv_api.h): argument validation, the host-buffer calls (H2D,
// the device call, D2H, timings) and the entry points on device pointers.
//
// The Python drop-in (ptv_interpolation_amd/interpolator.py) binds these symbols with
// ctypes; nothing here depends on torch.  The context is in ptv_ctx.hpp; the search preparation and
// the per-method runners the entry points call are in ptv_search.cpp, ptv_run_knn.cpp and
// ptv_run_chunked.cpp.
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

// ptv_div_params -> DivArgs, with the same checks for the host and device calls.
int div_args(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W, const void *out,
             DivArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!U || !V || !W || !out || !prm->fluid_mask) {
        set_error("divergence: NULL field, output or fluid mask");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30)) {
        set_error("divergence: dimensions must be positive");
        return PTV_E_ARG;
    }
    const int64_t lo = prm->edge_lo ? 0 : 1, hi = prm->nz - (prm->edge_hi ? 0 : 1);
    if (prm->z_begin < lo || prm->z_end > hi || prm->z_begin > prm->z_end) {
        set_error("divergence: planes [" + std::to_string(prm->z_begin) + ", " + std::to_string(prm->z_end) +
                  ") must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) +
                  ") (a non-edge buffer end is a halo plane)");
        return PTV_E_ARG;
    }
    if ((prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) ||
        (prm->result_dtype != PTV_F64 && prm->result_dtype != PTV_F32)) {
        set_error("divergence: dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.z_begin = (int)prm->z_begin;
    a.z_end = (int)prm->z_end;
    a.edge_lo = prm->edge_lo ? 1 : 0;
    a.edge_hi = prm->edge_hi ? 1 : 0;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.result_f32 = prm->result_dtype == PTV_F32;
    a.dx = prm->dx;
    a.dy = prm->dy;
    a.dz = prm->dz;
    if (!a.field_f32 && a.result_f32) {
        set_error("divergence: float64 fields cannot give float32 results (numpy promotion)");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int run_div(ptv_ctx *c, const DivArgs &a, const void *U, const void *V, const void *W, const uint8_t *M, void *out,
            hipStream_t s) {
    PTV_TRY(c->ev_div0.record(s));
    PTV_TRY(launch_divergence(a, U, V, W, M, out, s));
    PTV_TRY(c->ev_div1.record(s));
    c->div_pending = true;
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

int ptv_debug_stamps(ptv_ctx *c, int mode, double *out) {
    if (!c) {
        set_error("NULL context");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    constexpr long long cap = 1LL << 21;  // waves recorded (modulo-free: later waves dropped)
    constexpr int nf = 8;
    if (mode == 1) {  // enable + zero
        PTV_TRY(c->dbg.ensure((size_t)cap * nf));
        PTV_HIP(hipMemsetAsync(c->dbg.p, 0, (size_t)cap * nf * sizeof(unsigned long long), c->stream));
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

int ptv_divergence_dev(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W,
                       void *out, void *stream, ptv_stats *st) {
    DivArgs a{};
    PTV_TRY(div_args(c, prm, U, V, W, out, a));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_div(c, a, U, V, W, prm->fluid_mask, out, s));
    c->last.n_voxels = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_divergence(ptv_ctx *c, const ptv_div_params *prm, const void *U, const void *V, const void *W, void *out,
                   ptv_stats *st) {
    DivArgs a{};
    PTV_TRY(div_args(c, prm, U, V, W, out, a));
    hipStream_t s = c->stream;
    Event ev[4];
    const size_t ts = a.field_f32 ? 4 : 8, rs = a.result_f32 ? 4 : 8;
    const int64_t nfull = prm->nz * prm->nx * prm->ny;
    const int64_t nout = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    PTV_TRY(ev[0].record(s));
    const void *src[3] = {U, V, W};
    for (int i = 0; i < 3; ++i) {
        PTV_TRY(c->fld[i].ensure(nfull * ts));
        PTV_HIP(hipMemcpyAsync(c->fld[i].p, src[i], nfull * ts, hipMemcpyHostToDevice, s));
    }
    PTV_TRY(c->mask.ensure(nfull));
    PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, nfull, hipMemcpyHostToDevice, s));
    PTV_TRY(c->fld[3].ensure(nout * rs));
    PTV_TRY(ev[1].record(s));
    PTV_TRY(run_div(c, a, c->fld[0].p, c->fld[1].p, c->fld[2].p, c->mask.p, c->fld[3].p, s));
    PTV_TRY(ev[2].record(s));
    PTV_HIP(hipMemcpyAsync(out, c->fld[3].p, nout * rs, hipMemcpyDeviceToHost, s));
    PTV_TRY(ev[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    PTV_TRY(finish_host_timing(c, ev));
    c->last.n_voxels = nout;
    if (st) *st = c->last;
    return PTV_OK;
}

// ---- divergence cleaning (ptv_clean.hip) ----
static int clean_check(ptv_ctx *c, const ptv_clean_params *prm, CleanGrid &g) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!prm->fluid_mask) {
        set_error("clean: the fluid mask is required");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30) || prm->nx * prm->ny * prm->nz > 0x7fff0000LL) {
        set_error("clean: dimensions must be positive, with fewer than 2^31 voxels");
        return PTV_E_ARG;
    }
    g.nx = (int)prm->nx;
    g.ny = (int)prm->ny;
    g.nz = (int)prm->nz;
    g.dx = prm->dx;
    g.dy = prm->dy;
    g.dz = prm->dz;
    return PTV_OK;
}

// host fields -> c->clean_fld[0..nf), mask -> c->mask
static int clean_upload(ptv_ctx *c, const ptv_clean_params *prm, const double *const *src, int nf, hipStream_t s) {
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    for (int i = 0; i < nf; ++i) {
        PTV_TRY(c->clean_fld[i].ensure(n));
        PTV_HIP(hipMemcpyAsync(c->clean_fld[i].p, src[i], n * sizeof(double), hipMemcpyHostToDevice, s));
    }
    PTV_TRY(c->mask.ensure(n));
    PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, n, hipMemcpyHostToDevice, s));
    return PTV_OK;
}

// c->clean_fld[0..3) -> host fields
static int clean_download(ptv_ctx *c, const ptv_clean_params *prm, double *Uo, double *Vo, double *Wo, hipStream_t s) {
    const size_t nbytes = (size_t)(prm->nx * prm->ny * prm->nz) * sizeof(double);
    double *dst[3] = {Uo, Vo, Wo};
    for (int i = 0; i < 3; ++i)
        PTV_HIP(hipMemcpyAsync(dst[i], c->clean_fld[i].p, nbytes, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_clean_divergence_dev(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                             const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                             ptv_clean_stats *st) {
    CleanGrid g{};
    PTV_TRY(clean_check(c, prm, g));
    if (!U || !V || !W || !Uo || !Vo || !Wo) {
        set_error("clean: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const CleanSolve sv{prm->iterations, prm->damp, prm->atol, prm->btol, prm->iter_lim};
    return clean_run(c->clean, g, sv, prm->fluid_mask, U, V, W, Uo, Vo, Wo, s, st);
}

int ptv_clean_divergence(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, double *Uo, double *Vo, double *Wo, ptv_clean_stats *st) {
    CleanGrid g{};
    PTV_TRY(clean_check(c, prm, g));
    if (!U || !V || !W || !Uo || !Vo || !Wo) {
        set_error("clean: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[3] = {U, V, W};
    PTV_TRY(clean_upload(c, prm, src, 3, s));
    const CleanSolve sv{prm->iterations, prm->damp, prm->atol, prm->btol, prm->iter_lim};
    double *d[3] = {c->clean_fld[0].p, c->clean_fld[1].p, c->clean_fld[2].p};
    PTV_TRY(clean_run(c->clean, g, sv, c->mask.p, d[0], d[1], d[2], d[0], d[1], d[2], s, st));
    return clean_download(c, prm, Uo, Vo, Wo, s);
}

int ptv_apply_correction(ptv_ctx *c, const ptv_clean_params *prm, const double *U, const double *V,
                         const double *W, const double *phi_grid, double *Uo, double *Vo, double *Wo) {
    CleanGrid g{};
    PTV_TRY(clean_check(c, prm, g));
    if (!U || !V || !W || !phi_grid || !Uo || !Vo || !Wo) {
        set_error("apply_correction: NULL field, phi or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[4] = {U, V, W, phi_grid};
    PTV_TRY(clean_upload(c, prm, src, 4, s));
    double *d[3] = {c->clean_fld[0].p, c->clean_fld[1].p, c->clean_fld[2].p};
    PTV_TRY(launch_clean_correction(g, c->mask.p, d[0], d[1], d[2], c->clean_fld[3].p, d[0], d[1], d[2], s));
    return clean_download(c, prm, Uo, Vo, Wo, s);
}

int ptv_laplacian_apply(ptv_ctx *c, const ptv_clean_params *prm, const double *x_grid, double *y_grid) {
    CleanGrid g{};
    PTV_TRY(clean_check(c, prm, g));
    if (!x_grid || !y_grid) {
        set_error("laplacian_apply: NULL input or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[1] = {x_grid};
    PTV_TRY(clean_upload(c, prm, src, 1, s));
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_TRY(c->clean_fld[1].ensure(n));
    PTV_TRY(launch_clean_laplacian(g, c->mask.p, c->clean_fld[0].p, c->clean_fld[1].p, s));
    PTV_HIP(hipMemcpyAsync(y_grid, c->clean_fld[1].p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

// ---- variational divergence cleaning (ptv_variational.hip) ----
static int var_check(ptv_ctx *c, const ptv_variational_params *prm, VarGrid &g) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!prm->fluid_mask) {
        set_error("variational: the fluid mask is required");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30) || prm->nx * prm->ny * prm->nz > 0x7fff0000LL) {
        set_error("variational: dimensions must be positive, with fewer than 2^31 voxels");
        return PTV_E_ARG;
    }
    g.nx = (int)prm->nx;
    g.ny = (int)prm->ny;
    g.nz = (int)prm->nz;
    g.dx = prm->dx;
    g.dy = prm->dy;
    g.dz = prm->dz;
    return PTV_OK;
}

// host grids -> c->var_fld[0..nf), mask -> c->mask; var_fld[nf..nbuf) are sized for the results
static int var_upload(ptv_ctx *c, const ptv_variational_params *prm, const double *const *src, int nf, int nbuf,
                      hipStream_t s) {
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    for (int i = 0; i < nbuf; ++i) PTV_TRY(c->var_fld[i].ensure(n));
    for (int i = 0; i < nf; ++i)
        PTV_HIP(hipMemcpyAsync(c->var_fld[i].p, src[i], n * sizeof(double), hipMemcpyHostToDevice, s));
    PTV_TRY(c->mask.ensure(n));
    PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, n, hipMemcpyHostToDevice, s));
    return PTV_OK;
}

int ptv_clean_variational_dev(ptv_ctx *c, const ptv_variational_params *prm, const double *U, const double *V,
                              const double *W, double *Uo, double *Vo, double *Wo, void *stream,
                              ptv_variational_stats *st) {
    VarGrid g{};
    PTV_TRY(var_check(c, prm, g));
    if (!U || !V || !W || !Uo || !Vo || !Wo) {
        set_error("variational: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const VarSolve sv{prm->lambda_reg, prm->rtol, prm->maxiter};
    return variational_run(c->var, g, sv, prm->fluid_mask, U, V, W, Uo, Vo, Wo, s, st);
}

int ptv_clean_variational(ptv_ctx *c, const ptv_variational_params *prm, const double *U, const double *V,
                          const double *W, double *Uo, double *Vo, double *Wo, ptv_variational_stats *st) {
    VarGrid g{};
    PTV_TRY(var_check(c, prm, g));
    if (!U || !V || !W || !Uo || !Vo || !Wo) {
        set_error("variational: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[3] = {U, V, W};
    PTV_TRY(var_upload(c, prm, src, 3, 3, s));
    const VarSolve sv{prm->lambda_reg, prm->rtol, prm->maxiter};
    double *d[3] = {c->var_fld[0].p, c->var_fld[1].p, c->var_fld[2].p};
    PTV_TRY(variational_run(c->var, g, sv, c->mask.p, d[0], d[1], d[2], d[0], d[1], d[2], s, st));
    const size_t nbytes = (size_t)(prm->nx * prm->ny * prm->nz) * sizeof(double);
    double *dst[3] = {Uo, Vo, Wo};
    for (int i = 0; i < 3; ++i) PTV_HIP(hipMemcpyAsync(dst[i], d[i], nbytes, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_divergence_operator_apply(ptv_ctx *c, const ptv_variational_params *prm, const double *xu, const double *xv,
                                  const double *xw, double *d_grid) {
    VarGrid g{};
    PTV_TRY(var_check(c, prm, g));
    if (!xu || !xv || !xw || !d_grid) {
        set_error("divergence_operator_apply: NULL input or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[3] = {xu, xv, xw};
    PTV_TRY(var_upload(c, prm, src, 3, 4, s));
    PTV_TRY(launch_var_divergence(g, c->mask.p, c->var_fld[0].p, c->var_fld[1].p, c->var_fld[2].p, c->var_fld[3].p, s));
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_HIP(hipMemcpyAsync(d_grid, c->var_fld[3].p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_variational_apply(ptv_ctx *c, const ptv_variational_params *prm, const double *xu, const double *xv,
                          const double *xw, double *yu, double *yv, double *yw) {
    VarGrid g{};
    PTV_TRY(var_check(c, prm, g));
    if (!xu || !xv || !xw || !yu || !yv || !yw) {
        set_error("variational_apply: NULL input or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const double *src[3] = {xu, xv, xw};
    PTV_TRY(var_upload(c, prm, src, 3, 6, s));
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_TRY(c->var.d.ensure(n));
    double *f[6];
    for (int i = 0; i < 6; ++i) f[i] = c->var_fld[i].p;
    PTV_TRY(launch_var_divergence(g, c->mask.p, f[0], f[1], f[2], c->var.d.p, s));
    PTV_TRY(launch_var_adjoint(g, prm->lambda_reg, c->mask.p, c->var.d.p, f[0], f[1], f[2], f[3], f[4], f[5],
                               c->var.part, s));
    double *dst[3] = {yu, yv, yw};
    for (int i = 0; i < 3; ++i) PTV_HIP(hipMemcpyAsync(dst[i], f[3 + i], n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

// ---- pressure recovery (ptv_pressure.hip; the LSQR solve is ptv_clean.hip's) ----
// every argument check of the family, before any copy or launch
static int press_check(ptv_ctx *c, const ptv_pressure_params *prm, PressGrid &g) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (!prm->fluid_mask) {
        set_error("pressure: the fluid mask is required");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30) || prm->nx * prm->ny * prm->nz > 0x7fff0000LL) {
        set_error("pressure: dimensions must be positive, with fewer than 2^31 voxels");
        return PTV_E_ARG;
    }
    for (double h : {prm->dx, prm->dy, prm->dz}) {
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("pressure: spacings must be positive finite numbers");
            return PTV_E_ARG;
        }
    }
    if (!std::isfinite(prm->mu) || !std::isfinite(prm->rho)) {
        set_error("pressure: mu and rho must be finite");
        return PTV_E_ARG;
    }
    if (prm->wall_bc != PTV_WALL_ZERO_NEUMANN && prm->wall_bc != PTV_WALL_INHOMOGENEOUS) {
        set_error("pressure: wall_bc must be PTV_WALL_ZERO_NEUMANN or PTV_WALL_INHOMOGENEOUS");
        return PTV_E_ARG;
    }
    if (prm->anchor < PTV_ANCHOR_NONE || prm->anchor > PTV_ANCHOR_INLET || prm->flow_direction < -1 ||
        prm->flow_direction > 1) {
        set_error("pressure: anchor must be PTV_ANCHOR_* and flow_direction -1, 0 or 1");
        return PTV_E_ARG;
    }
    if (!std::isfinite(prm->rtol) || prm->maxiter < 0 || prm->lsqr_iter_lim < 0 || !(prm->lsqr_damp >= 0.0) ||
        !(prm->lsqr_atol >= 0.0) || !(prm->lsqr_btol >= 0.0)) {
        set_error("pressure: rtol must be finite; maxiter and the LSQR settings non-negative");
        return PTV_E_ARG;
    }
    g.nx = (int)prm->nx;
    g.ny = (int)prm->ny;
    g.nz = (int)prm->nz;
    g.dx = prm->dx;
    g.dy = prm->dy;
    g.dz = prm->dz;
    return PTV_OK;
}

static int press_rho_check(const ptv_pressure_params *prm) {
    if (prm->rho > 0.0 && (prm->nx < 2 || prm->ny < 2 || prm->nz < 2)) {
        set_error("pressure: rho > 0 needs at least 2 voxels along every axis (np.gradient)");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// CG with a Dirichlet grid, LSQR without one; all pointers device memory
static int press_solve(ptv_ctx *c, const ptv_pressure_params *prm, const PressGrid &g, const uint8_t *M,
                       const double *rhs, const uint8_t *Dir, double *X, hipStream_t s, ptv_pressure_stats &out) {
    if (Dir) return press_cg(c->press, g, prm->rtol, prm->maxiter, M, Dir, rhs, X, s, &out);
    const CleanGrid cg{g.nx, g.ny, g.nz, g.dx, g.dy, g.dz};
    const CleanSolve sv{0, prm->lsqr_damp, prm->lsqr_atol, prm->lsqr_btol, prm->lsqr_iter_lim};
    CleanRhsResult r{};
    PTV_TRY(clean_solve_rhs(c->clean, cg, sv, M, rhs, X, s, &r));
    out.solver = 1;
    out.n_fluid = r.n_fluid;
    out.n_dirichlet = 0;
    out.itn = r.itn;
    out.info = r.istop;
    out.bnorm = r.bnorm;
    out.rnorm = r.rnorm;
    out.ms_solve = r.ms_solve;
    out.ms_iter_median = r.ms_iter_median;
    return PTV_OK;
}

static size_t press_n(const ptv_pressure_params *prm) { return (size_t)(prm->nx * prm->ny * prm->nz); }

// host grids -> c->press_fld[first + i], the mask -> c->mask
static int press_upload(ptv_ctx *c, const ptv_pressure_params *prm, const double *const *src, int nf, int first,
                        hipStream_t s) {
    const size_t n = press_n(prm);
    for (int i = 0; i < nf; ++i) {
        PTV_TRY(c->press_fld[first + i].ensure(n));
        PTV_HIP(hipMemcpyAsync(c->press_fld[first + i].p, src[i], n * sizeof(double), hipMemcpyHostToDevice, s));
    }
    PTV_TRY(c->mask.ensure(n));
    PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, n, hipMemcpyHostToDevice, s));
    return PTV_OK;
}

int ptv_force_field_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                        double *Fx, double *Fy, double *Fz, void *stream, ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    if (!U || !V || !W || !Fx || !Fy || !Fz) {
        set_error("force_field: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(press_force(c->press, g, prm->mu, prm->rho, prm->fluid_mask, U, V, W, Fx, Fy, Fz, s, &out));
    out.ms_total = out.ms_force;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_force_field(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V, const double *W,
                    double *Fx, double *Fy, double *Fz, ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    if (!U || !V || !W || !Fx || !Fy || !Fz) {
        set_error("force_field: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = press_n(prm);
    const double *src[3] = {U, V, W};
    PTV_TRY(press_upload(c, prm, src, 3, 0, s));
    for (int i = 3; i < 6; ++i) PTV_TRY(c->press_fld[i].ensure(n));
    ptv_pressure_params dp = *prm;
    dp.fluid_mask = c->mask.p;
    PTV_TRY(ptv_force_field_dev(c, &dp, c->press_fld[0].p, c->press_fld[1].p, c->press_fld[2].p, c->press_fld[3].p,
                                c->press_fld[4].p, c->press_fld[5].p, s, st));
    double *dst[3] = {Fx, Fy, Fz};
    for (int i = 0; i < 3; ++i)
        PTV_HIP(hipMemcpyAsync(dst[i], c->press_fld[3 + i].p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_force_divergence_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                             const double *Fz, double *D, void *stream) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    if (!Fx || !Fy || !Fz || !D) {
        set_error("force_divergence: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, prm->fluid_mask, Fx, Fy, Fz, D, s);
}

int ptv_force_divergence(ptv_ctx *c, const ptv_pressure_params *prm, const double *Fx, const double *Fy,
                         const double *Fz, double *D) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    if (!Fx || !Fy || !Fz || !D) {
        set_error("force_divergence: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = press_n(prm);
    const double *src[3] = {Fx, Fy, Fz};
    PTV_TRY(press_upload(c, prm, src, 3, 3, s));
    PTV_TRY(c->press_fld[6].ensure(n));
    PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, c->mask.p, c->press_fld[3].p,
                             c->press_fld[4].p, c->press_fld[5].p, c->press_fld[6].p, s));
    PTV_HIP(hipMemcpyAsync(D, c->press_fld[6].p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_poisson_solve_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                          const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X, void *stream,
                          ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    if (!X || (!rhs && (!Fx || !Fy || !Fz))) {
        set_error("poisson_solve: NULL output, or neither a right-hand side nor a force field");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(c->ev_press[0].record(s));
    if (!rhs) {
        PTV_TRY(c->press.rhs.ensure(press_n(prm)));
        PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, prm->fluid_mask, Fx, Fy, Fz,
                                 c->press.rhs.p, s));
        rhs = c->press.rhs.p;
    }
    PTV_TRY(press_solve(c, prm, g, prm->fluid_mask, rhs, dirichlet, X, s, out));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_poisson_solve(ptv_ctx *c, const ptv_pressure_params *prm, const double *rhs, const double *Fx,
                      const double *Fy, const double *Fz, const uint8_t *dirichlet, double *X,
                      ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    if (!X || (!rhs && (!Fx || !Fy || !Fz))) {
        set_error("poisson_solve: NULL output, or neither a right-hand side nor a force field");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = press_n(prm);
    const double *src[3] = {Fx, Fy, Fz};
    if (rhs) {
        src[0] = rhs;
        PTV_TRY(press_upload(c, prm, src, 1, 6, s));
    } else {
        PTV_TRY(press_upload(c, prm, src, 3, 3, s));
        PTV_TRY(c->press_fld[6].ensure(n));
    }
    if (dirichlet) {
        PTV_TRY(c->press_dir.ensure(n));
        PTV_HIP(hipMemcpyAsync(c->press_dir.p, dirichlet, n, hipMemcpyHostToDevice, s));
    }
    ptv_pressure_params dp = *prm;
    dp.fluid_mask = c->mask.p;
    double *x = c->press_fld[6].p;
    PTV_TRY(ptv_poisson_solve_dev(c, &dp, rhs ? x : nullptr, c->press_fld[3].p, c->press_fld[4].p, c->press_fld[5].p,
                                  dirichlet ? c->press_dir.p : nullptr, x, s, st));
    PTV_HIP(hipMemcpyAsync(X, x, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_pressure_recover_dev(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                             const double *W, double *P, void *stream, ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    if (!U || !V || !W || !P) {
        set_error("pressure_recover: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = press_n(prm);
    PTV_TRY(c->press.f.ensure(3 * n));
    PTV_TRY(c->press.rhs.ensure(n));
    PTV_TRY(c->press.dir.ensure(n));
    double *F = c->press.f.p;
    const uint8_t *M = prm->fluid_mask;
    ptv_pressure_stats out{};
    out.anchor_plane = -1;
    PTV_TRY(c->ev_press[0].record(s));
    PTV_TRY(press_force(c->press, g, prm->mu, prm->rho, M, U, V, W, F, F + n, F + 2 * n, s, &out));
    if (out.n_fluid == 0) {  // physics.py:274-276
        PTV_HIP(hipMemsetAsync(P, 0, n * sizeof(double), s));
        PTV_HIP(hipStreamSynchronize(s));
        if (st) *st = out;
        return PTV_OK;
    }
    PTV_TRY(c->ev_press[1].record(s));
    PTV_TRY(press_divergence(g, prm->wall_bc == PTV_WALL_INHOMOGENEOUS, M, F, F + n, F + 2 * n, c->press.rhs.p, s));
    PTV_TRY(c->ev_press[2].record(s));
    const uint8_t *Dir = nullptr;
    if (prm->anchor != PTV_ANCHOR_NONE) {
        // velocity_analysis.py:304-321: np.mean(w[mask]) >= 0 has the sign of the sum
        const bool positive = prm->flow_direction == 1 || (prm->flow_direction == 0 && out.sum_w >= 0.0);
        const bool last = (prm->anchor == PTV_ANCHOR_OUTLET) == positive;
        out.anchor_plane = last ? g.nz - 1 : 0;
        PTV_TRY(press_anchor_plane(g, out.anchor_plane, M, c->press.dir.p, s));
        Dir = c->press.dir.p;
    }
    PTV_TRY(press_solve(c, prm, g, M, c->press.rhs.p, Dir, P, s, out));
    PTV_TRY(c->ev_press[3].record(s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[1], c->ev_press[2]));
    out.ms_divergence = ms;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_press[0], c->ev_press[3]));
    out.ms_total = ms;
    if (st) *st = out;
    return PTV_OK;
}

int ptv_pressure_recover(ptv_ctx *c, const ptv_pressure_params *prm, const double *U, const double *V,
                         const double *W, double *P, ptv_pressure_stats *st) {
    PressGrid g{};
    PTV_TRY(press_check(c, prm, g));
    PTV_TRY(press_rho_check(prm));
    if (!U || !V || !W || !P) {
        set_error("pressure_recover: NULL field or output");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = press_n(prm);
    const double *src[3] = {U, V, W};
    PTV_TRY(press_upload(c, prm, src, 3, 0, s));
    PTV_TRY(c->press_fld[6].ensure(n));
    ptv_pressure_params dp = *prm;
    dp.fluid_mask = c->mask.p;
    PTV_TRY(ptv_pressure_recover_dev(c, &dp, c->press_fld[0].p, c->press_fld[1].p, c->press_fld[2].p,
                                     c->press_fld[6].p, s, st));
    PTV_HIP(hipMemcpyAsync(P, c->press_fld[6].p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

// ---- flow analysis (ptv_flow.hip) ----
// ptv_flow_params -> FlowArgs, with the same checks for the host and device calls; the elementwise
// mode (stencil = false) reads neither the slab nor the spacings.
static int flow_args(ptv_ctx *c, const ptv_flow_params *prm, bool stencil, FlowArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("flow analysis: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    const int64_t least = stencil ? 2 : 1, most = 1 << 30;
    if (prm->nx < least || prm->ny < least || prm->nz < least) {
        set_error(stencil ? "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                            "elements are required."
                          : "flow derived: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->nx > most || prm->ny > most || prm->nz > most ||
        (double)prm->nx * (double)prm->ny * (double)prm->nz >= 1099511627776.0) {
        set_error("flow analysis: fewer than 2^40 voxels, at most 2^30 per axis");
        return PTV_E_ARG;
    }
    a = FlowArgs{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.strong = prm->spacing_strong ? 1 : 0;
    a.viscosity = prm->viscosity;
    if (stencil) {
        const int64_t lo = prm->edge_lo ? 0 : 1, hi = prm->nz - (prm->edge_hi ? 0 : 1);
        if (prm->z_begin < lo || prm->z_end > hi || prm->z_begin > prm->z_end) {
            set_error("flow analysis: planes [" + std::to_string(prm->z_begin) + ", " + std::to_string(prm->z_end) +
                      ") must lie in [" + std::to_string(lo) + ", " + std::to_string(hi) +
                      ") (a non-edge buffer end is a halo plane)");
            return PTV_E_ARG;
        }
        for (double h : {prm->dx, prm->dy, prm->dz})
            if (!(h > 0.0) || !std::isfinite(h)) {
                set_error("flow analysis: spacings must be positive and finite");
                return PTV_E_ARG;
            }
        a.z_begin = (int)prm->z_begin;
        a.z_end = (int)prm->z_end;
        a.edge_lo = prm->edge_lo ? 1 : 0;
        a.edge_hi = prm->edge_hi ? 1 : 0;
        a.dx = prm->dx;
        a.dy = prm->dy;
        a.dz = prm->dz;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

// the reduced rows -> ptv_flow_stats (synchronises `s`)
static int flow_finish(ptv_ctx *c, unsigned want, int64_t nvox, hipStream_t s, ptv_flow_stats *st) {
    double h[kFlowRows];
    PTV_HIP(hipMemcpyAsync(h, c->flow_res.p, sizeof(h), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, c->ev_flow0, c->ev_flow1));
    if (!st) return PTV_OK;
    *st = ptv_flow_stats{};
    st->n_voxels = nvox;
    st->n_fluid = (int64_t)h[15];
    st->sum_u = h[0];
    st->sum_v = h[1];
    st->sum_w = h[2];
    for (int k = 0; k < 4; ++k) {
        if (!(want >> k & 1)) continue;
        st->sum[k] = st->sum_fluid[k] = h[3 + 3 * k];
        st->max[k] = h[4 + 3 * k];
        st->min[k] = h[5 + 3 * k];
    }
    st->ms_stencil = ms;
    return PTV_OK;
}

static int run_flow(ptv_ctx *c, const FlowArgs &a, const void *U, const void *V, const void *W, const uint8_t *M,
                    void *const out[4], hipStream_t s) {
    PTV_TRY(c->flow_part.ensure(flow_partials(a)));
    PTV_TRY(c->flow_res.ensure(kFlowRows));
    PTV_TRY(c->ev_flow0.record(s));
    PTV_TRY(launch_flow(a, U, V, W, M, out, c->flow_part.p, c->flow_res.p, s));
    PTV_TRY(c->ev_flow1.record(s));
    return PTV_OK;
}

static unsigned flow_want(void *const out[4]) {
    return (out[0] ? 1u : 0u) | (out[1] ? 2u : 0u) | (out[2] ? 4u : 0u) | (out[3] ? 8u : 0u);
}

int ptv_flow_analysis_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                          void *strain, void *dissipation, void *vorticity, void *flow_type, void *stream,
                          ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_args(c, prm, true, a));
    if (!U || !V || !W) {
        set_error("flow analysis: NULL field");
        return PTV_E_ARG;
    }
    if (st) *st = ptv_flow_stats{};
    if (a.z_end <= a.z_begin) return PTV_OK;
    void *const out[4] = {strain, dissipation, vorticity, flow_type};
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_flow(c, a, U, V, W, prm->fluid_mask, out, s));
    return flow_finish(c, flow_want(out), (prm->z_end - prm->z_begin) * prm->nx * prm->ny, s, st);
}

int ptv_flow_analysis(ptv_ctx *c, const ptv_flow_params *prm, const void *U, const void *V, const void *W,
                      void *strain, void *dissipation, void *vorticity, void *flow_type, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_args(c, prm, true, a));
    if (!U || !V || !W) {
        set_error("flow analysis: NULL field");
        return PTV_E_ARG;
    }
    if (st) *st = ptv_flow_stats{};
    if (a.z_end <= a.z_begin) return PTV_OK;
    hipStream_t s = c->stream;
    const size_t ts = a.field_f32 ? 4 : 8;
    const int64_t nfull = prm->nz * prm->nx * prm->ny;
    const int64_t nout = (prm->z_end - prm->z_begin) * prm->nx * prm->ny;
    const void *src[3] = {U, V, W};
    for (int i = 0; i < 3; ++i) {
        PTV_TRY(c->flow_fld[i].ensure(nfull * ts));
        PTV_HIP(hipMemcpyAsync(c->flow_fld[i].p, src[i], nfull * ts, hipMemcpyHostToDevice, s));
    }
    const uint8_t *M = nullptr;
    if (prm->fluid_mask) {
        PTV_TRY(c->mask.ensure(nfull));
        PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, nfull, hipMemcpyHostToDevice, s));
        M = c->mask.p;
    }
    void *const host[4] = {strain, dissipation, vorticity, flow_type};
    void *out[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        PTV_TRY(c->flow_out[k].ensure(nout * ts));
        out[k] = c->flow_out[k].p;
    }
    PTV_TRY(run_flow(c, a, c->flow_fld[0].p, c->flow_fld[1].p, c->flow_fld[2].p, M, out, s));
    for (int k = 0; k < 4; ++k)
        if (host[k]) PTV_HIP(hipMemcpyAsync(host[k], out[k], nout * ts, hipMemcpyDeviceToHost, s));
    return flow_finish(c, flow_want(out), nout, s, st);
}

int ptv_flow_derived_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                         void *dissipation, void *flow_type, void *stream, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_args(c, prm, false, a));
    if (!strain || (flow_type && !vorticity_mag)) {
        set_error("flow derived: NULL strain rate, or flow type without the vorticity magnitude");
        return PTV_E_ARG;
    }
    if (st) *st = ptv_flow_stats{};
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int64_t n = prm->nz * prm->nx * prm->ny;
    PTV_TRY(c->flow_part.ensure(flow_derived_partials(n)));
    PTV_TRY(c->flow_res.ensure(kFlowRows));
    PTV_TRY(c->ev_flow0.record(s));
    PTV_TRY(launch_flow_derived(a, n, strain, vorticity_mag, prm->fluid_mask, dissipation, flow_type, c->flow_part.p,
                                c->flow_res.p, s));
    PTV_TRY(c->ev_flow1.record(s));
    return flow_finish(c, (dissipation ? 2u : 0u) | (flow_type ? 8u : 0u), n, s, st);
}

int ptv_flow_derived(ptv_ctx *c, const ptv_flow_params *prm, const void *strain, const void *vorticity_mag,
                     void *dissipation, void *flow_type, ptv_flow_stats *st) {
    FlowArgs a{};
    PTV_TRY(flow_args(c, prm, false, a));
    if (!strain || (flow_type && !vorticity_mag)) {
        set_error("flow derived: NULL strain rate, or flow type without the vorticity magnitude");
        return PTV_E_ARG;
    }
    hipStream_t s = c->stream;
    const size_t ts = a.field_f32 ? 4 : 8;
    const int64_t n = prm->nz * prm->nx * prm->ny;
    const void *src[2] = {strain, flow_type ? vorticity_mag : nullptr};
    for (int i = 0; i < 2; ++i) {
        if (!src[i]) continue;
        PTV_TRY(c->flow_fld[i].ensure(n * ts));
        PTV_HIP(hipMemcpyAsync(c->flow_fld[i].p, src[i], n * ts, hipMemcpyHostToDevice, s));
    }
    ptv_flow_params dp = *prm;
    dp.fluid_mask = nullptr;
    if (prm->fluid_mask) {
        PTV_TRY(c->mask.ensure(n));
        PTV_HIP(hipMemcpyAsync(c->mask.p, prm->fluid_mask, n, hipMemcpyHostToDevice, s));
        dp.fluid_mask = c->mask.p;
    }
    void *const host[2] = {dissipation, flow_type};
    void *out[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        PTV_TRY(c->flow_out[k].ensure(n * ts));
        out[k] = c->flow_out[k].p;
    }
    PTV_TRY(ptv_flow_derived_dev(c, &dp, c->flow_fld[0].p, src[1] ? c->flow_fld[1].p : nullptr, out[0], out[1], s, st));
    for (int k = 0; k < 2; ++k)
        if (host[k]) PTV_HIP(hipMemcpy(host[k], out[k], n * ts, hipMemcpyDeviceToHost));
    return PTV_OK;
}

// ---- interface drag and gradient sums (ptv_drag.hip) ----
static int drag_dims(int64_t nx, int64_t ny, int64_t nz, int64_t least, const char *what) {
    const int64_t most = 1 << 30;
    if (nx < least || ny < least || nz < least) {
        set_error(least == 2 ? "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                               "elements are required."
                             : std::string(what) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    if (nx > most || ny > most || nz > most || (double)nx * (double)ny * (double)nz >= 1099511627776.0) {
        set_error(std::string(what) + ": fewer than 2^40 voxels, at most 2^30 per axis");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

// ptv_drag_params -> DragArgs, with the same checks for the host and device calls
static int drag_args(ptv_ctx *c, const ptv_drag_params *prm, DragArgs &a) {
    if (!c || !prm) {
        set_error("NULL context/params");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("interface drag: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    PTV_TRY(drag_dims(prm->nx, prm->ny, prm->nz, 1, "interface drag"));
    for (double h : {prm->dx, prm->dy, prm->dz})
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("interface drag: spacings must be positive and finite");
            return PTV_E_ARG;
        }
    if (!std::isfinite(prm->viscosity)) {
        set_error("interface drag: viscosity must be finite");
        return PTV_E_ARG;
    }
    if (prm->n_labels < 1 || !prm->labels) {
        set_error("interface drag: at least one label");
        return PTV_E_ARG;
    }
    for (int i = 0; i < prm->n_labels; ++i)
        if (prm->labels[i] <= 0 || (i > 0 && prm->labels[i] <= prm->labels[i - 1])) {
            set_error("interface drag: labels must be positive and strictly ascending");
            return PTV_E_ARG;
        }
    a = DragArgs{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.area[0] = prm->dy * prm->dx;
    a.area[1] = prm->dz * prm->dx;
    a.area[2] = prm->dz * prm->dy;
    a.step[0] = prm->dz;
    a.step[1] = prm->dy;
    a.step[2] = prm->dx;
    a.viscosity = prm->viscosity;
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int ptv_interface_drag_dev(ptv_ctx *c, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
                           const void *W, const void *P, void *stream, ptv_drag_stats *records, double *ms) {
    DragArgs a{};
    PTV_TRY(drag_args(c, prm, a));
    if (!mask || !U || !V || !W || !records) {
        set_error("interface drag: NULL mask, field or records");
        return PTV_E_ARG;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int nl = prm->n_labels;
    const size_t nrows = (size_t)nl * kDragSlotRows;
    PTV_TRY(c->drag_part.ensure(drag_partials(a, nl)));
    PTV_TRY(c->drag_res.ensure(nrows));
    PTV_TRY(c->drag_labels.ensure((size_t)nl));
    PTV_HIP(hipMemcpyAsync(c->drag_labels.p, prm->labels, (size_t)nl * sizeof(int), hipMemcpyHostToDevice, s));
    PTV_TRY(c->ev_drag0.record(s));
    PTV_TRY(launch_drag(a, mask, U, V, W, P, c->drag_labels.p, nl, c->drag_part.p, c->drag_res.p, s));
    PTV_TRY(c->ev_drag1.record(s));
    std::vector<double> h(nrows);
    PTV_HIP(hipMemcpyAsync(h.data(), c->drag_res.p, nrows * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    float t = 0.f;
    PTV_HIP(hipEventElapsedTime(&t, c->ev_drag0, c->ev_drag1));
    if (ms) *ms = t;
    for (size_t r = 0; r < (size_t)nl * 6; ++r) {
        const double *v = h.data() + r * kDragVals;
        records[r] = ptv_drag_stats{(int64_t)v[0], v[1], v[2], v[3], v[4]};  // a count is an exact integer
    }
    return PTV_OK;
}

int ptv_interface_drag(ptv_ctx *c, const ptv_drag_params *prm, const int32_t *mask, const void *U, const void *V,
                       const void *W, const void *P, ptv_drag_stats *records, double *ms) {
    DragArgs a{};
    PTV_TRY(drag_args(c, prm, a));
    if (!mask || !U || !V || !W || !records) {
        set_error("interface drag: NULL mask, field or records");
        return PTV_E_ARG;
    }
    hipStream_t s = c->stream;
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz), ts = a.field_f32 ? 4 : 8;
    PTV_TRY(c->drag_mask.ensure(n));
    PTV_HIP(hipMemcpyAsync(c->drag_mask.p, mask, n * sizeof(int), hipMemcpyHostToDevice, s));
    const void *src[4] = {U, V, W, P};
    for (int i = 0; i < 4; ++i) {
        if (!src[i]) continue;
        PTV_TRY(c->drag_fld[i].ensure(n * ts));
        PTV_HIP(hipMemcpyAsync(c->drag_fld[i].p, src[i], n * ts, hipMemcpyHostToDevice, s));
    }
    return ptv_interface_drag_dev(c, prm, c->drag_mask.p, c->drag_fld[0].p, c->drag_fld[1].p, c->drag_fld[2].p,
                                  P ? c->drag_fld[3].p : nullptr, s, records, ms);
}

int ptv_gradient_sums_dev(ptv_ctx *c, const ptv_flow_params *prm, const void *P, void *stream, double sums3[3]) {
    if (!c || !prm || !P || !sums3) {
        set_error("gradient sums: NULL argument");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("gradient sums: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    PTV_TRY(drag_dims(prm->nx, prm->ny, prm->nz, 2, "gradient sums"));
    if (prm->z_begin != 0 || prm->z_end != prm->nz || !prm->edge_lo || !prm->edge_hi) {
        set_error("gradient sums: the plane range must be the whole buffer");
        return PTV_E_UNSUPPORTED;
    }
    for (double h : {prm->dx, prm->dy, prm->dz})
        if (!(h > 0.0) || !std::isfinite(h)) {
            set_error("gradient sums: spacings must be positive and finite");
            return PTV_E_ARG;
        }
    DragArgs a{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.field_f32 = prm->field_dtype == PTV_F32;
    a.strong = prm->spacing_strong ? 1 : 0;
    a.step[0] = prm->dz;
    a.step[1] = prm->dy;
    a.step[2] = prm->dx;
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(c->drag_part.ensure(drag_partials(a, 0)));
    PTV_TRY(c->drag_res.ensure(3));
    PTV_TRY(c->ev_drag0.record(s));
    PTV_TRY(launch_gradient_sums(a, P, c->drag_part.p, c->drag_res.p, s));
    PTV_TRY(c->ev_drag1.record(s));
    PTV_HIP(hipMemcpyAsync(sums3, c->drag_res.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_gradient_sums(ptv_ctx *c, const ptv_flow_params *prm, const void *P, double sums3[3]) {
    if (!c || !prm || !P || !sums3) {
        set_error("gradient sums: NULL argument");
        return PTV_E_ARG;
    }
    if (prm->field_dtype != PTV_F64 && prm->field_dtype != PTV_F32) {
        set_error("gradient sums: field_dtype must be PTV_F64 or PTV_F32");
        return PTV_E_ARG;
    }
    PTV_TRY(drag_dims(prm->nx, prm->ny, prm->nz, 2, "gradient sums"));
    PTV_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)(prm->nx * prm->ny * prm->nz) * (prm->field_dtype == PTV_F32 ? 4 : 8);
    PTV_TRY(c->drag_fld[3].ensure(bytes));
    PTV_HIP(hipMemcpyAsync(c->drag_fld[3].p, P, bytes, hipMemcpyHostToDevice, c->stream));
    return ptv_gradient_sums_dev(c, prm, c->drag_fld[3].p, c->stream, sums3);
}

// ---- distance transform and alignment score (ptv_edt.hip) ----
// the dimensions a uint32 squared distance can hold; decided before any allocation or copy
static int edt_dims(int64_t nx, int64_t ny, int64_t nz, const char *what) {
    if (nx < 1 || ny < 1 || nz < 1) {
        set_error(std::string(what) + ": dimensions must be positive");
        return PTV_E_ARG;
    }
    const int64_t most = 46340;  // floor(sqrt(2^31 - 1)): keeps the squares below from overflowing
    if (nx > most || ny > most || nz > most || nx * nx + ny * ny + nz * nz >= ((int64_t)1 << 31)) {
        set_error(std::string(what) + ": nz^2 + ny^2 + nx^2 must be below 2^31 (squared distances are 32-bit)");
        return PTV_E_UNSUPPORTED;
    }
    return PTV_OK;
}

int ptv_edt_dev(ptv_ctx *c, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist, void *stream,
                ptv_edt_stats *st) {
    if (!c || !prm || !mask) {
        set_error("distance transform: NULL context, params or mask");
        return PTV_E_ARG;
    }
    PTV_TRY(edt_dims(prm->nx, prm->ny, prm->nz, "distance transform"));
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_TRY(c->edt_a.ensure(n));
    PTV_TRY(c->edt_b.ensure(n));
    PTV_TRY(c->edt_max.ensure(1));
    double *kept = nullptr;
    if (prm->keep_distance) {
        c->align_dt_dims[0] = 0;  // nothing valid until this call has succeeded
        PTV_TRY(c->align_dt.ensure(n));
        kept = c->align_dt.p;
    }
    PTV_TRY(c->ev_edt0.record(s));
    // with both a caller's field and a kept one, the kernel writes the kept one and a copy follows
    PTV_TRY(launch_edt((int)prm->nx, (int)prm->ny, (int)prm->nz, mask, c->edt_a.p, c->edt_b.p, d2, kept ? kept : dist,
                       c->edt_max.p, s));
    if (kept && dist) PTV_HIP(hipMemcpyAsync(dist, kept, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    PTV_TRY(c->ev_edt1.record(s));
    unsigned top = 0;
    PTV_HIP(hipMemcpyAsync(&top, c->edt_max.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (top >= 0x80000000u) {
        set_error("distance transform: the mask has no zero voxel");
        return PTV_E_ARG;
    }
    if (kept) {
        c->align_dt_dims[0] = prm->nx;
        c->align_dt_dims[1] = prm->ny;
        c->align_dt_dims[2] = prm->nz;
    }
    if (st) {
        float t = 0.f;
        PTV_HIP(hipEventElapsedTime(&t, c->ev_edt0, c->ev_edt1));
        st->max_d2 = (int64_t)top;
        st->ms = t;
    }
    return PTV_OK;
}

int ptv_edt(ptv_ctx *c, const ptv_edt_params *prm, const uint8_t *mask, int32_t *d2, double *dist, ptv_edt_stats *st) {
    if (!c || !prm || !mask) {
        set_error("distance transform: NULL context, params or mask");
        return PTV_E_ARG;
    }
    PTV_TRY(edt_dims(prm->nx, prm->ny, prm->nz, "distance transform"));
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
    PTV_TRY(c->edt_mask.ensure(n));
    if (d2) PTV_TRY(c->edt_d2.ensure(n));
    // the float64 field of a host call lives in the context's resident buffer, kept or not
    ptv_edt_params q = *prm;
    const bool kept = prm->keep_distance != 0;
    if (dist) q.keep_distance = 1;
    PTV_HIP(hipMemcpyAsync(c->edt_mask.p, mask, n, hipMemcpyHostToDevice, s));
    const int rc = ptv_edt_dev(c, &q, c->edt_mask.p, d2 ? c->edt_d2.p : nullptr, nullptr, s, st);
    if (!kept) c->align_dt_dims[0] = 0;
    PTV_TRY(rc);
    if (d2) PTV_HIP(hipMemcpyAsync(d2, c->edt_d2.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (dist) PTV_HIP(hipMemcpyAsync(dist, c->align_dt.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

static int align_check(ptv_ctx *c, const ptv_align_params *prm, const double *offsets, ptv_align_record *records) {
    if (!c || !prm || !offsets || !records) {
        set_error("alignment score: NULL context, params, offsets or records");
        return PTV_E_ARG;
    }
    PTV_TRY(edt_dims(prm->nx, prm->ny, prm->nz, "alignment score"));
    if (prm->n_points < 0 || prm->n_points >= ((int64_t)1 << 31)) {
        set_error("alignment score: 0 <= n_points < 2^31");
        return PTV_E_ARG;
    }
    if (prm->n_offsets < 1) {
        set_error("alignment score: at least one offset");
        return PTV_E_ARG;
    }
    return PTV_OK;
}

int ptv_align_score_dev(ptv_ctx *c, const ptv_align_params *prm, const double *points, const double *dt,
                        const double *offsets, void *stream, ptv_align_record *records, double *ms) {
    PTV_TRY(align_check(c, prm, offsets, records));
    if (!dt || (!points && prm->n_points > 0)) {
        set_error("alignment score: NULL points or distance field");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    AlignArgs a{};
    a.nx = (int)prm->nx;
    a.ny = (int)prm->ny;
    a.nz = (int)prm->nz;
    a.n = prm->n_points;
    align_tile(a);
    const int chunk = 4096;  // offsets per launch (a grid's y extent is 16-bit)
    const int m = prm->n_offsets, mc = std::min(m, chunk);
    PTV_TRY(c->align_off.ensure((size_t)m * 3));
    PTV_TRY(c->align_rec.ensure((size_t)m));
    PTV_TRY(c->align_psum.ensure((size_t)mc * a.nblocks));
    PTV_TRY(c->align_pcnt.ensure((size_t)mc * a.nblocks));
    PTV_HIP(hipMemcpyAsync(c->align_off.p, offsets, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    PTV_TRY(c->ev_edt0.record(s));
    for (int o0 = 0; o0 < m; o0 += chunk)
        PTV_TRY(launch_align_score(a, points, dt, c->align_off.p + (size_t)o0 * 3, std::min(chunk, m - o0),
                                   c->align_psum.p, c->align_pcnt.p, c->align_rec.p + o0, s));
    PTV_TRY(c->ev_edt1.record(s));
    PTV_HIP(hipMemcpyAsync(records, c->align_rec.p, (size_t)m * sizeof(ptv_align_record), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (ms) {
        float t = 0.f;
        PTV_HIP(hipEventElapsedTime(&t, c->ev_edt0, c->ev_edt1));
        *ms = t;
    }
    return PTV_OK;
}

int ptv_align_score(ptv_ctx *c, const ptv_align_params *prm, const double *points, const double *dt,
                    const double *offsets, ptv_align_record *records, double *ms) {
    PTV_TRY(align_check(c, prm, offsets, records));
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (dt) {
        const size_t n = (size_t)(prm->nx * prm->ny * prm->nz);
        c->align_dt_dims[0] = 0;
        PTV_TRY(c->align_dt.ensure(n));
        PTV_HIP(hipMemcpyAsync(c->align_dt.p, dt, n * sizeof(double), hipMemcpyHostToDevice, s));
        c->align_dt_dims[0] = prm->nx;
        c->align_dt_dims[1] = prm->ny;
        c->align_dt_dims[2] = prm->nz;
    } else if (c->align_dt_dims[0] != prm->nx || c->align_dt_dims[1] != prm->ny || c->align_dt_dims[2] != prm->nz) {
        set_error("alignment score: dt is NULL and the context holds no distance field of these dimensions");
        return PTV_E_ARG;
    }
    if (points) {
        c->align_pts_n = -1;
        PTV_TRY(c->align_pts.ensure((size_t)prm->n_points * 3));
        PTV_HIP(hipMemcpyAsync(c->align_pts.p, points, (size_t)prm->n_points * 3 * sizeof(double),
                               hipMemcpyHostToDevice, s));
        c->align_pts_n = prm->n_points;
    } else if (c->align_pts_n != prm->n_points) {
        set_error("alignment score: points is NULL and the context holds no point set of this size");
        return PTV_E_ARG;
    }
    PTV_TRY(c->align_pts.ensure(1));  // zero points: still a pointer
    return ptv_align_score_dev(c, prm, c->align_pts.p, c->align_dt.p, offsets, s, records, ms);
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

// ---------------------------------------------------------------------------
// pore-mask path and outlier filter
// ---------------------------------------------------------------------------
namespace {

// raw axes -> device (ascending; a descending axis is reversed and flagged, as scipy's
// RegularGridInterpolator flips descending grids, _rgi.py _check_dimensionality/flip)
int mask_source(ptv_ctx *c, const ptv_mask_grid *src, MaskSampleLaunch &m, hipStream_t s) {
    if (!src || !src->raw || !src->ax || !src->ay || !src->az) {
        set_error("sample_mask: NULL raw mask or axis");
        return PTV_E_ARG;
    }
    const int64_t rn[3] = {src->nx, src->ny, src->nz};
    for (int d = 0; d < 3; ++d)
        if (rn[d] <= 0 || rn[d] > (1 << 30)) {
            set_error("sample_mask: raw mask extents must be positive");
            return PTV_E_ARG;
        }
    std::vector<double> h;
    h.reserve(rn[0] + rn[1] + rn[2]);
    const double *ax[3] = {src->ax, src->ay, src->az};
    size_t off[3];
    for (int d = 0; d < 3; ++d) {
        const double *a = ax[d];
        const int64_t n = rn[d];
        const bool desc = n > 1 && a[0] > a[n - 1];
        off[d] = h.size();
        for (int64_t i = 0; i < n; ++i) h.push_back(desc ? a[n - 1 - i] : a[i]);
        for (int64_t i = 1; i < n; ++i)
            if (!(h[off[d] + i] > h[off[d] + i - 1])) {
                set_error("The points in dimension " + std::to_string(2 - d) +
                          " must be strictly ascending or descending");
                return PTV_E_ARG;
            }
        m.rn[d] = (int)n;
        m.flip[d] = desc ? 1 : 0;
    }
    PTV_TRY(c->mask_axes.ensure(h.size()));
    PTV_HIP(hipMemcpyAsync(c->mask_axes.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
    for (int d = 0; d < 3; ++d) m.ra[d] = c->mask_axes.p + off[d];
    // the host vector must outlive the async copy
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int mask_grid_check(ptv_ctx *c, const ptv_grid *g, uint8_t *out) {
    if (!c) {
        set_error("NULL context");
        return PTV_E_ARG;
    }
    if (!g || !out) {
        set_error("sample_mask: NULL grid or output");
        return PTV_E_ARG;
    }
    if (g->nx <= 0 || g->ny <= 0 || g->nz <= 0 || g->nx > (1 << 30) || g->ny > (1 << 30) || g->nz > (1 << 30)) {
        set_error("grid: dimensions must be positive");
        return PTV_E_ARG;
    }
    const bool sep = g->ax && g->ay && g->az, pts = g->px && g->py && g->pz;
    if (!sep && !pts) {
        set_error("grid: give either the three axes or the three point arrays");
        return PTV_E_ARG;
    }
    if (g->z_begin < 0 || g->z_end > g->nz || g->z_begin > g->z_end) {
        set_error("grid: bad z slab");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

int run_mask_sample(ptv_ctx *c, MaskSampleLaunch &m, const ptv_grid *g, const uint8_t *raw, uint8_t *out,
                    hipStream_t s) {
    const Queries q = queries_of(g);
    m.raw = raw;
    m.nx = (int)g->nx;
    m.ny = (int)g->ny;
    m.nz = (int)g->nz;
    m.z0 = (int)g->z_begin;
    m.z1 = (int)g->z_end;
    PTV_TRY(c->mask_tabs.ensure(g->nx + g->ny + g->nz));
    return launch_mask_sample(m, q.ax, q.ay, q.az, q.qx, q.qy, q.qz, c->mask_tabs.p, out, s);
}

int boundary_check(ptv_ctx *c, const ptv_boundary_params *prm, int64_t *count, BoundaryLaunch &m) {
    if (!c || !prm || !prm->mask || !count) {
        set_error("boundary: NULL context, params, mask or count");
        return PTV_E_ARG;
    }
    if (prm->nx <= 0 || prm->ny <= 0 || prm->nz <= 0 || prm->nx > (1 << 30) || prm->ny > (1 << 30) ||
        prm->nz > (1 << 30)) {
        set_error("boundary: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->thickness < 1 || prm->sampling_step < 1 ||
        (prm->encoding != PTV_MASK_BOOL && prm->encoding != PTV_MASK_BITS)) {
        set_error("boundary: need thickness >= 1, sampling_step >= 1 and a known encoding");
        return PTV_E_ARG;
    }
    m.nx = (int)prm->nx;
    m.ny = (int)prm->ny;
    m.nz = (int)prm->nz;
    m.mask = prm->mask;
    m.is_bool = prm->encoding == PTV_MASK_BOOL;
    m.thickness = prm->thickness;
    m.step = prm->sampling_step;
    for (int d = 0; d < 3; ++d) {
        m.lo[d] = prm->lo[d];
        m.span[d] = prm->span[d];
        m.den[d] = prm->den[d];
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

// count pass (dilations + block counts + scan), then the emit pass into x, y, z if they fit
int run_boundary(ptv_ctx *c, const BoundaryLaunch &m, double *x, double *y, double *z, int64_t cap, int64_t *count,
                 hipStream_t s) {
    const int64_t nvox = (int64_t)m.nx * m.ny * m.nz;
    const size_t nb = boundary_blocks(nvox);
    PTV_TRY(c->bnd_counts.ensure(nb + 1));
    if (m.thickness > 1) {
        PTV_TRY(c->bnd_ping.ensure(nvox));
        if (m.thickness > 2) PTV_TRY(c->bnd_pong.ensure(nvox));
    }
    const uint8_t *grown = nullptr;
    PTV_TRY(c->ev_div0.record(s));
    PTV_TRY(launch_boundary_count(m, c->bnd_ping.p, c->bnd_pong.p, c->bnd_counts.p, &grown, s));
    unsigned long long total = 0;
    PTV_HIP(hipMemcpyAsync(&total, c->bnd_counts.p + nb, sizeof(total), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    const int64_t nsel = (int64_t)((total + (unsigned long long)m.step - 1) / (unsigned long long)m.step);
    *count = nsel;
    if (x && y && z && cap >= nsel && nsel > 0)
        PTV_TRY(launch_boundary_emit(m, grown, c->bnd_counts.p, x, y, z, s));
    PTV_TRY(c->ev_div1.record(s));
    c->div_pending = true;
    return PTV_OK;
}

int filter_check(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep) {
    if (!c || !p || !prm || !keep) {
        set_error("filter: NULL context, particles, params or keep");
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
    if (prm->k < 1) {
        set_error("filter: k must be >= 1");
        return PTV_E_ARG;
    }
    if (p->n <= prm->k) {
        set_error("filter: need more particles than k (the reference skips the filter)");
        return PTV_E_ARG;
    }
    PTV_HIP(hipSetDevice(c->device));
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_sample_mask_dev(ptv_ctx *c, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out, void *stream) {
    PTV_TRY(mask_grid_check(c, g, out));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    MaskSampleLaunch m{};
    PTV_TRY(mask_source(c, src, m, s));
    return run_mask_sample(c, m, g, src->raw, out, s);
}

int ptv_sample_mask(ptv_ctx *c, const ptv_mask_grid *src, const ptv_grid *g, uint8_t *out) {
    PTV_TRY(mask_grid_check(c, g, out));
    hipStream_t s = c->stream;
    MaskSampleLaunch m{};
    PTV_TRY(mask_source(c, src, m, s));
    const int64_t nraw = src->nx * src->ny * src->nz;
    PTV_TRY(c->mask_raw.ensure(nraw));
    PTV_HIP(hipMemcpyAsync(c->mask_raw.p, src->raw, nraw, hipMemcpyHostToDevice, s));
    ptv_grid dg;
    PTV_TRY(upload_grid(c, g, s, dg));
    const int64_t nout = (g->z_end - g->z_begin) * g->nx * g->ny;
    PTV_TRY(c->mask_out.ensure(nout));
    PTV_TRY(run_mask_sample(c, m, &dg, c->mask_raw.p, c->mask_out.p, s));
    PTV_HIP(hipMemcpyAsync(out, c->mask_out.p, nout, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_boundary_particles_dev(ptv_ctx *c, const ptv_boundary_params *prm, double *x, double *y, double *z,
                               int64_t cap, int64_t *count, void *stream) {
    BoundaryLaunch m{};
    PTV_TRY(boundary_check(c, prm, count, m));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_boundary(c, m, x, y, z, cap, count, s));
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_boundary_particles(ptv_ctx *c, const ptv_boundary_params *prm, double *x, double *y, double *z, int64_t cap,
                           int64_t *count) {
    BoundaryLaunch m{};
    PTV_TRY(boundary_check(c, prm, count, m));
    hipStream_t s = c->stream;
    const int64_t nvox = prm->nx * prm->ny * prm->nz;
    PTV_TRY(c->mask_raw.ensure(nvox));
    PTV_HIP(hipMemcpyAsync(c->mask_raw.p, prm->mask, nvox, hipMemcpyHostToDevice, s));
    m.mask = c->mask_raw.p;
    // size the device output from the count pass when the caller's buffers are large enough
    int64_t nsel = 0;
    PTV_TRY(run_boundary(c, m, nullptr, nullptr, nullptr, 0, &nsel, s));
    *count = nsel;
    if (x && y && z && cap >= nsel && nsel > 0) {
        PTV_TRY(c->bnd_xyz.ensure((size_t)3 * nsel));
        double *d = c->bnd_xyz.p;
        PTV_TRY(run_boundary(c, m, d, d + nsel, d + 2 * nsel, nsel, &nsel, s));
        PTV_HIP(hipMemcpyAsync(x, d, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipMemcpyAsync(y, d + nsel, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
        PTV_HIP(hipMemcpyAsync(z, d + 2 * nsel, nsel * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    PTV_HIP(hipStreamSynchronize(s));
    return PTV_OK;
}

int ptv_filter_outliers_knn_dev(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep,
                                double *kth_dist, void *stream, ptv_stats *st) {
    PTV_TRY(filter_check(c, p, prm, keep));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(run_filter(c, p, prm, keep, kth_dist, s));
    if (st) *st = c->last;
    return PTV_OK;
}

int ptv_filter_outliers_knn(ptv_ctx *c, const ptv_particles *p, const ptv_filter_params *prm, uint8_t *keep,
                            double *kth_dist, ptv_stats *st) {
    PTV_TRY(filter_check(c, p, prm, keep));
    hipStream_t s = c->stream;
    const int64_t n = p->n;
    ptv_particles dp;
    PTV_TRY(upload_particles(c, p, s, dp));
    PTV_TRY(c->flt_keep.ensure(n));
    PTV_TRY(c->flt_kth.ensure(n));
    PTV_TRY(run_filter(c, &dp, prm, c->flt_keep.p, c->flt_kth.p, s));
    PTV_HIP(hipMemcpyAsync(keep, c->flt_keep.p, n, hipMemcpyDeviceToHost, s));
    if (kth_dist) PTV_HIP(hipMemcpyAsync(kth_dist, c->flt_kth.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    PTV_TRY(finish_timing(c));
    if (st) *st = c->last;
    return PTV_OK;
}

}  // extern "C"
