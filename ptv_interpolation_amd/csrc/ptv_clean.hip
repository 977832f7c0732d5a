// ptv_clean.hip — projection-method divergence cleaning: matrix-free LSQR on the masked Laplacian.
//
// Restates physics.clean_divergence_projection (physics.py:149-209): per outer iteration the
// consistent divergence (ptv_div.hip), b = div[fluid] - mean(div[fluid]) (:182-183),
// scipy.sparse.linalg.lsqr(A, b, damp, atol, btol, iter_lim) (:186) on the Laplacian of
// build_laplacian_matrix (:55-108), and apply_consistent_correction (:110-147).
//
// Storage: every vector is a dense float64 (nz, ny, nx) grid, x fastest; the uint8 fluid mask is
// applied in the kernels.  Solid entries are never written (they stay the 0 of the initial memset)
// and are skipped by every sum, so the dense vectors are the reference's compact fluid vectors with
// zeros in between.  No compaction, no CSR: A is its 7-point stencil
//     (A x)_i = sum over fluid face neighbours j inside the domain of (x_j - x_i) * h_axis^-2,
// symmetric, so the same kernel serves A and A^T.
//
// One LSQR iteration (scipy _isolve/lsqr.py:424-572) is three streaming passes, each followed by a
// one-block kernel that sums the pass's per-block partials in a fixed order and advances the scalar
// recurrences on device-resident state:
//     k_bidiag(u):  u <- A v - alfa u,  sum u^2     ->  beta, anorm
//     k_bidiag(v):  v <- A u - beta v,  sum v^2     ->  alfa, the two plane rotations, t1, t2, rho
//     k_update:     x <- x + t1 w,  w <- v + t2 w,  sum (w/rho)^2  ->  ddnorm, the stopping tests
// u and v are stored un-normalised; every consumer multiplies by the 1/beta, 1/alfa of the state
// (the same product scipy's `u = (1/beta) * u` rounds once), which saves the scaling passes.
// Bytes per voxel and iteration: 2 x (8 read + 8 read + 8 write + 1 mask) + (3 x 8 read + 2 x 8
// write + 1 mask) = 91 (stencil neighbours come from the cache lines of adjacent lanes and rows).
//
// Reductions are two-stage and fixed-order (wave64 DPP sum, LDS across the block's 4 waves, then
// the one-block kernel over the partials): no floating-point atomics, so a call repeats bit for bit.
// The stop flag, the polling loop and the event numbering are those of ptv_grid_solve.hpp.
#include <cmath>
#include <algorithm>

#include "ptv_clean.hpp"
#include "ptv_grid_solve.hpp"

namespace ptv {

namespace {

// device-resident LSQR state (doubles; names follow scipy's lsqr)
enum {
    S_STOP = kStopSlot, S_ISTOP, S_ITN, S_ALFA, S_BETA, S_INV_ALFA, S_INV_BETA, S_RHOBAR, S_PHIBAR, S_ANORM,
    S_DDNORM, S_RES2, S_XNORM, S_XXNORM, S_Z, S_CS2, S_SN2, S_BNORM, S_RNORM, S_ARNORM, S_ACOND, S_T1,
    S_T2, S_INV_RHO, S_SKIPV, S_MEAN, S_MEANABS, S_NFLUID, S_NAN, S_COUNT
};
constexpr int kStateLen = 32;
static_assert(S_COUNT <= kStateLen, "state length");
// report slots: 0 initial flux, 1 final flux, 2 final mean |div|, 3.. mean |div| before solve i;
// the last slot takes the solves past PTV_CLEAN_MAX_OUTER, which the stats do not report
constexpr int kRepLen = 3 + PTV_CLEAN_MAX_OUTER + 1;

enum Phase { PH_DIVSTATS = 0, PH_INIT_BETA, PH_INIT_ALFA, PH_BETA, PH_ALFA, PH_TEST, PH_NAN };

struct CleanArgs : GridDims {
    double hx, hy, hz;   // 1.0 / (h ** 2) per axis (physics.py:68)
    double dx, dy, dz;
};

struct LsqrCfg {
    double damp, atol, btol, ctol;
    int iter_lim;
};

// (A (sc * X))_i for the VEC elements of a group, o.e[e] = 0 where the voxel is solid.  Neighbour
// offsets are clamped at the domain faces, so every load is in bounds and unconditional; a face or
// solid neighbour's term is dropped.  Term order: x-, x+, y-, y+, z-, z+ (physics.py:76-77).
template <int VEC>
__device__ __forceinline__ DV<VEC> lap_group(const CleanArgs &a, const double *__restrict__ X, double sc,
                                             const uint8_t *__restrict__ M, const Pos &p, const MV<VEC> &mc) {
    const bool xl = p.x > 0, xh = p.x + VEC < a.nx, yl = p.y > 0, yh = p.y + 1 < a.ny, zl = p.z > 0,
               zh = p.z + 1 < a.nz;
    const unsigned i = p.i;
    const DV<VEC> c = ldd<VEC>(X + i);
    const double cl = X[i - (xl ? 1u : 0u)], cr = X[i + VEC - 1 + (xh ? 1u : 0u)];
    const uint8_t ml = M[i - (xl ? 1u : 0u)], mr = M[i + VEC - 1 + (xh ? 1u : 0u)];
    const unsigned oym = yl ? (unsigned)a.nx : 0u, oyp = yh ? (unsigned)a.nx : 0u;
    const unsigned ozm = zl ? a.plane : 0u, ozp = zh ? a.plane : 0u;
    const DV<VEC> ym = ldd<VEC>(X + i - oym), yp = ldd<VEC>(X + i + oyp);
    const DV<VEC> zm = ldd<VEC>(X + i - ozm), zp = ldd<VEC>(X + i + ozp);
    const MV<VEC> mym = ldmk<VEC>(M + i - oym), myp = ldmk<VEC>(M + i + oyp);
    const MV<VEC> mzm = ldmk<VEC>(M + i - ozm), mzp = ldmk<VEC>(M + i + ozp);
    DV<VEC> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const double xi = c.e[e] * sc;
        const bool hasl = e > 0 ? true : xl, hasr = e + 1 < VEC ? true : xh;
        const double vl = e > 0 ? c.e[e > 0 ? e - 1 : 0] : cl;
        const double vr = e + 1 < VEC ? c.e[e + 1 < VEC ? e + 1 : e] : cr;
        const bool fl = (e > 0 ? mc.e[e > 0 ? e - 1 : 0] : ml) != 0;
        const bool fr = (e + 1 < VEC ? mc.e[e + 1 < VEC ? e + 1 : e] : mr) != 0;
        double acc = 0.0;
        if (hasl && fl) acc += (vl * sc - xi) * a.hx;
        if (hasr && fr) acc += (vr * sc - xi) * a.hx;
        if (yl && mym.e[e]) acc += (ym.e[e] * sc - xi) * a.hy;
        if (yh && myp.e[e]) acc += (yp.e[e] * sc - xi) * a.hy;
        if (zl && mzm.e[e]) acc += (zm.e[e] * sc - xi) * a.hz;
        if (zh && mzp.e[e]) acc += (zp.e[e] * sc - xi) * a.hz;
        o.e[e] = mc.e[e] ? acc : 0.0;
    }
    return o;
}

// y = A x (ptv_laplacian_apply): solid voxels are written as 0
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_laplacian(CleanArgs a, const double *__restrict__ X,
                                                        const uint8_t *__restrict__ M, double *__restrict__ Y) {
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i);
        std_<VEC>(Y + p.i, lap_group<VEC>(a, X, 1.0, M, p, mc));
    }
}

// Golub-Kahan step: Y <- A (sx X) - c (sy Y) on fluid voxels, partial sums of the new Y^2.
// which = 0: u <- A v - alfa u (lsqr.py:430);  which = 1: v <- A^T u - beta v (:436)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_bidiag(CleanArgs a, int which, const double *__restrict__ st,
                                                     const double *__restrict__ X, double *__restrict__ Y,
                                                     const uint8_t *__restrict__ M, double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    if (which == 1 && st[S_SKIPV] != 0.0) return;
    const double sx = which == 0 ? st[S_INV_ALFA] : st[S_INV_BETA];
    const double sy = which == 0 ? st[S_INV_BETA] : st[S_INV_ALFA];
    const double c = which == 0 ? st[S_ALFA] : st[S_BETA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || mc.e[e];
        if (!any) continue;
        const DV<VEC> ax = lap_group<VEC>(a, X, sx, M, p, mc);
        DV<VEC> y = ldd<VEC>(Y + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double t = ax.e[e] - c * (y.e[e] * sy);
            y.e[e] = mc.e[e] ? t : 0.0;
            ss += y.e[e] * y.e[e];
        }
        std_<VEC>(Y + p.i, y);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// x <- x + t1 w;  w <- v + t2 w;  partial sums of ((1/rho) w)^2 (lsqr.py:465-471)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_update(CleanArgs a, const double *__restrict__ st,
                                                     const double *__restrict__ V, double *__restrict__ W,
                                                     double *__restrict__ Xs, const uint8_t *__restrict__ M,
                                                     double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    const double t1 = st[S_T1], t2 = st[S_T2], ir = st[S_INV_RHO], ia = st[S_INV_ALFA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || mc.e[e];
        if (!any) continue;
        const DV<VEC> v = ldd<VEC>(V + p.i);
        DV<VEC> w = ldd<VEC>(W + p.i), x = ldd<VEC>(Xs + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (!mc.e[e]) continue;
            const double dk = ir * w.e[e];
            ss += dk * dk;
            x.e[e] = x.e[e] + t1 * w.e[e];
            w.e[e] = v.e[e] * ia + t2 * w.e[e];
        }
        std_<VEC>(W + p.i, w);
        std_<VEC>(Xs + p.i, x);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// LSQR's first u: b = div[fluid] - mean(div[fluid]) (physics.py:182-183), partial sums of b^2
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_rhs(CleanArgs a, const double *__restrict__ st,
                                                  const double *__restrict__ D, const uint8_t *__restrict__ M,
                                                  double *__restrict__ U, double *__restrict__ part) {
    const double mean = st[S_MEAN];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i);
        const DV<VEC> d = ldd<VEC>(D + p.i);
        DV<VEC> b;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            b.e[e] = mc.e[e] ? d.e[e] - mean : 0.0;
            ss += b.e[e] * b.e[e];
        }
        std_<VEC>(U + p.i, b);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// partial counts of NaN entries of the solution
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_nan(CleanArgs a, const double *__restrict__ Xs,
                                                  double *__restrict__ part) {
    double c = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const DV<VEC> x = ldd<VEC>(Xs + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) c += (x.e[e] != x.e[e]) ? 1.0 : 0.0;
    }
    c = block_sum(c);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

// net x-flux through the middle YZ plane: sum(u[:, :, nx // 2]) * dy * dz (physics.py:160-165)
__global__ __launch_bounds__(kGridFinalThreads) void k_flux(CleanArgs a, const double *__restrict__ U,
                                                        double *__restrict__ rep, int slot) {
    const unsigned rows = (unsigned)a.ny * (unsigned)a.nz;
    const unsigned mid = (unsigned)(a.nx / 2);
    double s = 0.0;
    for (unsigned r = threadIdx.x; r < rows; r += kGridFinalThreads) s += U[r * (unsigned)a.nx + mid];
    s = block_sum(s);
    if (threadIdx.x == 0) rep[slot] = s * a.dy * a.dz;
}

__device__ __forceinline__ double sgn(double a) { return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0); }

// scipy's _sym_ortho (lsqr.py:62-94)
__device__ __forceinline__ void sym_ortho(double a, double b, double &c, double &s, double &r) {
    if (b == 0.0) {
        c = sgn(a);
        s = 0.0;
        r = fabs(a);
    } else if (a == 0.0) {
        c = 0.0;
        s = sgn(b);
        r = fabs(b);
    } else if (fabs(b) > fabs(a)) {
        const double tau = a / b;
        s = sgn(b) / sqrt(1.0 + tau * tau);
        c = s * tau;
        r = b / s;
    } else {
        const double tau = b / a;
        c = sgn(a) / sqrt(1.0 + tau * tau);
        s = c * tau;
        r = a / c;
    }
}

// Second reduction stage and the scalar recurrences.  One block sums the partials in a fixed order
// (partial_sum), then thread 0 alone advances the state exactly as scipy's lsqr does between its
// vector operations.
__global__ __launch_bounds__(kGridFinalThreads) void k_scalar(int phase, LsqrCfg cfg, double *__restrict__ st,
                                                          const double *__restrict__ part, unsigned npart,
                                                          double *__restrict__ rep, int slot) {
    const bool solver = phase == PH_BETA || phase == PH_ALFA || phase == PH_TEST;
    if (solver && st[S_STOP] != 0.0) return;
    const double r0 = partial_sum(part, npart);
    double r1 = 0.0, r2 = 0.0;
    if (phase == PH_DIVSTATS) {
        r1 = partial_sum(part + npart, npart);
        r2 = partial_sum(part + 2 * npart, npart);
    }
    if (threadIdx.x != 0) return;
    const double dampsq = cfg.damp * cfg.damp;
    switch (phase) {
    case PH_DIVSTATS:
        st[S_NFLUID] = r2;
        st[S_MEAN] = r0 / r2;
        st[S_MEANABS] = r1 / r2;
        rep[slot] = r1 / r2;
        break;
    case PH_NAN:
        st[S_NAN] = r0;
        break;
    case PH_INIT_BETA: {  // lsqr.py:355-385: u = b, beta = ||b||
        const double beta = sqrt(r0);
        for (int k = 0; k < S_MEAN; ++k) st[k] = 0.0;
        st[S_NAN] = 0.0;
        st[S_CS2] = -1.0;
        st[S_BNORM] = beta;
        st[S_BETA] = beta;
        st[S_INV_BETA] = beta > 0.0 ? 1.0 / beta : 1.0;
        st[S_INV_ALFA] = 1.0;  // v is still the zero vector
        st[S_SKIPV] = beta > 0.0 ? 0.0 : 1.0;
        break;
    }
    case PH_INIT_ALFA: {  // lsqr.py:386-408: v = A^T u, alfa = ||v||, w = v
        const double beta = st[S_BETA];
        const double alfa = st[S_SKIPV] != 0.0 ? 0.0 : sqrt(r0);
        st[S_ALFA] = alfa;
        st[S_INV_ALFA] = alfa > 0.0 ? 1.0 / alfa : 1.0;
        st[S_T1] = 0.0;  // the first k_update only copies w = v (x and w are 0)
        st[S_T2] = 0.0;
        st[S_INV_RHO] = 0.0;
        st[S_RHOBAR] = alfa;
        st[S_PHIBAR] = beta;
        st[S_RNORM] = beta;
        st[S_ARNORM] = alfa * beta;
        if (alfa * beta == 0.0) st[S_STOP] = 1.0;  // x = 0 is the solution, istop = 0
        if (cfg.iter_lim <= 0) st[S_STOP] = 1.0;
        break;
    }
    case PH_BETA: {  // lsqr.py:425-435
        st[S_ITN] += 1.0;
        const double beta = sqrt(r0), alfa = st[S_ALFA], an = st[S_ANORM];
        st[S_BETA] = beta;
        if (beta > 0.0) {
            st[S_INV_BETA] = 1.0 / beta;
            st[S_ANORM] = sqrt(an * an + alfa * alfa + beta * beta + dampsq);
            st[S_SKIPV] = 0.0;
        } else {
            st[S_INV_BETA] = 1.0;  // u is the zero vector (or NaN), left as it is
            st[S_SKIPV] = 1.0;
        }
        break;
    }
    case PH_ALFA: {  // lsqr.py:436-488
        double alfa = st[S_ALFA];
        if (st[S_SKIPV] == 0.0) {
            alfa = sqrt(r0);
            st[S_ALFA] = alfa;
            st[S_INV_ALFA] = alfa > 0.0 ? 1.0 / alfa : 1.0;
        }
        const double beta = st[S_BETA];
        double rhobar = st[S_RHOBAR], phibar = st[S_PHIBAR];
        double rhobar1, psi;
        if (cfg.damp > 0.0) {
            rhobar1 = sqrt(rhobar * rhobar + dampsq);
            const double cs1 = rhobar / rhobar1, sn1 = cfg.damp / rhobar1;
            psi = sn1 * phibar;
            phibar = cs1 * phibar;
        } else {
            rhobar1 = rhobar;
            psi = 0.0;
        }
        double cs, sn, rho;
        sym_ortho(rhobar1, beta, cs, sn, rho);
        const double theta = sn * alfa;
        rhobar = -cs * alfa;
        const double phi = cs * phibar;
        phibar = sn * phibar;
        const double tau = sn * phi;
        st[S_T1] = phi / rho;
        st[S_T2] = -theta / rho;
        st[S_INV_RHO] = 1.0 / rho;
        st[S_RHOBAR] = rhobar;
        st[S_PHIBAR] = phibar;
        const double delta = st[S_SN2] * rho, gambar = -st[S_CS2] * rho;
        const double rhs = phi - delta * st[S_Z];
        const double zbar = rhs / gambar;
        st[S_XNORM] = sqrt(st[S_XXNORM] + zbar * zbar);
        const double gamma = sqrt(gambar * gambar + theta * theta);
        st[S_CS2] = gambar / gamma;
        st[S_SN2] = theta / gamma;
        const double z = rhs / gamma;
        st[S_Z] = z;
        st[S_XXNORM] = st[S_XXNORM] + z * z;
        st[S_RES2] = st[S_RES2] + psi * psi;
        st[S_RNORM] = sqrt(phibar * phibar + st[S_RES2]);
        st[S_ARNORM] = alfa * fabs(tau);
        break;
    }
    case PH_TEST: {  // lsqr.py:471, 490-572
        const double eps = 2.220446049250313e-16;
        const double nd = sqrt(r0);
        const double ddnorm = st[S_DDNORM] + nd * nd;
        st[S_DDNORM] = ddnorm;
        const double anorm = st[S_ANORM], rnorm = st[S_RNORM], arnorm = st[S_ARNORM], xnorm = st[S_XNORM],
                     bnorm = st[S_BNORM];
        const double acond = anorm * sqrt(ddnorm);
        st[S_ACOND] = acond;
        const double test1 = rnorm / bnorm;
        const double test2 = arnorm / (anorm * rnorm + eps);
        const double test3 = 1.0 / (acond + eps);
        const double t1 = test1 / (1.0 + anorm * xnorm / bnorm);
        const double rtol = cfg.btol + cfg.atol * anorm * xnorm / bnorm;
        int istop = 0;
        if (st[S_ITN] >= (double)cfg.iter_lim) istop = 7;
        if (1.0 + test3 <= 1.0) istop = 6;
        if (1.0 + test2 <= 1.0) istop = 5;
        if (1.0 + t1 <= 1.0) istop = 4;
        if (test3 <= cfg.ctol) istop = 3;
        if (test2 <= cfg.atol) istop = 2;
        if (test1 <= rtol) istop = 1;
        if (istop != 0) {
            st[S_ISTOP] = (double)istop;
            st[S_STOP] = 1.0;
        }
        break;
    }
    default:
        break;
    }
}

// apply_consistent_correction (physics.py:110-147) with phi already on the grid.  Per axis
//     g_next = (i < n-1 && fluid[i+1] && fluid[i]) ? (p[i+1] - p[i]) / h : 0      (:126-130)
//     g_prev = (i > 0   && fluid[i] && fluid[i-1]) ? (p[i] - p[i-1]) / h : 0      (:133-135)
//     out = vel - (g_next + g_prev) / 2.0, solid voxels 0                         (:138-146)
// in the reference's operation order: bit-identical to numpy given the same phi.  May run in place
// (Uo == U): a voxel reads only its own velocity.
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_correction(CleanArgs a, const double *__restrict__ P,
                                                         const uint8_t *__restrict__ M, const double *U,
                                                         const double *V, const double *W, double *Uo, double *Vo,
                                                         double *Wo) {
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const bool xl = p.x > 0, xh = p.x + VEC < a.nx, yl = p.y > 0, yh = p.y + 1 < a.ny, zl = p.z > 0,
                   zh = p.z + 1 < a.nz;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        const DV<VEC> c = ldd<VEC>(P + i);
        const double cl = P[i - (xl ? 1u : 0u)], cr = P[i + VEC - 1 + (xh ? 1u : 0u)];
        const uint8_t ml = M[i - (xl ? 1u : 0u)], mr = M[i + VEC - 1 + (xh ? 1u : 0u)];
        const unsigned oym = yl ? (unsigned)a.nx : 0u, oyp = yh ? (unsigned)a.nx : 0u;
        const unsigned ozm = zl ? a.plane : 0u, ozp = zh ? a.plane : 0u;
        const DV<VEC> ym = ldd<VEC>(P + i - oym), yp = ldd<VEC>(P + i + oyp);
        const DV<VEC> zm = ldd<VEC>(P + i - ozm), zp = ldd<VEC>(P + i + ozp);
        const MV<VEC> mym = ldmk<VEC>(M + i - oym), myp = ldmk<VEC>(M + i + oyp);
        const MV<VEC> mzm = ldmk<VEC>(M + i - ozm), mzp = ldmk<VEC>(M + i + ozp);
        DV<VEC> u = ldd<VEC>(U + i), v = ldd<VEC>(V + i), w = ldd<VEC>(W + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double pc = c.e[e];
            const bool hasl = e > 0 ? true : xl, hasr = e + 1 < VEC ? true : xh;
            const double vl = e > 0 ? c.e[e > 0 ? e - 1 : 0] : cl;
            const double vr = e + 1 < VEC ? c.e[e + 1 < VEC ? e + 1 : e] : cr;
            const bool fl = (e > 0 ? mc.e[e > 0 ? e - 1 : 0] : ml) != 0;
            const bool fr = (e + 1 < VEC ? mc.e[e + 1 < VEC ? e + 1 : e] : mr) != 0;
            const bool own = mc.e[e] != 0;
            const double gxn = (hasr && fr && own) ? (vr - pc) / a.dx : 0.0;
            const double gxp = (hasl && fl && own) ? (pc - vl) / a.dx : 0.0;
            const double gyn = (yh && myp.e[e] && own) ? (yp.e[e] - pc) / a.dy : 0.0;
            const double gyp = (yl && mym.e[e] && own) ? (pc - ym.e[e]) / a.dy : 0.0;
            const double gzn = (zh && mzp.e[e] && own) ? (zp.e[e] - pc) / a.dz : 0.0;
            const double gzp = (zl && mzm.e[e] && own) ? (pc - zm.e[e]) / a.dz : 0.0;
            u.e[e] = own ? u.e[e] - (gxn + gxp) * 0.5 : 0.0;  // / 2.0 == * 0.5 exactly
            v.e[e] = own ? v.e[e] - (gyn + gyp) * 0.5 : 0.0;
            w.e[e] = own ? w.e[e] - (gzn + gzp) * 0.5 : 0.0;
        }
        std_<VEC>(Uo + i, u);
        std_<VEC>(Vo + i, v);
        std_<VEC>(Wo + i, w);
    }
}

int make_args(const GridSpec &g, CleanArgs &a) {
    PTV_TRY(grid_dims("clean", g.nx, g.ny, g.nz, a));
    if (!(g.dx != 0.0) || !(g.dy != 0.0) || !(g.dz != 0.0) || std::isnan(g.dx) || std::isnan(g.dy) ||
        std::isnan(g.dz)) {
        set_error("clean: spacings must be non-zero numbers");
        return PTV_E_ARG;
    }
    a.dx = g.dx;
    a.dy = g.dy;
    a.dz = g.dz;
    a.hx = 1.0 / (g.dx * g.dx);
    a.hy = 1.0 / (g.dy * g.dy);
    a.hz = 1.0 / (g.dz * g.dz);
    return PTV_OK;
}

// one LSQR solve on the vectors of `wk`; u holds b on entry, x the solution on exit
struct Solver {
    CleanWork &wk;
    CleanArgs a;
    LsqrCfg cfg;
    const uint8_t *M;
    hipStream_t s;
    bool vec2;
    unsigned nb;

    int bidiag(int which) {
        const double *X = which == 0 ? wk.v.p : wk.u.p;
        double *Y = which == 0 ? wk.u.p : wk.v.p;
        GRID_LAUNCH(k_bidiag, vec2, nb, s, a, which, wk.state.p, X, Y, M, wk.part.p);
        return PTV_OK;
    }
    int update() {
        GRID_LAUNCH(k_update, vec2, nb, s, a, wk.state.p, wk.v.p, wk.w.p, wk.x.p, M, wk.part.p);
        return PTV_OK;
    }
    int scalar(int phase, int slot = 0) {
        hipLaunchKernelGGL(k_scalar, dim3(1), dim3(kGridFinalThreads), 0, s, phase, cfg, wk.state.p, wk.part.p, nb, wk.rep.p, slot);
        PTV_HIP(hipGetLastError());
        return PTV_OK;
    }
    int div_stats(int slot) {
        GRID_LAUNCH(k_div_stats, vec2, nb, s, a, wk.div.p, M, wk.part.p, nb);
        return scalar(PH_DIVSTATS, slot);
    }
    int flux(const double *U, int slot) {
        hipLaunchKernelGGL(k_flux, dim3(1), dim3(kGridFinalThreads), 0, s, a, U, wk.rep.p, slot);
        PTV_HIP(hipGetLastError());
        return PTV_OK;
    }
    int event(size_t k) { return record_event(wk.ev, k, s); }

    // one solve; also returns the median ms per iteration over its polling batches
    int solve(double *h_final, double &ms_solve, double &ms_iter_median) {
        const size_t nbytes = (size_t)a.n * sizeof(double);
        PTV_TRY(event(2));
        GRID_LAUNCH(k_rhs, vec2, nb, s, a, wk.state.p, wk.div.p, M, wk.u.p, wk.part.p);
        PTV_TRY(scalar(PH_INIT_BETA));
        PTV_HIP(hipMemsetAsync(wk.v.p, 0, nbytes, s));
        PTV_HIP(hipMemsetAsync(wk.w.p, 0, nbytes, s));
        PTV_HIP(hipMemsetAsync(wk.x.p, 0, nbytes, s));
        PTV_TRY(bidiag(1));
        PTV_TRY(scalar(PH_INIT_ALFA));
        PTV_TRY(update());  // w = v
        PTV_TRY(event(3));
        const size_t sbytes = kStateLen * sizeof(double);
        std::vector<int> batch_iters;
        PTV_TRY(poll_batches(s, wk.state.p, wk.h_state.p, kStateLen, wk.ev, cfg.iter_lim, [&](int) -> int {
            PTV_TRY(bidiag(0));
            PTV_TRY(scalar(PH_BETA));
            PTV_TRY(bidiag(1));
            PTV_TRY(scalar(PH_ALFA));
            PTV_TRY(update());
            return scalar(PH_TEST);
        }, batch_iters));
        const size_t batches = batch_iters.size();
        GRID_LAUNCH(k_nan, vec2, nb, s, a, wk.x.p, wk.part.p);
        PTV_TRY(scalar(PH_NAN));
        PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, sbytes, hipMemcpyDeviceToHost, s));
        PTV_TRY(event(4 + batches));
        PTV_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, wk.ev[2], wk.ev[4 + batches]));
        ms_solve = ms;
        PTV_TRY(median_iter_ms(wk.ev, 3, batch_iters, (int)h_final[S_ITN], ms_solve, ms_iter_median));
        return PTV_OK;
    }
};

}  // namespace

int launch_clean_laplacian(const GridSpec &g, const uint8_t *M, const double *x, double *y, hipStream_t s) {
    CleanArgs a{};
    PTV_TRY(make_args(g, a));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(x, y) && aligned(M, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    GRID_LAUNCH(k_laplacian, vec2, nb, s, a, x, M, y);
    return PTV_OK;
}

int launch_clean_correction(const GridSpec &g, const uint8_t *M, const double *U, const double *V, const double *W,
                            const double *phi, double *Uo, double *Vo, double *Wo, hipStream_t s) {
    CleanArgs a{};
    PTV_TRY(make_args(g, a));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(U, V, W, phi, Uo, Vo, Wo) && aligned(M, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    GRID_LAUNCH(k_correction, vec2, nb, s, a, phi, M, U, V, W, Uo, Vo, Wo);
    return PTV_OK;
}

int clean_solve_rhs(CleanWork &wk, const GridSpec &g, const CleanSolve &sv, const uint8_t *M, const double *rhs,
                    double *X, hipStream_t s, CleanRhsResult *res) {
    CleanArgs a{};
    PTV_TRY(make_args(g, a));
    if (sv.iter_lim < 0 || !(sv.damp >= 0.0) || !(sv.atol >= 0.0) || !(sv.btol >= 0.0)) {
        set_error("clean: iter_lim, damp, atol and btol must be non-negative");
        return PTV_E_ARG;
    }
    const size_t n = a.n, nbytes = n * sizeof(double);
    for (DevBuf<double> *b : {&wk.u, &wk.v, &wk.w, &wk.x, &wk.div}) PTV_TRY(b->ensure(n));
    const bool vec2 = a.nx % 2 == 0 && aligned(M, 2);  // every vector is hipMalloc-aligned scratch
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    PTV_TRY(wk.part.ensure(3 * (size_t)nb));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.rep.ensure(kRepLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen + kRepLen));
    double *h_final = wk.h_state.p + 2 * kStateLen;
    Solver sol{wk, a, LsqrCfg{sv.damp, sv.atol, sv.btol, 1.0 / 1e8, sv.iter_lim}, M, s, vec2, nb};
    PTV_HIP(hipMemsetAsync(wk.state.p, 0, kStateLen * sizeof(double), s));
    PTV_HIP(hipMemcpyAsync(wk.div.p, rhs, nbytes, hipMemcpyDeviceToDevice, s));
    PTV_TRY(sol.div_stats(3));  // the mean of rhs over the fluid voxels, which k_rhs subtracts
    double ms = 0.0, med = 0.0;
    PTV_TRY(sol.solve(h_final, ms, med));
    PTV_HIP(hipMemcpyAsync(X, wk.x.p, nbytes, hipMemcpyDeviceToDevice, s));  // solid entries are the memset's 0
    PTV_HIP(hipStreamSynchronize(s));
    if (res) {
        res->n_fluid = (int64_t)h_final[S_NFLUID];
        res->istop = (int)h_final[S_ISTOP];
        res->itn = (int)h_final[S_ITN];
        res->bnorm = h_final[S_BNORM];
        res->rnorm = h_final[S_RNORM];
        res->ms_solve = ms;
        res->ms_iter_median = med;
    }
    return PTV_OK;
}

int clean_run(CleanWork &wk, const GridSpec &g, const CleanSolve &sv, const uint8_t *M, const double *U,
              const double *V, const double *W, double *Uo, double *Vo, double *Wo, hipStream_t s,
              ptv_clean_stats *st) {
    CleanArgs a{};
    PTV_TRY(make_args(g, a));
    if (sv.iterations < 0 || sv.iter_lim < 0 || !(sv.damp >= 0.0) || !(sv.atol >= 0.0) || !(sv.btol >= 0.0)) {
        set_error("clean: iterations, iter_lim, damp, atol and btol must be non-negative");
        return PTV_E_ARG;
    }
    const size_t n = a.n, nbytes = n * sizeof(double);
    for (DevBuf<double> *b : {&wk.u, &wk.v, &wk.w, &wk.x, &wk.div}) PTV_TRY(b->ensure(n));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(Uo, Vo, Wo) && aligned(M, 2);  // scratch is hipMalloc-aligned
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    PTV_TRY(wk.part.ensure(3 * (size_t)nb));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.rep.ensure(kRepLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen + kRepLen));
    double *h_final = wk.h_state.p + 2 * kStateLen, *h_rep = wk.h_state.p + 3 * kStateLen;

    Solver sol{wk, a, LsqrCfg{sv.damp, sv.atol, sv.btol, 1.0 / 1e8, sv.iter_lim}, M, s, vec2, nb};
    const DivArgs d = full_grid_div(a, g.dx, g.dy, g.dz);

    ptv_clean_stats out{};
    PTV_TRY(sol.event(0));
    PTV_HIP(hipMemsetAsync(wk.state.p, 0, kStateLen * sizeof(double), s));
    PTV_HIP(hipMemsetAsync(wk.rep.p, 0, kRepLen * sizeof(double), s));
    PTV_TRY(sol.flux(U, 0));
    // the divergence of the input: iteration 1's "current" and the report's "initial" (physics.py:173, :199)
    PTV_TRY(launch_divergence(d, U, V, W, M, wk.div.p, s));
    PTV_TRY(sol.div_stats(3));
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, kStateLen * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    out.n_fluid = (int64_t)h_final[S_NFLUID];
    if (out.n_fluid <= 0) {  // an argument error: the outputs are not written
        set_error("clean: the fluid mask has no fluid voxel");
        return PTV_E_ARG;
    }
    if (Uo != U) PTV_HIP(hipMemcpyAsync(Uo, U, nbytes, hipMemcpyDeviceToDevice, s));
    if (Vo != V) PTV_HIP(hipMemcpyAsync(Vo, V, nbytes, hipMemcpyDeviceToDevice, s));
    if (Wo != W) PTV_HIP(hipMemcpyAsync(Wo, W, nbytes, hipMemcpyDeviceToDevice, s));
    double ms_solve_total = 0.0;
    for (int i = 0; i < sv.iterations; ++i) {
        const int slot = std::min(i, PTV_CLEAN_MAX_OUTER);  // past the stats' capacity: the spare slot
        if (i > 0) {
            PTV_TRY(launch_divergence(d, Uo, Vo, Wo, M, wk.div.p, s));
            PTV_TRY(sol.div_stats(3 + slot));
        }
        double ms = 0.0, med = 0.0;
        PTV_TRY(sol.solve(h_final, ms, med));
        ms_solve_total += ms;
        out.n_outer = i + 1;
        if (i < PTV_CLEAN_MAX_OUTER) {
            out.istop[i] = (int32_t)h_final[S_ISTOP];
            out.itn[i] = (int32_t)h_final[S_ITN];
            out.rnorm[i] = h_final[S_RNORM];
            out.ms_iter_median[i] = med;
        }
        if (h_final[S_NAN] != 0.0) {  // physics.py:189-191
            out.nan_stop = 1;
            break;
        }
        PTV_TRY(launch_clean_correction(g, M, Uo, Vo, Wo, wk.x.p, Uo, Vo, Wo, s));
    }
    PTV_TRY(launch_divergence(d, Uo, Vo, Wo, M, wk.div.p, s));
    PTV_TRY(sol.div_stats(2));
    PTV_TRY(sol.flux(Uo, 1));
    PTV_HIP(hipMemcpyAsync(h_rep, wk.rep.p, kRepLen * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_TRY(sol.event(1));
    PTV_HIP(hipStreamSynchronize(s));
    out.flux_initial = h_rep[0];
    out.flux_final = h_rep[1];
    out.mean_abs_div_final = h_rep[2];
    for (int i = 0; i < PTV_CLEAN_MAX_OUTER; ++i) out.mean_abs_div[i] = h_rep[3 + i];
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, wk.ev[0], wk.ev[1]));
    out.ms_total = ms;
    out.ms_solve = ms_solve_total;
    if (st) *st = out;
    return PTV_OK;
}

}  // namespace ptv
