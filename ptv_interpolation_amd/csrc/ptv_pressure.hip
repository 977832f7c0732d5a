// ptv_pressure.hip — pressure recovery: force field, force divergence, anchored matrix-free CG.
//
// Restates velocity_analysis.compute_pressure_field (velocity_analysis.py:190-330) and the parts of
// physics.py it calls: compute_force_divergence (:211-262) and solve_poisson's anchored branch
// (:264-345, cg(A, b, tol=1e-10, maxiter=3000) on build_laplacian_matrix, :55-108).
//
// Storage as in ptv_clean.hip and ptv_variational.hip: dense float64 (nz, ny, nx) grids, x fastest,
// a uint8 mask (nonzero = fluid); a lane owns VEC consecutive x (2 when nx is even and the buffers
// are aligned).  Reductions are the two-stage fixed-order sums of ptv_grid_vec.hpp.
//
// Force field (laplacian_mask_aware, :210-269, then :273-289), three passes:
//   k_lap     raw Laplacian of u, v, w at every voxel, lap = 0 + tz + ty + tx with
//             t = (f_next - 2 f + f_prev) / h**2 and clamped neighbours; the voxel's code: 0 solid,
//             1 bulk (scipy's binary_erosion: fluid with six fluid neighbours inside the domain),
//             4 fluid not bulk; partial counts of bulk voxels
//   k_fill    round 1 in place: a code-4 voxel averages the Laplacians of its code-1 neighbours in
//             the order z+1, z-1, y+1, y-1, x+1, x-1 (np.roll: they wrap around the domain) and
//             becomes code 2.  A round reads only voxels whose code is at most the round's number
//             and writes only code-4 voxels, so it runs in place without a race
//   k_force   round 2 fused with the force: a code-4 voxel averages its code-1 and code-2
//             neighbours (not stored: nothing reads it later); f = mu * lap, and for rho > 0
//             f -= rho * (u gx + v gy + w gz) with np.gradient's formula; partial sums over the
//             fluid voxels of |fx|, |fy|, |fz|, w and 1
// With no bulk voxel the reference returns the raw Laplacian: both fills test the device-resident
// bulk count.
//
// CG: the unknowns are the fluid voxels that are not Dirichlet ("active").  x, r, p are 0 at every
// other voxel and stay 0, so a Dirichlet neighbour enters (A p)_i = sum (p_j - p_i) h^-2 as p_j = 0
// and counts in the diagonal: the symmetric system with the Dirichlet rows and columns eliminated.
// One iteration (scipy _isolve/iterative.py, cg):
//     k_pcg_scalar TOP:    rr = sum r^2;  ||r|| < rtol ||b|| stops, info 0;  else rho, beta
//     k_pq:                p' = r + beta p (into the other p buffer),  q = A p',  partial sums of p' q
//     k_pcg_scalar ALPHA:  alpha = rho / sum p' q
//     k_pxr:               x += alpha p',  r -= alpha q,  partial sums of r^2
// k_pq recomputes the six neighbours' p' from r and p with the owners' expression.  Bytes per voxel
// and iteration: k_pq 8 r + 8 p + 8 p' + 8 q + 1 mask = 33; k_pxr 8 p' + 8 q + 8 x + 8 r reads, 8 x +
// 8 r writes + 1 = 49; 82 in all, + 2 with a Dirichlet grid (one byte in each pass).
// The scalar recurrence with its stopping rules and NaN outcome, the stop flag and the polling loop
// are those of ptv_grid_solve.hpp.
#include <cmath>
#include <algorithm>

#include "ptv_pressure.hpp"
#include "ptv_grid_solve.hpp"

namespace ptv {

namespace {

using namespace cg;

// device-resident state (doubles): the CG recurrence, the solve's counts, then what the force pass leaves
enum { S_NDIR = S_CG_COUNT, S_NFLUID, S_RZ, S_COUNT, F_BULK = 16, F_SFX, F_SFY, F_SFZ, F_SW, F_NFLUID, F_COUNT };
constexpr int kStateLen = 24;
static_assert(S_COUNT <= F_BULK && F_COUNT <= kStateLen, "state length");

enum { PH_BULK = PH_CG_COUNT, PH_FORCE };
enum Code : uint8_t { C_SOLID = 0, C_BULK = 1, C_FILL1 = 2, C_FILL2 = 3, C_OPEN = 4 };

struct PArgs : GridDims {
    double h[3];    // dx, dy, dz
    double h2[3];   // h ** 2 (the raw Laplacian divides by it)
    double ih2[3];  // 1.0 / h ** 2 (the matrix entries, physics.py:68)
};

// the six neighbours of voxel (x, y, z) at index i, clamped at the array ends
struct Clamp {
    unsigned xm, xp, ym, yp, zm, zp;
};
__device__ __forceinline__ Clamp clamped(const GridDims &a, unsigned i, int x, int y, int z) {
    Clamp c;
    c.xm = x > 0 ? i - 1 : i;
    c.xp = x + 1 < a.nx ? i + 1 : i;
    c.ym = y > 0 ? i - (unsigned)a.nx : i;
    c.yp = y + 1 < a.ny ? i + (unsigned)a.nx : i;
    c.zm = z > 0 ? i - a.plane : i;
    c.zp = z + 1 < a.nz ? i + a.plane : i;
    return c;
}

// raw Laplacian of three fields at every voxel, the voxel codes, partial counts of bulk voxels
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_lap(PArgs a, CV3 F, const uint8_t *__restrict__ M, V3 L,
                                                      uint8_t *__restrict__ code, double *__restrict__ part) {
    double nbulk = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned i = p.i + e;
            const int x = p.x + e;
            const Clamp c = clamped(a, i, x, p.y, p.z);
            const bool inside = x > 0 && x + 1 < a.nx && p.y > 0 && p.y + 1 < a.ny && p.z > 0 && p.z + 1 < a.nz;
            const bool fluid = M[i] != 0;
            const bool bulk = fluid && inside && M[c.xm] && M[c.xp] && M[c.ym] && M[c.yp] && M[c.zm] && M[c.zp];
            code[i] = !fluid ? C_SOLID : bulk ? C_BULK : C_OPEN;
            nbulk += bulk ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *__restrict__ f = F.c[k];
                const double fc = f[i];
                double lap = 0.0;
                lap += ((f[c.zp] - 2 * fc) + f[c.zm]) / a.h2[2];
                lap += ((f[c.yp] - 2 * fc) + f[c.ym]) / a.h2[1];
                lap += ((f[c.xp] - 2 * fc) + f[c.xm]) / a.h2[0];
                L.c[k][i] = lap;
            }
        }
    }
    nbulk = block_sum(nbulk);
    if (threadIdx.x == 0) part[blockIdx.x] = nbulk;
}

// the six neighbours under np.roll: they wrap around the domain; order z+1, z-1, y+1, y-1, x+1, x-1
struct Wrap {
    unsigned j[6];
};
__device__ __forceinline__ Wrap wrapped(const GridDims &a, unsigned i, int x, int y, int z) {
    Wrap w;
    w.j[0] = z + 1 < a.nz ? i + a.plane : i - (unsigned)z * a.plane;
    w.j[1] = z > 0 ? i - a.plane : i + (unsigned)(a.nz - 1) * a.plane;
    w.j[2] = y + 1 < a.ny ? i + (unsigned)a.nx : i - (unsigned)y * (unsigned)a.nx;
    w.j[3] = y > 0 ? i - (unsigned)a.nx : i + (unsigned)(a.ny - 1) * (unsigned)a.nx;
    w.j[4] = x + 1 < a.nx ? i + 1 : i - (unsigned)x;
    w.j[5] = x > 0 ? i - 1 : i + (unsigned)(a.nx - 1);
    return w;
}

// one fill round at a code-4 voxel: sum / count over the neighbours whose code is in [1, top]
// (:252-264); false when no neighbour qualifies
__device__ __forceinline__ bool fill_average(const Wrap &w, const uint8_t *__restrict__ code, uint8_t top, CV3 L,
                                             double out[3]) {
    double sum[3] = {0.0, 0.0, 0.0}, count = 0.0;
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const uint8_t cn = code[w.j[n]];
        if (cn >= C_BULK && cn <= top) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sum[k] += L.c[k][w.j[n]];
            count += 1.0;
        }
    }
    if (count == 0.0) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = sum[k] / count;
    return true;
}

// fill round 1, in place (see the head of the file for why that is no race)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_fill(PArgs a, const double *__restrict__ st, V3 L,
                                                       uint8_t *code) {
    if (st[F_BULK] == 0.0) return;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned i = p.i + e;
            if (code[i] != C_OPEN) continue;
            double v[3];
            if (!fill_average(wrapped(a, i, p.x + e, p.y, p.z), code, C_BULK, CV3{{L.c[0], L.c[1], L.c[2]}}, v))
                continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) L.c[k][i] = v[k];
            code[i] = C_FILL1;
        }
    }
}

// np.gradient along one axis at position t of n (n >= 2) with the neighbours' values
__device__ __forceinline__ double grad1(double fm, double fc, double fp, int t, int n, double h) {
    if (t == 0) return (fp - fc) / h;
    if (t == n - 1) return (fc - fm) / h;
    return (fp - fm) / (2. * h);
}

// fill round 2 fused with the force field and its sums
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_force(PArgs a, const double *__restrict__ st, double mu, double rho,
                                                        CV3 F, const uint8_t *__restrict__ M, CV3 L,
                                                        const uint8_t *__restrict__ code, V3 O,
                                                        double *__restrict__ part, unsigned npart) {
    const bool fill = st[F_BULK] != 0.0;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned i = p.i + e;
            const int x = p.x + e;
            double lap[3] = {L.c[0][i], L.c[1][i], L.c[2][i]};
            if (fill && code[i] == C_OPEN) (void)fill_average(wrapped(a, i, x, p.y, p.z), code, C_FILL1, L, lap);
            double f[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) f[k] = mu * lap[k];
            const double vel[3] = {F.c[0][i], F.c[1][i], F.c[2][i]};
            if (rho > 0.0) {
                const Clamp c = clamped(a, i, x, p.y, p.z);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double *__restrict__ g = F.c[k];
                    const double gx = grad1(g[c.xm], vel[k], g[c.xp], x, a.nx, a.h[0]);
                    const double gy = grad1(g[c.ym], vel[k], g[c.yp], p.y, a.ny, a.h[1]);
                    const double gz = grad1(g[c.zm], vel[k], g[c.zp], p.z, a.nz, a.h[2]);
                    const double adv = (vel[0] * gx + vel[1] * gy) + vel[2] * gz;
                    f[k] = f[k] - rho * adv;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) O.c[k][i] = f[k];
            if (M[i]) {
                s[0] += fabs(f[0]);
                s[1] += fabs(f[1]);
                s[2] += fabs(f[2]);
                s[3] += vel[2];
                s[4] += 1.0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double r = block_sum(s[k]);
        if (threadIdx.x == 0) part[k * npart + blockIdx.x] = r;
    }
}

// the face value between a voxel and its next one along an axis (physics.py:227-244)
__device__ __forceinline__ double face(double fc, double fn, bool mc, bool mn, bool inhom) {
    if (mc && mn) return 0.5 * (fc + fn);
    if (inhom && mc) return fc;
    if (inhom && mn) return fn;
    return 0.0;
}
// (face_i - face_{i-1}) / h at position t of n; the faces outside the array are 0
__device__ __forceinline__ double flux_term(const double *__restrict__ f, const uint8_t *__restrict__ M, unsigned i,
                                            unsigned stride, int t, int n, double h, bool inhom) {
    const double fc = f[i];
    const bool mc = M[i] != 0;
    const double hi = t + 1 < n ? face(fc, f[i + stride], mc, M[i + stride] != 0, inhom) : 0.0;
    const double lo = t > 0 ? face(f[i - stride], fc, M[i - stride] != 0, mc, inhom) : 0.0;
    return (hi - lo) / h;
}

// force divergence at every voxel (physics.py:211-262): x term + y term + z term
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_fdiv(PArgs a, int inhom, CV3 F, const uint8_t *__restrict__ M,
                                                       double *__restrict__ D) {
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        DV<VEC> d;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned i = p.i + e;
            const double tx = flux_term(F.c[0], M, i, 1u, p.x + e, a.nx, a.h[0], inhom != 0);
            const double ty = flux_term(F.c[1], M, i, (unsigned)a.nx, p.y, a.ny, a.h[1], inhom != 0);
            const double tz = flux_term(F.c[2], M, i, a.plane, p.z, a.nz, a.h[2], inhom != 0);
            d.e[e] = (tx + ty) + tz;
        }
        std_<VEC>(D + p.i, d);
    }
}

// Dir = the fluid voxels of plane z
__global__ __launch_bounds__(kGridThreads) void k_anchor(GridDims a, unsigned z, const uint8_t *__restrict__ M,
                                                         uint8_t *__restrict__ Dir) {
    const unsigned i = blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= a.n) return;
    Dir[i] = (i / a.plane == z && M[i]) ? 1 : 0;
}

template <int VEC>
__device__ __forceinline__ MV<VEC> active_of(const uint8_t *__restrict__ M, const uint8_t *__restrict__ Dir,
                                             unsigned i) {
    MV<VEC> m = ldmk<VEC>(M + i);
    if (Dir) {
        const MV<VEC> d = ldmk<VEC>(Dir + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) m.e[e] = (m.e[e] && !d.e[e]) ? 1 : 0;
    }
    return m;
}

// x = 0, r = b at active voxels (0 elsewhere); partial sums of b^2, Dirichlet and fluid counts
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_pinit(PArgs a, const double *__restrict__ B,
                                                        const uint8_t *__restrict__ M,
                                                        const uint8_t *__restrict__ Dir, double *__restrict__ X,
                                                        double *__restrict__ R, double *__restrict__ part,
                                                        unsigned npart) {
    double ss = 0.0, nd = 0.0, nf = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i), act = active_of<VEC>(M, Dir, p.i);
        DV<VEC> b = ldd<VEC>(B + p.i), z;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            z.e[e] = 0.0;
            b.e[e] = act.e[e] ? b.e[e] : 0.0;
            ss += b.e[e] * b.e[e];
            nf += mc.e[e] ? 1.0 : 0.0;
            nd += (mc.e[e] && !act.e[e]) ? 1.0 : 0.0;
        }
        std_<VEC>(R + p.i, b);
        std_<VEC>(X + p.i, z);
    }
    ss = block_sum(ss);
    nd = block_sum(nd);
    nf = block_sum(nf);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = ss;
        part[npart + blockIdx.x] = nd;
        part[2 * npart + blockIdx.x] = nf;
    }
}

// p' = r + beta p on active voxels (into Pn), q = A p', partial sums of p' q.  Neighbour offsets are
// clamped at the domain faces, so every load is in bounds and unconditional; a face or solid
// neighbour's term is dropped.  Term order: x-, x+, y-, y+, z-, z+ (physics.py:76-77).
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_pq(PArgs a, const double *__restrict__ st,
                                                     const double *__restrict__ R, const double *__restrict__ P,
                                                     double *__restrict__ Pn, double *__restrict__ Q,
                                                     const uint8_t *__restrict__ M, const uint8_t *__restrict__ Dir,
                                                     double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    const double beta = st[S_BETA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> act = active_of<VEC>(M, Dir, i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || act.e[e];
        if (!any) continue;
        const bool xl = p.x > 0, xh = p.x + VEC < a.nx, yl = p.y > 0, yh = p.y + 1 < a.ny, zl = p.z > 0,
                   zh = p.z + 1 < a.nz;
        const unsigned il = i - (xl ? 1u : 0u), ir = i + VEC - 1 + (xh ? 1u : 0u);
        const unsigned oym = yl ? (unsigned)a.nx : 0u, oyp = yh ? (unsigned)a.nx : 0u;
        const unsigned ozm = zl ? a.plane : 0u, ozp = zh ? a.plane : 0u;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        const uint8_t ml = M[il], mr = M[ir];
        const MV<VEC> mym = ldmk<VEC>(M + i - oym), myp = ldmk<VEC>(M + i + oyp);
        const MV<VEC> mzm = ldmk<VEC>(M + i - ozm), mzp = ldmk<VEC>(M + i + ozp);
        const DV<VEC> rc = ldd<VEC>(R + i), pc = ldd<VEC>(P + i);
        const double cl = R[il] + beta * P[il], cr = R[ir] + beta * P[ir];
        DV<VEC> ym = ldd<VEC>(R + i - oym), yp = ldd<VEC>(R + i + oyp);
        DV<VEC> zm = ldd<VEC>(R + i - ozm), zp = ldd<VEC>(R + i + ozp);
        const DV<VEC> pym = ldd<VEC>(P + i - oym), pyp = ldd<VEC>(P + i + oyp);
        const DV<VEC> pzm = ldd<VEC>(P + i - ozm), pzp = ldd<VEC>(P + i + ozp);
        DV<VEC> c, q;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            // an inactive voxel's r and p are 0, so the owners' expression gives the neighbours 0 too
            c.e[e] = act.e[e] ? rc.e[e] + beta * pc.e[e] : 0.0;
            ym.e[e] = ym.e[e] + beta * pym.e[e];
            yp.e[e] = yp.e[e] + beta * pyp.e[e];
            zm.e[e] = zm.e[e] + beta * pzm.e[e];
            zp.e[e] = zp.e[e] + beta * pzp.e[e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double xi = c.e[e];
            const bool hasl = e > 0 ? true : xl, hasr = e + 1 < VEC ? true : xh;
            const double vl = e > 0 ? c.e[e > 0 ? e - 1 : 0] : cl;
            const double vr = e + 1 < VEC ? c.e[e + 1 < VEC ? e + 1 : e] : cr;
            const bool fl = (e > 0 ? mc.e[e > 0 ? e - 1 : 0] : ml) != 0;
            const bool fr = (e + 1 < VEC ? mc.e[e + 1 < VEC ? e + 1 : e] : mr) != 0;
            double acc = 0.0;
            if (hasl && fl) acc += (vl - xi) * a.ih2[0];
            if (hasr && fr) acc += (vr - xi) * a.ih2[0];
            if (yl && mym.e[e]) acc += (ym.e[e] - xi) * a.ih2[1];
            if (yh && myp.e[e]) acc += (yp.e[e] - xi) * a.ih2[1];
            if (zl && mzm.e[e]) acc += (zm.e[e] - xi) * a.ih2[2];
            if (zh && mzp.e[e]) acc += (zp.e[e] - xi) * a.ih2[2];
            q.e[e] = act.e[e] ? acc : 0.0;
            if (act.e[e]) ss += xi * acc;
        }
        std_<VEC>(Pn + i, c);
        std_<VEC>(Q + i, q);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// k_pq for the preconditioned solve: p' = z + beta p on active voxels (into Pn), q = A p', partial sums
// of p' q, with q in the form of the assembled matrix the oracle multiplies by, so that the product
// is scipy's bits: the diagonal d = 0 + h^-2 of every fluid neighbour inside the domain in the order
// x-, x+, y-, y+, z-, z+ (Dirichlet ones included: their columns are eliminated, their count stays),
// and the row sum in ascending column order, q = 0 + w p'(z-) + w p'(y-) + w p'(x-) + (-d) p' + w p'(x+)
// + w p'(y+) + w p'(z+).  A Dirichlet neighbour's p' is 0 and adds nothing.  The plain solve keeps
// k_pq's difference form, which its own oracle (the slice operator) has.
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_pqm(PArgs a, const double *__restrict__ st,
                                                      const double *__restrict__ Z, const double *__restrict__ P,
                                                      double *__restrict__ Pn, double *__restrict__ Q,
                                                      const uint8_t *__restrict__ M, const uint8_t *__restrict__ Dir,
                                                      double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    const double beta = st[S_BETA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> act = active_of<VEC>(M, Dir, p.i);
        const DV<VEC> zc = ldd<VEC>(Z + p.i), pc = ldd<VEC>(P + p.i);
        DV<VEC> c, q;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned i = p.i + e;
            const int x = p.x + e;
            c.e[e] = 0.0;
            q.e[e] = 0.0;
            if (!act.e[e]) continue;
            const double xi = zc.e[e] + beta * pc.e[e];
            const Clamp n = clamped(a, i, x, p.y, p.z);
            // a clamped index is the voxel itself: the face is then outside the domain
            const bool fxm = n.xm != i && M[n.xm], fxp = n.xp != i && M[n.xp], fym = n.ym != i && M[n.ym],
                       fyp = n.yp != i && M[n.yp], fzm = n.zm != i && M[n.zm], fzp = n.zp != i && M[n.zp];
            double d = 0.0;
            if (fxm) d += a.ih2[0];
            if (fxp) d += a.ih2[0];
            if (fym) d += a.ih2[1];
            if (fyp) d += a.ih2[1];
            if (fzm) d += a.ih2[2];
            if (fzp) d += a.ih2[2];
            // an inactive voxel's z and p are 0, so the owners' expression gives the neighbours 0 too
            double acc = 0.0;
            if (fzm) acc += a.ih2[2] * (Z[n.zm] + beta * P[n.zm]);
            if (fym) acc += a.ih2[1] * (Z[n.ym] + beta * P[n.ym]);
            if (fxm) acc += a.ih2[0] * (Z[n.xm] + beta * P[n.xm]);
            acc += (-d) * xi;
            if (fxp) acc += a.ih2[0] * (Z[n.xp] + beta * P[n.xp]);
            if (fyp) acc += a.ih2[1] * (Z[n.yp] + beta * P[n.yp]);
            if (fzp) acc += a.ih2[2] * (Z[n.zp] + beta * P[n.zp]);
            c.e[e] = xi;
            q.e[e] = acc;
            ss += xi * acc;
        }
        std_<VEC>(Pn + p.i, c);
        std_<VEC>(Q + p.i, q);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// x += alpha p;  r -= alpha q;  partial sums of the new r^2
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_pxr(PArgs a, const double *__restrict__ st,
                                                      const double *__restrict__ P, const double *__restrict__ Q,
                                                      double *__restrict__ X, double *__restrict__ R,
                                                      const uint8_t *__restrict__ M, const uint8_t *__restrict__ Dir,
                                                      double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    const double alpha = st[S_ALPHA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> act = active_of<VEC>(M, Dir, i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || act.e[e];
        if (!any) continue;
        const DV<VEC> pc = ldd<VEC>(P + i), qc = ldd<VEC>(Q + i);
        DV<VEC> x = ldd<VEC>(X + i), r = ldd<VEC>(R + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (!act.e[e]) continue;
            x.e[e] = x.e[e] + alpha * pc.e[e];
            r.e[e] = r.e[e] - alpha * qc.e[e];
            ss += r.e[e] * r.e[e];
        }
        std_<VEC>(X + i, x);
        std_<VEC>(R + i, r);
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// the output: x at active voxels, 0 at solid and Dirichlet voxels; NaN at every fluid voxel when the
// right-hand side held one (scipy's x += alpha p with alpha = NaN reaches the Dirichlet entries too)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_pout(PArgs a, const double *__restrict__ st,
                                                       const double *__restrict__ X, const uint8_t *__restrict__ M,
                                                       const uint8_t *__restrict__ Dir, double *__restrict__ O) {
    const bool nan = st[S_NAN] != 0.0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const MV<VEC> mc = ldmk<VEC>(M + p.i), act = active_of<VEC>(M, Dir, p.i);
        DV<VEC> x = ldd<VEC>(X + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x.e[e] = !mc.e[e] ? 0.0 : nan ? qnan : act.e[e] ? x.e[e] : 0.0;
        std_<VEC>(O + p.i, x);
    }
}

// Second reduction stage and the scalar steps.  One block sums the partials in a fixed order, then
// thread 0 alone advances the state: cg_step (PH_INIT also stores the Dirichlet and fluid counts),
// or the force pass's sums.
__global__ __launch_bounds__(kGridFinalThreads) void k_pcg_scalar(int phase, CgCfg cfg, double *__restrict__ st,
                                                                   const double *__restrict__ part, unsigned npart) {
    if (in_iteration(phase) && st[S_STOP] != 0.0) return;
    double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int rows = phase == PH_FORCE ? 5 : phase == PH_INIT ? 3 : phase == PH_TOP0 ? 0 : 1;
    for (int k = 0; k < rows; ++k) r[k] = partial_sum(part + k * npart, npart);
    if (threadIdx.x != 0) return;
    if (phase == PH_BULK) {
        st[F_BULK] = r[0];
    } else if (phase == PH_FORCE) {
        st[F_SFX] = r[0];
        st[F_SFY] = r[1];
        st[F_SFZ] = r[2];
        st[F_SW] = r[3];
        st[F_NFLUID] = r[4];
    } else {
        cg_step(phase, cfg, st, r[0]);
        if (phase == PH_INIT) {
            st[S_NDIR] = r[1];
            st[S_NFLUID] = r[2];
        }
    }
}

// partial sums of r z (the preconditioned solve's rho); both are 0 at every voxel that is not active
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_rz(PArgs a, const double *__restrict__ st,
                                                     const double *__restrict__ R, const double *__restrict__ Z,
                                                     double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const DV<VEC> r = ldd<VEC>(R + p.i), z = ldd<VEC>(Z + p.i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) ss += r.e[e] * z.e[e];
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// the second stage and the scalar step of the preconditioned recurrence's own phases
__global__ __launch_bounds__(kGridFinalThreads) void k_ppcg_scalar(int phase, CgCfg cfg, double *__restrict__ st,
                                                                    const double *__restrict__ part, unsigned npart) {
    if (pcg_in_iteration(phase) && st[S_STOP] != 0.0) return;
    const double r0 = phase == PH_PTOP0 ? 0.0 : partial_sum(part, npart);
    if (threadIdx.x != 0) return;
    pcg_step(phase, cfg, st, S_RZ, r0);
}

int make_args(const GridSpec &g, PArgs &a) {
    PTV_TRY(grid_dims("pressure", g.nx, g.ny, g.nz, a));
    if (!(g.dx > 0.0) || !(g.dy > 0.0) || !(g.dz > 0.0) || !std::isfinite(g.dx) || !std::isfinite(g.dy) ||
        !std::isfinite(g.dz)) {
        set_error("pressure: spacings must be positive finite numbers");
        return PTV_E_ARG;
    }
    const double h[3] = {g.dx, g.dy, g.dz};
    for (int k = 0; k < 3; ++k) {
        a.h[k] = h[k];
        a.h2[k] = h[k] * h[k];
        a.ih2[k] = 1.0 / (h[k] * h[k]);
    }
    return PTV_OK;
}

int scalar(PressWork &wk, int phase, const CgCfg &cfg, unsigned nb, hipStream_t s) {
    hipLaunchKernelGGL(k_pcg_scalar, dim3(1), dim3(kGridFinalThreads), 0, s, phase, cfg, wk.state.p, wk.part.p, nb);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

}  // namespace

int press_force(PressWork &wk, const GridSpec &g, double mu, double rho, const uint8_t *M, const double *U,
                const double *V, const double *W, double *Fx, double *Fy, double *Fz, hipStream_t s,
                ptv_pressure_stats *st) {
    PArgs a{};
    PTV_TRY(make_args(g, a));
    if (!std::isfinite(mu) || !std::isfinite(rho)) {
        set_error("pressure: mu and rho must be finite");
        return PTV_E_ARG;
    }
    if (rho > 0.0 && (a.nx < 2 || a.ny < 2 || a.nz < 2)) {
        set_error("pressure: rho > 0 needs at least 2 voxels along every axis (np.gradient)");
        return PTV_E_ARG;
    }
    const size_t n = a.n;
    // the stencil passes address single elements: one x per lane serves every alignment
    const unsigned nb = blocks_for(a.n, 1);
    PTV_TRY(wk.lap.ensure(3 * n));
    PTV_TRY(wk.code.ensure(n));
    PTV_TRY(wk.part.ensure(5 * (size_t)nb));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen));
    double *h_final = wk.h_state.p + 2 * kStateLen;
    const CgCfg cfg{0.0, 0};
    const V3 L = parts(wk.lap.p, n);
    const CV3 cL = cparts(wk.lap.p, n), F{{U, V, W}};
    PTV_TRY(record_event(wk.ev, 0, s));
    hipLaunchKernelGGL(k_lap<1>, dim3(nb), dim3(kGridThreads), 0, s, a, F, M, L, wk.code.p, wk.part.p);
    PTV_HIP(hipGetLastError());
    PTV_TRY(scalar(wk, PH_BULK, cfg, nb, s));
    hipLaunchKernelGGL(k_fill<1>, dim3(nb), dim3(kGridThreads), 0, s, a, (const double *)wk.state.p, L, wk.code.p);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_force<1>, dim3(nb), dim3(kGridThreads), 0, s, a, (const double *)wk.state.p, mu, rho, F, M,
                       cL, (const uint8_t *)wk.code.p, V3{{Fx, Fy, Fz}}, wk.part.p, nb);
    PTV_HIP(hipGetLastError());
    PTV_TRY(scalar(wk, PH_FORCE, cfg, nb, s));
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, kStateLen * sizeof(double), hipMemcpyDeviceToHost, s));
    PTV_TRY(record_event(wk.ev, 1, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (st) {
        st->n_fluid = (int64_t)h_final[F_NFLUID];
        st->sum_abs_fx = h_final[F_SFX];
        st->sum_abs_fy = h_final[F_SFY];
        st->sum_abs_fz = h_final[F_SFZ];
        st->sum_w = h_final[F_SW];
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, wk.ev[0], wk.ev[1]));
        st->ms_force = ms;
    }
    return PTV_OK;
}

int press_divergence(const GridSpec &g, bool inhomogeneous, const uint8_t *M, const double *Fx, const double *Fy,
                     const double *Fz, double *D, hipStream_t s) {
    PArgs a{};
    PTV_TRY(make_args(g, a));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(D);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    GRID_LAUNCH(k_fdiv, vec2, nb, s, a, inhomogeneous ? 1 : 0, CV3{{Fx, Fy, Fz}}, M, D);
    return PTV_OK;
}

int press_anchor_plane(const GridSpec &g, int z, const uint8_t *M, uint8_t *Dir, hipStream_t s) {
    PArgs a{};
    PTV_TRY(make_args(g, a));
    if (z < 0 || z >= a.nz) {
        set_error("pressure: the anchor plane lies outside the grid");
        return PTV_E_ARG;
    }
    const unsigned nb = (a.n + kGridThreads - 1) / kGridThreads;
    hipLaunchKernelGGL(k_anchor, dim3(nb), dim3(kGridThreads), 0, s, (GridDims)a, (unsigned)z, M, Dir);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

int press_cg(PressWork &wk, const GridSpec &g, double rtol, int maxiter, const uint8_t *M, const uint8_t *Dir,
             const double *B, double *X, hipStream_t s, ptv_pressure_stats *st) {
    PArgs a{};
    PTV_TRY(make_args(g, a));
    if (!std::isfinite(rtol) || maxiter < 0) {
        set_error("pressure: rtol must be finite and maxiter non-negative");
        return PTV_E_ARG;
    }
    const size_t n = a.n, nbytes = n * sizeof(double);
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(B, X) && aligned(M, 2) && (!Dir || aligned(Dir, 2));
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    for (DevBuf<double> *b : {&wk.x, &wk.r, &wk.p[0], &wk.p[1], &wk.q}) PTV_TRY(b->ensure(n));
    PTV_TRY(wk.part.ensure(5 * (size_t)blocks_for(a.n, 1)));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen));
    double *h_final = wk.h_state.p + 2 * kStateLen;
    const size_t sbytes = kStateLen * sizeof(double);
    const CgCfg cfg{rtol, maxiter};
    const double *cst = wk.state.p;

    PTV_TRY(record_event(wk.ev, 2, s));
    PTV_HIP(hipMemsetAsync(wk.p[0].p, 0, nbytes, s));
    PTV_HIP(hipMemsetAsync(wk.p[1].p, 0, nbytes, s));
    PTV_HIP(hipMemsetAsync(wk.q.p, 0, nbytes, s));
    GRID_LAUNCH(k_pinit, vec2, nb, s, a, B, M, Dir, wk.x.p, wk.r.p, wk.part.p, nb);
    PTV_TRY(scalar(wk, PH_INIT, cfg, nb, s));
    PTV_TRY(record_event(wk.ev, 3, s));
    int cur = 0;  // p[cur] holds the last direction
    std::vector<int> batch_iters;
    PTV_TRY(poll_batches(s, wk.state.p, wk.h_state.p, kStateLen, wk.ev, maxiter, [&](int it) -> int {
        PTV_TRY(scalar(wk, it == 0 ? PH_TOP0 : PH_TOP, cfg, nb, s));
        GRID_LAUNCH(k_pq, vec2, nb, s, a, cst, (const double *)wk.r.p, (const double *)wk.p[cur].p, wk.p[cur ^ 1].p,
                    wk.q.p, M, Dir, wk.part.p);
        cur ^= 1;
        PTV_TRY(scalar(wk, PH_ALPHA, cfg, nb, s));
        GRID_LAUNCH(k_pxr, vec2, nb, s, a, cst, (const double *)wk.p[cur].p, (const double *)wk.q.p, wk.x.p, wk.r.p, M,
                    Dir, wk.part.p);
        return PTV_OK;
    }, batch_iters));
    const size_t batches = batch_iters.size();
    PTV_TRY(scalar(wk, PH_END, cfg, nb, s));
    PTV_TRY(record_event(wk.ev, 4 + batches, s));
    GRID_LAUNCH(k_pout, vec2, nb, s, a, cst, (const double *)wk.x.p, M, Dir, X);
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, sbytes, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    if (st) {
        st->solver = 0;
        st->itn = (int32_t)h_final[S_ITN];
        st->info = (int32_t)h_final[S_INFO];
        st->bnorm = h_final[S_BNORM];
        st->rnorm = sqrt(h_final[S_RR]);
        st->n_fluid = (int64_t)h_final[S_NFLUID];
        st->n_dirichlet = (int64_t)h_final[S_NDIR];
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, wk.ev[2], wk.ev[4 + batches]));
        st->ms_solve = ms;
        PTV_TRY(median_iter_ms(wk.ev, 3, batch_iters, st->itn, st->ms_solve, st->ms_iter_median));
    }
    return PTV_OK;
}

// One iteration (scipy _isolve/iterative.py, cg with M):
//     k_ppcg_scalar PTOP:  rr = sum r^2;  ||r|| < rtol ||b|| stops, info 0
//     mg_vcycle:           z = M r  (q is its level-0 scratch: nothing reads q before k_pqm rewrites it)
//     k_rz, PRHO:          rho = sum r z, beta = rho / rho_prev
//     k_pqm:               p' = z + beta p,  q = A p' in the assembled matrix's form,  partial sums of p' q
//     k_pcg_scalar ALPHA, k_pxr: as in press_cg
// The first V-cycle of every polling batch is timed (events 4 + 2 b, 5 + 2 b of the multigrid work).
int press_pcg(PressWork &wk, MgWork &mg, const MgPlan &plan, const GridSpec &g, double rtol, int maxiter,
              const uint8_t *M, const uint8_t *Dir, const double *B, double *X, hipStream_t s,
              ptv_pressure_stats *st, ptv_mg_stats *mst) {
    PArgs a{};
    PTV_TRY(make_args(g, a));
    if (!std::isfinite(rtol) || maxiter < 0) {
        set_error("pressure: rtol must be finite and maxiter non-negative");
        return PTV_E_ARG;
    }
    if (!Dir) {
        set_error("pressure: the preconditioned solve needs a Dirichlet grid");
        return PTV_E_UNSUPPORTED;
    }
    const size_t n = a.n, nbytes = n * sizeof(double);
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(B, X) && aligned(M, 2) && aligned(Dir, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    for (DevBuf<double> *b : {&wk.x, &wk.r, &wk.p[0], &wk.p[1], &wk.q, &wk.z}) PTV_TRY(b->ensure(n));
    PTV_TRY(wk.part.ensure(5 * (size_t)blocks_for(a.n, 1)));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen));
    double *h_final = wk.h_state.p + 2 * kStateLen;
    const size_t sbytes = kStateLen * sizeof(double);
    const CgCfg cfg{rtol, maxiter};
    const double *cst = wk.state.p;
    auto pscalar = [&](int phase) -> int {
        hipLaunchKernelGGL(k_ppcg_scalar, dim3(1), dim3(kGridFinalThreads), 0, s, phase, cfg, wk.state.p, wk.part.p, nb);
        PTV_HIP(hipGetLastError());
        return PTV_OK;
    };

    PTV_TRY(record_event(wk.ev, 2, s));
    PTV_TRY(mg_setup(mg, plan, M, Dir, s));
    PTV_HIP(hipMemsetAsync(wk.p[0].p, 0, nbytes, s));
    PTV_HIP(hipMemsetAsync(wk.p[1].p, 0, nbytes, s));
    PTV_HIP(hipMemsetAsync(wk.q.p, 0, nbytes, s));
    GRID_LAUNCH(k_pinit, vec2, nb, s, a, B, M, Dir, wk.x.p, wk.r.p, wk.part.p, nb);
    PTV_TRY(scalar(wk, PH_INIT, cfg, nb, s));
    PTV_TRY(record_event(wk.ev, 3, s));
    int cur = 0;  // p[cur] holds the last direction
    std::vector<int> batch_iters;
    PTV_TRY(poll_batches(s, wk.state.p, wk.h_state.p, kStateLen, wk.ev, maxiter, [&](int it) -> int {
        PTV_TRY(pscalar(it == 0 ? PH_PTOP0 : PH_PTOP));
        const bool timed = it % kPoll == 0;
        if (timed) PTV_TRY(record_event(mg.ev, 4 + 2 * (size_t)(it / kPoll), s));
        PTV_TRY(mg_vcycle(mg, plan, M, Dir, cst, wk.r.p, wk.z.p, wk.q.p, s));
        if (timed) PTV_TRY(record_event(mg.ev, 5 + 2 * (size_t)(it / kPoll), s));
        GRID_LAUNCH(k_rz, vec2, nb, s, a, cst, (const double *)wk.r.p, (const double *)wk.z.p, wk.part.p);
        PTV_TRY(pscalar(PH_PRHO));
        GRID_LAUNCH(k_pqm, vec2, nb, s, a, cst, (const double *)wk.z.p, (const double *)wk.p[cur].p, wk.p[cur ^ 1].p,
                    wk.q.p, M, Dir, wk.part.p);
        cur ^= 1;
        PTV_TRY(scalar(wk, PH_ALPHA, cfg, nb, s));
        GRID_LAUNCH(k_pxr, vec2, nb, s, a, cst, (const double *)wk.p[cur].p, (const double *)wk.q.p, wk.x.p, wk.r.p, M,
                    Dir, wk.part.p);
        return PTV_OK;
    }, batch_iters));
    const size_t batches = batch_iters.size();
    PTV_TRY(scalar(wk, PH_END, cfg, nb, s));
    PTV_TRY(record_event(wk.ev, 4 + batches, s));
    GRID_LAUNCH(k_pout, vec2, nb, s, a, cst, (const double *)wk.x.p, M, Dir, X);
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, sbytes, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    const int itn = (int)h_final[S_ITN];
    if (st) {
        st->solver = 0;
        st->itn = itn;
        st->info = (int32_t)h_final[S_INFO];
        st->bnorm = h_final[S_BNORM];
        st->rnorm = sqrt(h_final[S_RR]);
        st->n_fluid = (int64_t)h_final[S_NFLUID];
        st->n_dirichlet = (int64_t)h_final[S_NDIR];
        float ms = 0.f;
        PTV_HIP(hipEventElapsedTime(&ms, wk.ev[2], wk.ev[4 + batches]));
        st->ms_solve = ms;
        PTV_TRY(median_iter_ms(wk.ev, 3, batch_iters, st->itn, st->ms_solve, st->ms_iter_median));
    }
    if (mst) {
        PTV_TRY(mg_fill_stats(mg, plan, mst));
        std::vector<double> per;  // the timed V-cycles that ran: those of the batches begun before the stop
        for (size_t b = 0; b < batches && (int)(b * kPoll) < itn; ++b) {
            float ms = 0.f;
            PTV_HIP(hipEventElapsedTime(&ms, mg.ev[4 + 2 * b], mg.ev[5 + 2 * b]));
            per.push_back(ms);
        }
        std::sort(per.begin(), per.end());
        mst->ms_vcycle_median = per.empty() ? 0.0 : per[per.size() / 2];
    }
    return PTV_OK;
}

}  // namespace ptv
