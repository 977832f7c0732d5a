// ptv_variational.hip — variational divergence cleaning: matrix-free CG on I + lambda D^T D.
//
// Restates physics.clean_divergence_variational (physics.py:440-514): the divergence operators of
// build_divergence_operators (:356-438), the system (I + lambda D^T D) x = (u, v, w)[fluid]
// (:460-480) and scipy.sparse.linalg.cg(A, b, rtol=1e-8, atol=0, maxiter=2000) (:485, `tol` in the
// reference's spelling).  The reference assembles three CSR operators, six sparse products and a
// 3n x 3n block matrix; here nothing is assembled.
//
// Per axis with spacing h, ch = 0.5 / h and eh = 1.0 / h (each rounded once), and for a fluid voxel
// i with neighbours i+ and i- along the axis, n+ = (i+ inside the grid and fluid), e+ = (i+ outside
// the grid), n-, e- likewise:
//     c_i        = n+ ch + e+ eh - n- ch - e- eh                       (exact)
//     (D v)_i    = c_i v_i + n+ ch v_{i+} - n- ch v_{i-}
//     (D^T d)_j  = c_j d_j + n- ch d_{j-} - n+ ch d_{j+}
//     A x        = x + lambda D^T (Dx x_u + Dy x_v + Dz x_w)
//
// Storage as in ptv_clean.hip: x, r, p, q are three dense float64 (nz, ny, nx) grids each, d is
// one; the uint8 mask is applied in the kernels, solid entries stay 0 and no sum sees them.
//
// One CG iteration (scipy _isolve/iterative.py, cg) is three streaming passes and two one-block
// scalar kernels on device-resident state:
//     k_scalar TOP:    rr = sum r^2 (partials of the last pass);  ||r|| < rtol ||b|| stops, info 0;
//                      else rho = rr, beta = rho / rho_prev
//     k_dir:           p' = r + beta p,  d = D p'
//     k_q:             q = p' + lambda D^T d,  partial sums of p' q
//     k_scalar ALPHA:  alpha = rho / sum p' q
//     k_xr:            x += alpha p',  r -= alpha q,  partial sums of r^2
// k_dir reads p and writes p' to a second buffer (the two swap every iteration): a lane needs p' at
// its neighbours, which it recomputes from r and p with the expression their owners use, so the
// update is fused with the stencil without a race.
// Bytes per voxel and iteration: k_dir 24 r + 24 p + 24 p' + 8 d + 1 mask = 81; k_q 8 d + 24 p' +
// 24 q + 1 = 57; k_xr 24 x + 24 p' + 24 r + 24 q reads, 24 x + 24 r writes + 1 = 145; 283 in all
// (stencil neighbours come from the cache lines of adjacent lanes and rows).
//
// Reductions are the two-stage fixed-order sums of ptv_grid_vec.hpp: no floating-point atomics, a
// call repeats bit for bit.  The scalar recurrence with its stopping rules, the stop flag and the
// polling loop are those of ptv_grid_solve.hpp.
#include <cmath>
#include <algorithm>

#include "ptv_variational.hpp"
#include "ptv_grid_solve.hpp"

namespace ptv {

namespace {

using namespace cg;

// device-resident state (doubles): the CG recurrence, then the report's slots
enum { S_NFLUID = S_CG_COUNT, S_DIV0, S_DIV1, S_COUNT };
constexpr int kStateLen = 16;
static_assert(S_COUNT <= kStateLen, "state length");

enum { PH_DIV = PH_CG_COUNT };

struct VarArgs : GridDims {
    double ch[3], eh[3];  // 0.5 / h and 1.0 / h for x, y, z (physics.py:406-414)
    double lambda;
};

// The stencil of a group: which neighbours are fluid voxels inside the grid, the diagonal
// coefficients, and the neighbour offsets, clamped at the domain faces so that every load is in
// bounds and unconditional (a clamped load's value is never used).
template <int VEC>
struct Nbr {
    bool fm[3][VEC], fp[3][VEC];  // fluid neighbour on the minus / plus side; axis 0 x, 1 y, 2 z
    double c[3][VEC];
    unsigned il, ir;              // index of the x neighbours of the group's first / last element
    unsigned oym, oyp, ozm, ozp;  // offsets of the y and z neighbours
};

__device__ __forceinline__ double diag_coef(bool fp, bool outp, bool fm, bool outm, double ch, double eh) {
    double c = 0.0;
    c += fp ? ch : 0.0;
    c += outp ? eh : 0.0;
    c -= fm ? ch : 0.0;
    c -= outm ? eh : 0.0;
    return c;
}

template <int VEC>
__device__ __forceinline__ Nbr<VEC> neighbours(const VarArgs &a, const uint8_t *__restrict__ M, const Pos &p,
                                               const MV<VEC> &mc) {
    const bool xl = p.x > 0, xh = p.x + VEC < a.nx, yl = p.y > 0, yh = p.y + 1 < a.ny, zl = p.z > 0,
               zh = p.z + 1 < a.nz;
    Nbr<VEC> n;
    const unsigned i = p.i;
    n.il = i - (xl ? 1u : 0u);
    n.ir = i + VEC - 1 + (xh ? 1u : 0u);
    n.oym = yl ? (unsigned)a.nx : 0u;
    n.oyp = yh ? (unsigned)a.nx : 0u;
    n.ozm = zl ? a.plane : 0u;
    n.ozp = zh ? a.plane : 0u;
    const uint8_t ml = M[n.il], mr = M[n.ir];
    const MV<VEC> mym = ldmk<VEC>(M + i - n.oym), myp = ldmk<VEC>(M + i + n.oyp);
    const MV<VEC> mzm = ldmk<VEC>(M + i - n.ozm), mzp = ldmk<VEC>(M + i + n.ozp);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const bool inl = e > 0 ? true : xl, inr = e + 1 < VEC ? true : xh;
        n.fm[0][e] = inl && (e > 0 ? mc.e[e > 0 ? e - 1 : 0] : ml) != 0;
        n.fp[0][e] = inr && (e + 1 < VEC ? mc.e[e + 1 < VEC ? e + 1 : e] : mr) != 0;
        n.fm[1][e] = yl && mym.e[e] != 0;
        n.fp[1][e] = yh && myp.e[e] != 0;
        n.fm[2][e] = zl && mzm.e[e] != 0;
        n.fp[2][e] = zh && mzp.e[e] != 0;
        n.c[0][e] = diag_coef(n.fp[0][e], !inr, n.fm[0][e], !inl, a.ch[0], a.eh[0]);
        n.c[1][e] = diag_coef(n.fp[1][e], !yh, n.fm[1][e], !yl, a.ch[1], a.eh[1]);
        n.c[2][e] = diag_coef(n.fp[2][e], !zh, n.fm[2][e], !zl, a.ch[2], a.eh[2]);
    }
    return n;
}

// one axis of D v for element e: c v + n+ ch v+ - n- ch v-
__device__ __forceinline__ double div_term(double c, double v, bool fp, double vp, bool fm, double vm, double ch) {
    double s = c * v;
    if (fp) s += ch * vp;
    if (fm) s -= ch * vm;
    return s;
}
// one axis of D^T d for element e: c d + n- ch d- - n+ ch d+
__device__ __forceinline__ double adj_term(double c, double d, bool fm, double dm, bool fp, double dp, double ch) {
    double s = c * d;
    if (fm) s += ch * dm;
    if (fp) s -= ch * dp;
    return s;
}

// (Dx u + Dy v + Dz w) of a group from the centre values and the six neighbour values; 0 at solid
template <int VEC>
__device__ __forceinline__ DV<VEC> div_group(const VarArgs &a, const Nbr<VEC> &n, const MV<VEC> &mc,
                                             const DV<VEC> &cu, double ul, double ur, const DV<VEC> &cv,
                                             const DV<VEC> &vym, const DV<VEC> &vyp, const DV<VEC> &cw,
                                             const DV<VEC> &wzm, const DV<VEC> &wzp) {
    DV<VEC> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const double um = e > 0 ? cu.e[e > 0 ? e - 1 : 0] : ul;
        const double up = e + 1 < VEC ? cu.e[e + 1 < VEC ? e + 1 : e] : ur;
        const double sx = div_term(n.c[0][e], cu.e[e], n.fp[0][e], up, n.fm[0][e], um, a.ch[0]);
        const double sy = div_term(n.c[1][e], cv.e[e], n.fp[1][e], vyp.e[e], n.fm[1][e], vym.e[e], a.ch[1]);
        const double sz = div_term(n.c[2][e], cw.e[e], n.fp[2][e], wzp.e[e], n.fm[2][e], wzm.e[e], a.ch[2]);
        o.e[e] = mc.e[e] ? (sx + sy) + sz : 0.0;
    }
    return o;
}

// d = D x on the caller's three grids (ptv_divergence_operator_apply): solid entries of x are not used
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_var_div(VarArgs a, CV3 X, const uint8_t *__restrict__ M,
                                                          double *__restrict__ Dd) {
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        const Nbr<VEC> n = neighbours<VEC>(a, M, p, mc);
        const DV<VEC> cu = ldd<VEC>(X.c[0] + i), cv = ldd<VEC>(X.c[1] + i), cw = ldd<VEC>(X.c[2] + i);
        const double ul = X.c[0][n.il], ur = X.c[0][n.ir];
        const DV<VEC> vym = ldd<VEC>(X.c[1] + i - n.oym), vyp = ldd<VEC>(X.c[1] + i + n.oyp);
        const DV<VEC> wzm = ldd<VEC>(X.c[2] + i - n.ozm), wzp = ldd<VEC>(X.c[2] + i + n.ozp);
        std_<VEC>(Dd + i, div_group<VEC>(a, n, mc, cu, ul, ur, cv, vym, vyp, cw, wzm, wzp));
    }
}

// p' = r + beta p on fluid voxels (into Pn; P is last iteration's), d = D p'.  Neighbour values of
// p' are recomputed from R and P with the owner's expression.
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_dir(VarArgs a, const double *__restrict__ st, CV3 R, CV3 P, V3 Pn,
                                                      const uint8_t *__restrict__ M, double *__restrict__ Dd) {
    if (st[S_STOP] != 0.0) return;
    const double beta = st[S_BETA];
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || mc.e[e];
        if (!any) continue;
        const Nbr<VEC> n = neighbours<VEC>(a, M, p, mc);
        DV<VEC> c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const DV<VEC> r = ldd<VEC>(R.c[k] + i), po = ldd<VEC>(P.c[k] + i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) c[k].e[e] = mc.e[e] ? r.e[e] + beta * po.e[e] : 0.0;
        }
        const double ul = R.c[0][n.il] + beta * P.c[0][n.il], ur = R.c[0][n.ir] + beta * P.c[0][n.ir];
        DV<VEC> vym = ldd<VEC>(R.c[1] + i - n.oym), vyp = ldd<VEC>(R.c[1] + i + n.oyp);
        DV<VEC> wzm = ldd<VEC>(R.c[2] + i - n.ozm), wzp = ldd<VEC>(R.c[2] + i + n.ozp);
        const DV<VEC> pym = ldd<VEC>(P.c[1] + i - n.oym), pyp = ldd<VEC>(P.c[1] + i + n.oyp);
        const DV<VEC> pzm = ldd<VEC>(P.c[2] + i - n.ozm), pzp = ldd<VEC>(P.c[2] + i + n.ozp);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            vym.e[e] = vym.e[e] + beta * pym.e[e];
            vyp.e[e] = vyp.e[e] + beta * pyp.e[e];
            wzm.e[e] = wzm.e[e] + beta * pzm.e[e];
            wzp.e[e] = wzp.e[e] + beta * pzp.e[e];
        }
        const DV<VEC> d = div_group<VEC>(a, n, mc, c[0], ul, ur, c[1], vym, vyp, c[2], wzm, wzp);
#pragma unroll
        for (int k = 0; k < 3; ++k) std_<VEC>(Pn.c[k] + i, c[k]);
        std_<VEC>(Dd + i, d);
    }
}

// q = p + lambda D^T d on fluid voxels (0 at solid), partial sums of p q.  st == NULL: the operator
// call (ptv_variational_apply), which has no stop flag.
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_q(VarArgs a, const double *__restrict__ st,
                                                    const double *__restrict__ Dd, CV3 P, V3 Q,
                                                    const uint8_t *__restrict__ M, double *__restrict__ part) {
    if (st && st[S_STOP] != 0.0) return;
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || mc.e[e];
        if (!any) {
            if (!st) {  // the operator call writes every voxel of its output
                DV<VEC> z;
#pragma unroll
                for (int e = 0; e < VEC; ++e) z.e[e] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) std_<VEC>(Q.c[k] + i, z);
            }
            continue;
        }
        const Nbr<VEC> n = neighbours<VEC>(a, M, p, mc);
        const DV<VEC> dc = ldd<VEC>(Dd + i);
        const double dl = Dd[n.il], dr = Dd[n.ir];
        const DV<VEC> dym = ldd<VEC>(Dd + i - n.oym), dyp = ldd<VEC>(Dd + i + n.oyp);
        const DV<VEC> dzm = ldd<VEC>(Dd + i - n.ozm), dzp = ldd<VEC>(Dd + i + n.ozp);
        DV<VEC> pc[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) pc[k] = ldd<VEC>(P.c[k] + i);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double dm = e > 0 ? dc.e[e > 0 ? e - 1 : 0] : dl;
            const double dp = e + 1 < VEC ? dc.e[e + 1 < VEC ? e + 1 : e] : dr;
            const double t0 = adj_term(n.c[0][e], dc.e[e], n.fm[0][e], dm, n.fp[0][e], dp, a.ch[0]);
            const double t1 = adj_term(n.c[1][e], dc.e[e], n.fm[1][e], dym.e[e], n.fp[1][e], dyp.e[e], a.ch[1]);
            const double t2 = adj_term(n.c[2][e], dc.e[e], n.fm[2][e], dzm.e[e], n.fp[2][e], dzp.e[e], a.ch[2]);
            const bool own = mc.e[e] != 0;
            q[0].e[e] = own ? pc[0].e[e] + a.lambda * t0 : 0.0;
            q[1].e[e] = own ? pc[1].e[e] + a.lambda * t1 : 0.0;
            q[2].e[e] = own ? pc[2].e[e] + a.lambda * t2 : 0.0;
        }
        // summed in the order of k_init's b^2 and k_xr's r^2: with lambda = 0 (q = p = r) the sum is
        // rho bit for bit, alpha is 1 and the first step ends on r = 0 exactly
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (mc.e[e]) ss += pc[k].e[e] * q[k].e[e];
            std_<VEC>(Q.c[k] + i, q[k]);
        }
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// x += alpha p;  r -= alpha q;  partial sums of the new r^2 (iterative.py, cg)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_xr(VarArgs a, const double *__restrict__ st, CV3 P, CV3 Q, V3 X,
                                                     V3 R, const uint8_t *__restrict__ M,
                                                     double *__restrict__ part) {
    if (st[S_STOP] != 0.0) return;
    const double alpha = st[S_ALPHA];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        bool any = false;
#pragma unroll
        for (int e = 0; e < VEC; ++e) any = any || mc.e[e];
        if (!any) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const DV<VEC> pc = ldd<VEC>(P.c[k] + i), qc = ldd<VEC>(Q.c[k] + i);
            DV<VEC> x = ldd<VEC>(X.c[k] + i), r = ldd<VEC>(R.c[k] + i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (!mc.e[e]) continue;
                x.e[e] = x.e[e] + alpha * pc.e[e];
                r.e[e] = r.e[e] - alpha * qc.e[e];
                ss += r.e[e] * r.e[e];
            }
            std_<VEC>(X.c[k] + i, x);
            std_<VEC>(R.c[k] + i, r);
        }
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// x = 0, r = b = the fields at fluid voxels (0 at solid), partial sums of b^2
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_init(VarArgs a, CV3 F, const uint8_t *__restrict__ M, V3 X, V3 R,
                                                       double *__restrict__ part) {
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
        DV<VEC> z;
#pragma unroll
        for (int e = 0; e < VEC; ++e) z.e[e] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            DV<VEC> b = ldd<VEC>(F.c[k] + i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                b.e[e] = mc.e[e] ? b.e[e] : 0.0;
                ss += b.e[e] * b.e[e];
            }
            std_<VEC>(R.c[k] + i, b);
            std_<VEC>(X.c[k] + i, z);
        }
    }
    ss = block_sum(ss);
    if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

// the outputs: x at fluid voxels, 0 at solid (physics.py:494-500); NaN at every fluid voxel when
// the right-hand side held one (what the recurrence gives from its first step on)
template <int VEC>
__global__ __launch_bounds__(kGridThreads) void k_out(VarArgs a, const double *__restrict__ st, CV3 X,
                                                      const uint8_t *__restrict__ M, V3 O) {
    const bool nan = st[S_NAN] != 0.0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(a, it, p)) break;
        const unsigned i = p.i;
        const MV<VEC> mc = ldmk<VEC>(M + i);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            DV<VEC> x = ldd<VEC>(X.c[k] + i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) x.e[e] = mc.e[e] ? (nan ? qnan : x.e[e]) : 0.0;
            std_<VEC>(O.c[k] + i, x);
        }
    }
}

// Second reduction stage and the scalar step.  One block sums the partials in a fixed order, then
// thread 0 alone advances the state: cg_step, or the report's mean |div| into slot S_DIV0 + slot.
__global__ __launch_bounds__(kGridFinalThreads) void k_cg_scalar(int phase, CgCfg cfg, double *__restrict__ st,
                                                                  const double *__restrict__ part, unsigned npart,
                                                                  int slot) {
    if (in_iteration(phase) && st[S_STOP] != 0.0) return;
    double r0 = 0.0, r1 = 0.0;
    if (phase == PH_DIV) {
        r0 = partial_sum(part + npart, npart);      // sum |div|
        r1 = partial_sum(part + 2 * npart, npart);  // fluid voxels
    } else if (phase != PH_TOP0) {
        r0 = partial_sum(part, npart);
    }
    if (threadIdx.x != 0) return;
    if (phase == PH_DIV) {
        st[S_NFLUID] = r1;
        st[S_DIV0 + slot] = r0 / r1;
    } else {
        cg_step(phase, cfg, st, r0);
    }
}

int make_args(const GridSpec &g, double lambda_reg, VarArgs &a) {
    PTV_TRY(grid_dims("variational", g.nx, g.ny, g.nz, a));
    if (!(g.dx > 0.0) || !(g.dy > 0.0) || !(g.dz > 0.0) || !std::isfinite(g.dx) || !std::isfinite(g.dy) ||
        !std::isfinite(g.dz)) {
        set_error("variational: spacings must be positive finite numbers");
        return PTV_E_ARG;
    }
    if (!std::isfinite(lambda_reg)) {
        set_error("variational: lambda_reg must be finite");
        return PTV_E_ARG;
    }
    if (lambda_reg < 0.0) {
        set_error("variational: lambda_reg < 0 (the system is not positive definite)");
        return PTV_E_UNSUPPORTED;
    }
    const double h[3] = {g.dx, g.dy, g.dz};
    for (int k = 0; k < 3; ++k) {
        a.ch[k] = 0.5 / h[k];
        a.eh[k] = 1.0 / h[k];
    }
    a.lambda = lambda_reg;
    return PTV_OK;
}

}  // namespace

int launch_var_divergence(const GridSpec &g, const uint8_t *M, const double *xu, const double *xv, const double *xw,
                          double *d, hipStream_t s) {
    VarArgs a{};
    PTV_TRY(make_args(g, 0.0, a));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(xu, xv, xw, d) && aligned(M, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    GRID_LAUNCH(k_var_div, vec2, nb, s, a, CV3{{xu, xv, xw}}, M, d);
    return PTV_OK;
}

int launch_var_adjoint(const GridSpec &g, double lambda_reg, const uint8_t *M, const double *d, const double *xu,
                       const double *xv, const double *xw, double *yu, double *yv, double *yw, DevBuf<double> &part,
                       hipStream_t s) {
    VarArgs a{};
    PTV_TRY(make_args(g, lambda_reg, a));
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(d, xu, xv, xw, yu, yv, yw) && aligned(M, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    PTV_TRY(part.ensure(nb));
    GRID_LAUNCH(k_q, vec2, nb, s, a, (const double *)nullptr, d, CV3{{xu, xv, xw}}, V3{{yu, yv, yw}}, M, part.p);
    return PTV_OK;
}

int variational_run(VarWork &wk, const GridSpec &g, const VarSolve &sv, const uint8_t *M, const double *U,
                    const double *V, const double *W, double *Uo, double *Vo, double *Wo, hipStream_t s,
                    ptv_variational_stats *st) {
    VarArgs a{};
    PTV_TRY(make_args(g, sv.lambda_reg, a));
    if (!std::isfinite(sv.rtol) || sv.maxiter < 0) {
        set_error("variational: rtol must be finite and maxiter non-negative");
        return PTV_E_ARG;
    }
    const size_t n = a.n;
    // vec2: nx is even, so n is, and the three parts of a scratch vector are 16-byte aligned
    const bool vec2 = a.nx % 2 == 0 && all_aligned16(U, V, W, Uo, Vo, Wo) && aligned(M, 2);
    const unsigned nb = blocks_for(a.n, vec2 ? 2 : 1);
    for (DevBuf<double> *b : {&wk.x, &wk.r, &wk.p[0], &wk.p[1], &wk.q}) PTV_TRY(b->ensure(3 * n));
    PTV_TRY(wk.d.ensure(n));
    PTV_TRY(wk.div.ensure(n));
    PTV_TRY(wk.part.ensure(3 * (size_t)nb));
    PTV_TRY(wk.state.ensure(kStateLen));
    PTV_TRY(wk.h_state.ensure(3 * kStateLen));
    double *h_final = wk.h_state.p + 2 * kStateLen;
    const size_t sbytes = kStateLen * sizeof(double);
    const CgCfg cfg{sv.rtol, sv.maxiter};
    auto event = [&](size_t k) { return record_event(wk.ev, k, s); };
    auto scalar = [&](int phase, int slot) {
        hipLaunchKernelGGL(k_cg_scalar, dim3(1), dim3(kGridFinalThreads), 0, s, phase, cfg, wk.state.p, wk.part.p, nb,
                           slot);
        PTV_HIP(hipGetLastError());
        return PTV_OK;
    };
    const DivArgs d = full_grid_div(a, g.dx, g.dy, g.dz);
    // mean |div| over the fluid voxels of three fields into state slot S_DIV0 + slot (physics.py:503-504)
    auto mean_abs_div = [&](const double *fu, const double *fv, const double *fw, int slot) {
        PTV_TRY(launch_divergence(d, fu, fv, fw, M, wk.div.p, s));
        GRID_LAUNCH(k_div_stats, vec2, nb, s, (GridDims)a, wk.div.p, M, wk.part.p, nb);
        return scalar(PH_DIV, slot);
    };

    ptv_variational_stats out{};
    PTV_TRY(event(0));
    PTV_HIP(hipMemsetAsync(wk.state.p, 0, sbytes, s));
    PTV_TRY(mean_abs_div(U, V, W, 0));
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, sbytes, hipMemcpyDeviceToHost, s));
    PTV_HIP(hipStreamSynchronize(s));
    out.n_fluid = (int64_t)h_final[S_NFLUID];
    if (out.n_fluid <= 0) {  // an argument error: the outputs are not written
        set_error("variational: the fluid mask has no fluid voxel");
        return PTV_E_ARG;
    }

    const V3 X = parts(wk.x.p, n), R = parts(wk.r.p, n), Q = parts(wk.q.p, n);
    const CV3 cR = cparts(wk.r.p, n), cQ = cparts(wk.q.p, n);
    PTV_TRY(event(2));
    for (DevBuf<double> *b : {&wk.p[0], &wk.p[1], &wk.q}) PTV_HIP(hipMemsetAsync(b->p, 0, 3 * n * sizeof(double), s));
    PTV_HIP(hipMemsetAsync(wk.d.p, 0, n * sizeof(double), s));
    GRID_LAUNCH(k_init, vec2, nb, s, a, CV3{{U, V, W}}, M, X, R, wk.part.p);
    PTV_TRY(scalar(PH_INIT, 0));
    PTV_TRY(event(3));
    int cur = 0;  // p[cur] holds the last direction
    std::vector<int> batch_iters;
    PTV_TRY(poll_batches(s, wk.state.p, wk.h_state.p, kStateLen, wk.ev, sv.maxiter, [&](int it) -> int {
        PTV_TRY(scalar(it == 0 ? PH_TOP0 : PH_TOP, 0));
        GRID_LAUNCH(k_dir, vec2, nb, s, a, (const double *)wk.state.p, cR, cparts(wk.p[cur].p, n),
                    parts(wk.p[cur ^ 1].p, n), M, wk.d.p);
        cur ^= 1;
        const CV3 cP = cparts(wk.p[cur].p, n);
        GRID_LAUNCH(k_q, vec2, nb, s, a, (const double *)wk.state.p, (const double *)wk.d.p, cP, Q, M, wk.part.p);
        PTV_TRY(scalar(PH_ALPHA, 0));
        GRID_LAUNCH(k_xr, vec2, nb, s, a, (const double *)wk.state.p, cP, cQ, X, R, M, wk.part.p);
        return PTV_OK;
    }, batch_iters));
    const size_t batches = batch_iters.size();
    PTV_TRY(scalar(PH_END, 0));
    PTV_TRY(event(4 + batches));
    GRID_LAUNCH(k_out, vec2, nb, s, a, (const double *)wk.state.p, cparts(wk.x.p, n), M, V3{{Uo, Vo, Wo}});
    PTV_TRY(mean_abs_div(Uo, Vo, Wo, 1));
    PTV_HIP(hipMemcpyAsync(h_final, wk.state.p, sbytes, hipMemcpyDeviceToHost, s));
    PTV_TRY(event(1));
    PTV_HIP(hipStreamSynchronize(s));
    out.itn = (int32_t)h_final[S_ITN];
    out.info = (int32_t)h_final[S_INFO];
    out.bnorm = h_final[S_BNORM];
    out.rnorm = sqrt(h_final[S_RR]);
    out.mean_abs_div_initial = h_final[S_DIV0];
    out.mean_abs_div_final = h_final[S_DIV1];
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, wk.ev[0], wk.ev[1]));
    out.ms_total = ms;
    PTV_HIP(hipEventElapsedTime(&ms, wk.ev[2], wk.ev[4 + batches]));
    out.ms_solve = ms;
    PTV_TRY(median_iter_ms(wk.ev, 3, batch_iters, out.itn, out.ms_solve, out.ms_iter_median));
    if (st) *st = out;
    return PTV_OK;
}

}  // namespace ptv
