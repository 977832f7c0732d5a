// ptv_multigrid.hip — the multigrid preconditioner of the anchored pressure solve: z = M r, one
// symmetric V-cycle on the active (fluid, not Dirichlet) voxels of ptv_pressure.hip's system
// (A p)_i = sum (p_j - p_i) h^-2, Dirichlet neighbours counted in the diagonal.  A is negative
// definite as written and so is M.
//
// Levels.  Level 0 is the grid; level l + 1 has ceil(n / 2) cells per axis, and a coarse cell
// aggregates the at most 2 x 2 x 2 cells under it (P copies, R = P^T sums).  Coarsening stops when
// every extent is at most 2, or at ptv_mg_params.max_levels.
//
// Operators.  A level is a 7-point operator: per cell the weights of its +x, +y, +z faces (0 at the
// domain edge or where a side is inactive) and an extra diagonal term e; the diagonal is
//     d = 0 + w(x-) + w(x+) + w(y-) + w(y+) + w(z-) + w(z+) + e          (added in this order).
// Level 0 derives them from the mask and Dirichlet bytes: w = 1 / h^2 of the axis between two active
// voxels, e = 0 + [1 / h^2 of the axis for every Dirichlet fluid neighbour, x-, x+, y-, y+, z-, z+],
// both 0 at an inactive voxel.  Coarser levels store 4 doubles per cell, the Galerkin product
// P^T A P: the +x weight is 0 + the +x weights of the children (2X+1, 2Y+b, 2Z+c) in the order
// (c, b) = (0,0) (0,1) (1,0) (1,1); +y: children (2X+a, 2Y+1, 2Z+c), order (c, a); +z: children
// (2X+a, 2Y+b, 2Z+1), order (b, a); e = 0 + the children's e, z slowest, x fastest.  A child
// outside the fine grid is skipped.  Faces inside an aggregate cancel.
//
// One cell's operations (A z uses clamped neighbour indices, a missing face has weight 0):
//     (A z)_i = ((0 + w(x-) (z_x- - z_i)) + ... + w(z+) (z_z+ - z_i)) - e z_i
//     sweep      z_i <- z_i - (omega (r_i - (A z)_i)) / d_i         (from zero: 0 - (omega r_i) / d_i)
//     residual   r_i - (A z)_i
//     restrict   r_C = 0 + the children's residuals, z slowest, x fastest
//     prolong    z_i <- z_i + z_C
// A cell with d = 0 (inactive, an isolated active voxel, an aggregate of such) is outside the system:
// its z is 0, its residual 0, and the prolongation leaves it alone.  Sweeps are Jacobi: they read one
// buffer and write the other; sweep k of S writes the iterate's own buffer when S - k is even, so
// the last one lands there (the prolongation writes the buffer sweep 1 reads).
//
// Cycle at level l: nu sweeps from zero, residual + restriction, level l + 1, prolongation, nu
// sweeps; the coarsest level runs coarse_sweeps sweeps from zero.  Nothing but elementwise double
// arithmetic without contraction and sums of at most eight terms in the order above, so the result
// is the bits of tests/_mg_ref.py.
//
// Launches.  A level above the tail takes one launch per sweep, one for residual + restriction (a
// thread per coarse cell) and one for the prolongation, in the dense-grid frame of ptv_grid_vec.hpp
// (two x per lane when nx is even and the vectors are 16-byte aligned).  From the first level of at
// most kMgTailCells cells down to the coarsest and back up, one workgroup runs everything in one
// launch, its vectors in LDS (z and r per level, one scratch vector), sweeps separated by
// __syncthreads(), with the very same per-cell functions.  Every kernel of a cycle returns at once
// when the solver's stop flag is set.  No floating-point atomics; the only atomics count cells.
#include <algorithm>
#include <cmath>

#include "ptv_multigrid.hpp"
#include "ptv_grid_solve.hpp"

namespace ptv {

namespace {

constexpr int kTailThreads = 1024;

// a level as the kernels see it; W is NULL on level 0
struct Lvl : GridDims {
    const double *W;
};
// what level 0 derives its operator from
struct Fine {
    const uint8_t *M, *Dir;
    double ih2[3];
};

struct Sten {
    double w[6];  // x-, x+, y-, y+, z-, z+
    double e;
    unsigned j[6];  // the neighbours' indices, clamped at the domain faces
};

__device__ __forceinline__ bool is_active(const Fine &F, unsigned i) {
    return F.M[i] != 0 && !(F.Dir && F.Dir[i] != 0);
}

template <bool FINE>
__device__ __forceinline__ void stencil(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z, Sten &s) {
    const bool has[6] = {x > 0, x + 1 < L.nx, y > 0, y + 1 < L.ny, z > 0, z + 1 < L.nz};
    s.j[0] = has[0] ? i - 1u : i;
    s.j[1] = has[1] ? i + 1u : i;
    s.j[2] = has[2] ? i - (unsigned)L.nx : i;
    s.j[3] = has[3] ? i + (unsigned)L.nx : i;
    s.j[4] = has[4] ? i - L.plane : i;
    s.j[5] = has[5] ? i + L.plane : i;
    if constexpr (FINE) {
        const bool act = is_active(F, i);
        s.e = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            bool a = false, d = false;
            if (act && has[k]) {
                const bool m = F.M[s.j[k]] != 0, dir = F.Dir && F.Dir[s.j[k]] != 0;
                a = m && !dir;
                d = m && dir;
            }
            s.w[k] = a ? F.ih2[k >> 1] : 0.0;
            if (d) s.e += F.ih2[k >> 1];
        }
    } else {
        const double *__restrict__ W = L.W;
        s.w[0] = has[0] ? W[4 * (size_t)s.j[0] + 0] : 0.0;
        s.w[1] = W[4 * (size_t)i + 0];
        s.w[2] = has[2] ? W[4 * (size_t)s.j[2] + 1] : 0.0;
        s.w[3] = W[4 * (size_t)i + 1];
        s.w[4] = has[4] ? W[4 * (size_t)s.j[4] + 2] : 0.0;
        s.w[5] = W[4 * (size_t)i + 2];
        s.e = W[4 * (size_t)i + 3];
    }
}

__device__ __forceinline__ double diag_of(const Sten &s) {
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) d += s.w[k];
    d += s.e;
    return d;
}

__device__ __forceinline__ double apply_a(const Sten &s, const double *z, double zi) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc += s.w[k] * (z[s.j[k]] - zi);
    acc = acc - s.e * zi;
    return acc;
}

// one cell of a sweep; zin is not read when from_zero
template <bool FINE>
__device__ __forceinline__ double sweep_cell(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z,
                                             double omega, bool from_zero, const double *r, const double *zin) {
    Sten s;
    stencil<FINE>(L, F, i, x, y, z, s);
    const double d = diag_of(s);
    if (d == 0.0) return 0.0;
    if (from_zero) return 0.0 - (omega * r[i]) / d;
    const double zi = zin[i];
    return zi - (omega * (r[i] - apply_a(s, zin, zi))) / d;
}

template <bool FINE>
__device__ __forceinline__ double residual_cell(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z,
                                                const double *r, const double *zv) {
    Sten s;
    stencil<FINE>(L, F, i, x, y, z, s);
    if (diag_of(s) == 0.0) return 0.0;
    return r[i] - apply_a(s, zv, zv[i]);
}

// the restricted residual of coarse cell (X, Y, Z) over fine level L
template <bool FINE>
__device__ __forceinline__ double restrict_cell(const Lvl &L, const Fine &F, int X, int Y, int Z, const double *r,
                                                const double *zv) {
    double sum = 0.0;
    for (int c = 0; c < 2; ++c) {
        for (int b = 0; b < 2; ++b) {
            for (int a = 0; a < 2; ++a) {
                const int x = 2 * X + a, y = 2 * Y + b, z = 2 * Z + c;
                if (x >= L.nx || y >= L.ny || z >= L.nz) continue;
                const unsigned i = (unsigned)z * L.plane + (unsigned)y * (unsigned)L.nx + (unsigned)x;
                sum += residual_cell<FINE>(L, F, i, x, y, z, r, zv);
            }
        }
    }
    return sum;
}

// one cell of the prolongation: zin + the parent's correction; (cnx, cplane) index the coarse level
template <bool FINE>
__device__ __forceinline__ double prolong_cell(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z,
                                               unsigned cnx, unsigned cplane, const double *zc, const double *zin) {
    Sten s;
    stencil<FINE>(L, F, i, x, y, z, s);
    const double zi = zin[i];
    if (diag_of(s) == 0.0) return zi;
    return zi + zc[(unsigned)(z >> 1) * cplane + (unsigned)(y >> 1) * cnx + (unsigned)(x >> 1)];
}

// the +axis face weight and the extra term of fine cell i (setup)
template <bool FINE>
__device__ __forceinline__ double face_plus(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z, int axis) {
    if constexpr (FINE) {
        const int t = axis == 0 ? x : axis == 1 ? y : z, n = axis == 0 ? L.nx : axis == 1 ? L.ny : L.nz;
        if (t + 1 >= n) return 0.0;
        const unsigned stride = axis == 0 ? 1u : axis == 1 ? (unsigned)L.nx : L.plane;
        return (is_active(F, i) && is_active(F, i + stride)) ? F.ih2[axis] : 0.0;
    } else {
        return L.W[4 * (size_t)i + axis];
    }
}
template <bool FINE>
__device__ __forceinline__ double extra_of(const Lvl &L, const Fine &F, unsigned i, int x, int y, int z) {
    if constexpr (FINE) {
        Sten s;
        stencil<true>(L, F, i, x, y, z, s);
        return s.e;
    } else {
        return L.W[4 * (size_t)i + 3];
    }
}

__device__ __forceinline__ void coords(const GridDims &a, unsigned i, int &x, int &y, int &z) {
    z = (int)(i / a.plane);
    const unsigned r = i - (unsigned)z * a.plane;
    y = (int)(r / (unsigned)a.nx);
    x = (int)(r - (unsigned)y * (unsigned)a.nx);
}

__device__ __forceinline__ bool stopped(const double *st) { return st && st[kStopSlot] != 0.0; }

// ---- setup ----

// the Galerkin operator of coarse level C from fine level L: a thread per coarse cell
template <bool FINE>
__global__ __launch_bounds__(kGridThreads) void k_mg_coarsen(Lvl L, Fine F, GridDims C, double *__restrict__ Wc) {
    const unsigned ci = blockIdx.x * kGridThreads + threadIdx.x;
    if (ci >= C.n) return;
    int X, Y, Z;
    coords(C, ci, X, Y, Z);
    double w[3] = {0.0, 0.0, 0.0}, e = 0.0;
    for (int c = 0; c < 2; ++c) {
        for (int b = 0; b < 2; ++b) {
            for (int a = 0; a < 2; ++a) {
                const int x = 2 * X + a, y = 2 * Y + b, z = 2 * Z + c;
                if (x >= L.nx || y >= L.ny || z >= L.nz) continue;
                const unsigned i = (unsigned)z * L.plane + (unsigned)y * (unsigned)L.nx + (unsigned)x;
                if (a == 1) w[0] += face_plus<FINE>(L, F, i, x, y, z, 0);
                if (b == 1) w[1] += face_plus<FINE>(L, F, i, x, y, z, 1);
                if (c == 1) w[2] += face_plus<FINE>(L, F, i, x, y, z, 2);
                e += extra_of<FINE>(L, F, i, x, y, z);
            }
        }
    }
    Wc[4 * (size_t)ci + 0] = w[0];
    Wc[4 * (size_t)ci + 1] = w[1];
    Wc[4 * (size_t)ci + 2] = w[2];
    Wc[4 * (size_t)ci + 3] = e;
}

// count[0] += the cells of the level with a non-zero diagonal
template <bool FINE>
__global__ __launch_bounds__(kGridThreads) void k_mg_count(Lvl L, Fine F, unsigned *count) {
    const unsigned i = blockIdx.x * kGridThreads + threadIdx.x;
    bool in = false;
    if (i < L.n) {
        int x, y, z;
        coords(L, i, x, y, z);
        Sten s;
        stencil<FINE>(L, F, i, x, y, z, s);
        in = diag_of(s) != 0.0;
    }
    const int c = __syncthreads_count(in ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(count, (unsigned)c);
}

// ---- a level above the tail ----

template <bool FINE, int VEC>
__global__ __launch_bounds__(kGridThreads) void k_mg_sweep(Lvl L, Fine F, const double *__restrict__ st, double omega,
                                                           int from_zero, const double *__restrict__ R,
                                                           const double *__restrict__ Zin, double *__restrict__ Zout) {
    if (stopped(st)) return;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(L, it, p)) break;
        DV<VEC> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            o.e[e] = sweep_cell<FINE>(L, F, p.i + e, p.x + e, p.y, p.z, omega, from_zero != 0, R, Zin);
        std_<VEC>(Zout + p.i, o);
    }
}

// Rc = P^T (R - A Z): a thread per coarse cell
template <bool FINE>
__global__ __launch_bounds__(kGridThreads) void k_mg_restrict(Lvl L, Fine F, GridDims C, const double *__restrict__ st,
                                                              const double *__restrict__ R,
                                                              const double *__restrict__ Zv, double *__restrict__ Rc) {
    if (stopped(st)) return;
    const unsigned ci = blockIdx.x * kGridThreads + threadIdx.x;
    if (ci >= C.n) return;
    int X, Y, Z;
    coords(C, ci, X, Y, Z);
    Rc[ci] = restrict_cell<FINE>(L, F, X, Y, Z, R, Zv);
}

template <bool FINE, int VEC>
__global__ __launch_bounds__(kGridThreads) void k_mg_prolong(Lvl L, Fine F, GridDims C, const double *__restrict__ st,
                                                             const double *__restrict__ Zc, const double *Zin,
                                                             double *Zout) {
    if (stopped(st)) return;
#pragma unroll
    for (int it = 0; it < kGridItems; ++it) {
        Pos p;
        if (!group_pos<VEC>(L, it, p)) break;
        DV<VEC> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            o.e[e] = prolong_cell<FINE>(L, F, p.i + e, p.x + e, p.y, p.z, (unsigned)C.nx, C.plane, Zc, Zin);
        std_<VEC>(Zout + p.i, o);
    }
}

// ---- the fused tail: one workgroup, vectors in LDS ----

struct TailArgs {
    int first, levels;  // levels first .. levels - 1 run here
    int nu, coarse_sweeps;
    double omega;
    unsigned off_t;                 // LDS offsets in doubles: the scratch vector,
    unsigned off_z[kMgMaxLevels];   // a level's iterate
    unsigned off_r[kMgMaxLevels];   // and right-hand side
    Lvl L[kMgMaxLevels];
};

// `count` sweeps on the level ending in zv; the first from zero, or reading the buffer the parity
// rule names (see the head of the file)
template <bool FINE>
__device__ __forceinline__ void tail_sweeps(const Lvl &L, const Fine &F, double omega, int count, bool from_zero,
                                            const double *r, double *zv, double *t) {
    for (int k = 1; k <= count; ++k) {
        double *dst = ((count - k) & 1) ? t : zv;
        const double *src = ((count - k) & 1) ? zv : t;
        for (unsigned i = threadIdx.x; i < L.n; i += kTailThreads) {
            int x, y, z;
            coords(L, i, x, y, z);
            dst[i] = sweep_cell<FINE>(L, F, i, x, y, z, omega, from_zero && k == 1, r, src);
        }
        __syncthreads();
    }
}

template <bool FINE>
__device__ __forceinline__ void tail_restrict(const Lvl &L, const Fine &F, const GridDims &C, const double *r,
                                              const double *zv, double *rc) {
    for (unsigned ci = threadIdx.x; ci < C.n; ci += kTailThreads) {
        int X, Y, Z;
        coords(C, ci, X, Y, Z);
        rc[ci] = restrict_cell<FINE>(L, F, X, Y, Z, r, zv);
    }
    __syncthreads();
}

template <bool FINE>
__device__ __forceinline__ void tail_prolong(const Lvl &L, const Fine &F, const GridDims &C, const double *zc,
                                             const double *zin, double *zout) {
    for (unsigned i = threadIdx.x; i < L.n; i += kTailThreads) {
        int x, y, z;
        coords(L, i, x, y, z);
        zout[i] = prolong_cell<FINE>(L, F, i, x, y, z, (unsigned)C.nx, C.plane, zc, zin);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kTailThreads) void k_mg_tail(TailArgs A, Fine F, const double *__restrict__ st,
                                                          const double *__restrict__ R, double *__restrict__ Zg) {
    extern __shared__ double lds[];
    if (stopped(st)) return;
    double *const t = lds + A.off_t;
    const int first = A.first, last = A.levels - 1;
    {
        double *r0 = lds + A.off_r[first];
        for (unsigned i = threadIdx.x; i < A.L[first].n; i += kTailThreads) r0[i] = R[i];
        __syncthreads();
    }
    for (int l = first; l < last; ++l) {
        double *zv = lds + A.off_z[l], *r = lds + A.off_r[l], *rc = lds + A.off_r[l + 1];
        if (l == 0) {
            tail_sweeps<true>(A.L[l], F, A.omega, A.nu, true, r, zv, t);
            tail_restrict<true>(A.L[l], F, A.L[l + 1], r, zv, rc);
        } else {
            tail_sweeps<false>(A.L[l], F, A.omega, A.nu, true, r, zv, t);
            tail_restrict<false>(A.L[l], F, A.L[l + 1], r, zv, rc);
        }
    }
    if (last == 0) tail_sweeps<true>(A.L[0], F, A.omega, A.coarse_sweeps, true, lds + A.off_r[0], lds + A.off_z[0], t);
    else tail_sweeps<false>(A.L[last], F, A.omega, A.coarse_sweeps, true, lds + A.off_r[last], lds + A.off_z[last], t);
    for (int l = last - 1; l >= first; --l) {
        double *zv = lds + A.off_z[l], *r = lds + A.off_r[l];
        const double *zc = lds + A.off_z[l + 1];
        double *start = (A.nu & 1) ? t : zv;  // the buffer the first of nu sweeps reads
        if (l == 0) {
            tail_prolong<true>(A.L[l], F, A.L[l + 1], zc, zv, start);
            tail_sweeps<true>(A.L[l], F, A.omega, A.nu, false, r, zv, t);
        } else {
            tail_prolong<false>(A.L[l], F, A.L[l + 1], zc, zv, start);
            tail_sweeps<false>(A.L[l], F, A.omega, A.nu, false, r, zv, t);
        }
    }
    const double *z0 = lds + A.off_z[first];
    for (unsigned i = threadIdx.x; i < A.L[first].n; i += kTailThreads) Zg[i] = z0[i];
}

// ---- host ----

Lvl level_of(const MgPlan &plan, int l, const double *w_base) {
    const MgLevel &m = plan.lv[l];
    Lvl L{};
    L.nx = m.nx;
    L.ny = m.ny;
    L.nz = m.nz;
    L.n = m.n;
    L.plane = m.plane;
    L.W = l == 0 ? nullptr : w_base + m.w;
    return L;
}

Fine fine_of(const MgPlan &plan, const uint8_t *M, const uint8_t *Dir) {
    Fine F{};
    F.M = M;
    F.Dir = Dir;
    for (int k = 0; k < 3; ++k) F.ih2[k] = plan.ih2[k];
    return F;
}

size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

// LDS bytes of a tail that starts at level l
size_t tail_bytes(const MgPlan &plan, int l) {
    size_t d = even(plan.lv[l].n);
    for (int k = l; k < plan.levels; ++k) d += 2 * even(plan.lv[k].n);
    return d * sizeof(double);
}

#define MG_LAUNCH_FV(kernel, fine, vec2, nb, s, ...)                                                          \
    do {                                                                                                      \
        if (fine) GRID_LAUNCH_T(kernel, true, vec2, nb, s, __VA_ARGS__);                                      \
        else GRID_LAUNCH_T(kernel, false, vec2, nb, s, __VA_ARGS__);                                          \
    } while (0)
#define GRID_LAUNCH_T(kernel, F, vec2, nb, s, ...)                                                            \
    do {                                                                                                      \
        if (vec2) hipLaunchKernelGGL((kernel<F, 2>), dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);         \
        else hipLaunchKernelGGL((kernel<F, 1>), dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);              \
        PTV_HIP(hipGetLastError());                                                                           \
    } while (0)
#define MG_LAUNCH_F(kernel, fine, nb, s, ...)                                                                 \
    do {                                                                                                      \
        if (fine) hipLaunchKernelGGL((kernel<true>), dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);         \
        else hipLaunchKernelGGL((kernel<false>), dim3(nb), dim3(kGridThreads), 0, s, __VA_ARGS__);             \
        PTV_HIP(hipGetLastError());                                                                           \
    } while (0)

unsigned cell_blocks(unsigned n) { return (n + kGridThreads - 1) / kGridThreads; }

// `count` sweeps on a level above the tail, ending in Z
int level_sweeps(const Lvl &L, const Fine &F, bool fine, const double *st, double omega, int count, bool from_zero,
                 const double *R, double *Z, double *T, hipStream_t s) {
    const bool vec2 = L.nx % 2 == 0 && all_aligned16(R, Z, T);
    const unsigned nb = blocks_for(L.n, vec2 ? 2 : 1);
    for (int k = 1; k <= count; ++k) {
        double *dst = ((count - k) & 1) ? T : Z;
        const double *src = ((count - k) & 1) ? Z : T;
        MG_LAUNCH_FV(k_mg_sweep, fine, vec2, nb, s, L, F, st, omega, (from_zero && k == 1) ? 1 : 0, R, src, dst);
    }
    return PTV_OK;
}

}  // namespace

int mg_plan(const GridSpec &g, const ptv_mg_params *prm, MgPlan &plan) {
    const ptv_mg_params def{};
    if (!prm) prm = &def;
    if (prm->max_levels < 0 || prm->nu < 0 || prm->coarse_sweeps < 0 || !std::isfinite(prm->omega) ||
        prm->omega < 0.0) {
        set_error("multigrid: max_levels, nu, coarse_sweeps and omega must be non-negative (0: the default), "
                  "omega finite");
        return PTV_E_ARG;
    }
    GridDims a{};
    PTV_TRY(grid_dims("multigrid", g.nx, g.ny, g.nz, a));
    const double h[3] = {g.dx, g.dy, g.dz};
    for (int k = 0; k < 3; ++k) {
        if (!(h[k] > 0.0) || !std::isfinite(h[k])) {
            set_error("multigrid: spacings must be positive finite numbers");
            return PTV_E_ARG;
        }
        plan.ih2[k] = 1.0 / (h[k] * h[k]);
    }
    plan.nu = prm->nu > 0 ? prm->nu : 2;
    plan.coarse_sweeps = prm->coarse_sweeps > 0 ? prm->coarse_sweeps : 16;
    plan.omega = prm->omega > 0.0 ? prm->omega : 2.0 / 3.0;
    const int cap = prm->max_levels > 0 ? std::min(prm->max_levels, kMgMaxLevels) : kMgMaxLevels;
    int nx = g.nx, ny = g.ny, nz = g.nz;
    size_t w = 0, v = 0;
    plan.levels = 0;
    for (;;) {
        MgLevel &m = plan.lv[plan.levels];
        m.nx = nx;
        m.ny = ny;
        m.nz = nz;
        m.n = (unsigned)nx * (unsigned)ny * (unsigned)nz;
        m.plane = (unsigned)nx * (unsigned)ny;
        m.w = m.z = m.r = m.t = 0;
        if (plan.levels > 0) {  // every array starts on a 16-byte boundary
            m.w = w;
            w += 4 * (size_t)m.n;
            m.z = v;
            m.r = v + even(m.n);
            m.t = v + 2 * even(m.n);
            v += 3 * even(m.n);
        }
        ++plan.levels;
        if (std::max(nx, std::max(ny, nz)) <= 2 || plan.levels >= cap) break;
        nx = (nx + 1) / 2;
        ny = (ny + 1) / 2;
        nz = (nz + 1) / 2;
    }
    plan.w_len = w;
    plan.vec_len = v;
    plan.tail = plan.levels;  // no level fits: every level takes its own launches
    plan.tail_lds = 0;
    for (int l = 0; l < plan.levels; ++l) {
        if (plan.lv[l].n <= kMgTailCells && tail_bytes(plan, l) <= kMgTailLdsBytes) {
            plan.tail = l;
            plan.tail_lds = tail_bytes(plan, l);
            break;
        }
    }
    return PTV_OK;
}

int mg_setup(MgWork &wk, const MgPlan &plan, const uint8_t *M, const uint8_t *Dir, hipStream_t s) {
    PTV_TRY(wk.w.ensure(plan.w_len));
    PTV_TRY(wk.vec.ensure(plan.vec_len));
    PTV_TRY(wk.counts.ensure(kMgMaxLevels));
    PTV_TRY(wk.h_counts.ensure(kMgMaxLevels));
    const Fine F = fine_of(plan, M, Dir);
    if (wk.ev.size() < 4) wk.ev.resize(4);
    PTV_TRY(wk.ev[0].record(s));
    PTV_HIP(hipMemsetAsync(wk.counts.p, 0, kMgMaxLevels * sizeof(unsigned), s));
    for (int l = 0; l < plan.levels; ++l) {
        const Lvl L = level_of(plan, l, wk.w.p);
        if (l + 1 < plan.levels) {
            const Lvl C = level_of(plan, l + 1, wk.w.p);
            MG_LAUNCH_F(k_mg_coarsen, l == 0, cell_blocks(C.n), s, L, F, (GridDims)C, wk.w.p + plan.lv[l + 1].w);
        }
    }
    for (int l = 0; l < plan.levels; ++l) {
        const Lvl L = level_of(plan, l, wk.w.p);
        MG_LAUNCH_F(k_mg_count, l == 0, cell_blocks(L.n), s, L, F, wk.counts.p + l);
    }
    PTV_HIP(hipMemcpyAsync(wk.h_counts.p, wk.counts.p, kMgMaxLevels * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    PTV_TRY(wk.ev[1].record(s));
    return PTV_OK;
}

int mg_vcycle(MgWork &wk, const MgPlan &plan, const uint8_t *M, const uint8_t *Dir, const double *st,
              const double *R, double *Z, double *T0, hipStream_t s) {
    const Fine F = fine_of(plan, M, Dir);
    if (!T0) {
        PTV_TRY(wk.t0.ensure(plan.lv[0].n));
        T0 = wk.t0.p;
    }
    double *base = wk.vec.p;
    auto zof = [&](int l) { return l == 0 ? Z : base + plan.lv[l].z; };
    auto rof = [&](int l) { return l == 0 ? R : (const double *)(base + plan.lv[l].r); };
    auto tof = [&](int l) { return l == 0 ? T0 : base + plan.lv[l].t; };
    // levels 0 .. G - 1 take their own launches; level G is the tail's first, or the coarsest
    const bool has_tail = plan.tail < plan.levels;
    const int G = has_tail ? plan.tail : plan.levels - 1;
    for (int l = 0; l < G; ++l) {
        const Lvl L = level_of(plan, l, wk.w.p), C = level_of(plan, l + 1, wk.w.p);
        PTV_TRY(level_sweeps(L, F, l == 0, st, plan.omega, plan.nu, true, rof(l), zof(l), tof(l), s));
        MG_LAUNCH_F(k_mg_restrict, l == 0, cell_blocks(C.n), s, L, F, (GridDims)C, st, rof(l), (const double *)zof(l),
                    base + plan.lv[l + 1].r);
    }
    if (has_tail) {
        TailArgs A{};
        A.first = plan.tail;
        A.levels = plan.levels;
        A.nu = plan.nu;
        A.coarse_sweeps = plan.coarse_sweeps;
        A.omega = plan.omega;
        size_t off = 0;
        A.off_t = (unsigned)off;
        off += even(plan.lv[plan.tail].n);
        for (int l = plan.tail; l < plan.levels; ++l) {
            A.off_z[l] = (unsigned)off;
            off += even(plan.lv[l].n);
            A.off_r[l] = (unsigned)off;
            off += even(plan.lv[l].n);
            A.L[l] = level_of(plan, l, wk.w.p);
        }
        if (off * sizeof(double) != plan.tail_lds || plan.tail_lds > kMgTailLdsBytes) {
            set_error("multigrid: the tail's LDS layout does not match its plan");
            return PTV_E_HIP;
        }
        // above 64 KiB the runtime wants to be told; a runtime that has no such limit may refuse the
        // attribute, and the launch below reports what matters
        (void)hipFuncSetAttribute((const void *)k_mg_tail, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)plan.tail_lds);
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(kTailThreads), plan.tail_lds, s, A, F, st, rof(G), zof(G));
        PTV_HIP(hipGetLastError());
    } else {
        const Lvl L = level_of(plan, G, wk.w.p);
        PTV_TRY(level_sweeps(L, F, G == 0, st, plan.omega, plan.coarse_sweeps, true, rof(G), zof(G), tof(G), s));
    }
    for (int l = G - 1; l >= 0; --l) {
        const Lvl L = level_of(plan, l, wk.w.p), C = level_of(plan, l + 1, wk.w.p);
        double *start = (plan.nu & 1) ? tof(l) : zof(l);
        const bool vec2 = L.nx % 2 == 0 && all_aligned16(zof(l), tof(l));
        MG_LAUNCH_FV(k_mg_prolong, l == 0, vec2, blocks_for(L.n, vec2 ? 2 : 1), s, L, F, (GridDims)C, st,
                     (const double *)zof(l + 1), (const double *)zof(l), start);
        PTV_TRY(level_sweeps(L, F, l == 0, st, plan.omega, plan.nu, false, rof(l), zof(l), tof(l), s));
    }
    return PTV_OK;
}

int mg_fill_stats(MgWork &wk, const MgPlan &plan, ptv_mg_stats *out) {
    if (!out) return PTV_OK;
    *out = ptv_mg_stats{};
    out->levels = plan.levels;
    out->tail_level = plan.tail;
    for (int l = 0; l < plan.levels; ++l) {
        out->cells[l] = plan.lv[l].n;
        out->active[l] = wk.h_counts.p[l];
    }
    float ms = 0.f;
    PTV_HIP(hipEventElapsedTime(&ms, wk.ev[0], wk.ev[1]));
    out->ms_setup = ms;
    return PTV_OK;
}

}  // namespace ptv
