// ptv_mesh.hip — cubic B-spline prefilter, order 0 / 1 / 3 sampling and the traction integration of
// the mesh interface drag.
//
// Restates scipy.ndimage.spline_filter / map_coordinates for mode='nearest' and
// velocity_analysis.compute_interface_drag_mesh from the triangulation onward
// (velocity_analysis.py:547-655).  The reference filters the whole volume again for every label and
// field; here a field is filtered once, the coefficients stay in HBM and all labels' triangles go
// through one launch.  The build passes -ffp-contract=off: every product and sum below rounds as
// written; the fused multiply-adds are the explicit ones of the double-double helpers.
//
// Prefilter.  The coefficient array is the field padded by 12 edge-replicated samples per side,
// (nz + 24, ny + 24, nx + 24) float64, filtered along axis 0, 1, 2 in turn with scipy's recursion
// (filter_line below): gain, reflect start, forward, anticausal start, backward.
//   - Axis 0 (z): one lane per padded (y, x) column, x fastest across lanes, so every load and store
//     of a wave is one run of the row.  The padding happens in this pass's loads (clamped indices
//     into the raw field); there is no padded copy of the input.
//   - Axis 1 (y): one lane per (z, x) column, in place, again x fastest.
//   - Axis 2 (x): the lines themselves are contiguous, so a lane per line would load with a stride
//     of a whole line.  A block of one wave takes 64 lines and walks them in chunks of 64 columns:
//     the chunk is loaded row by row (512 B runs) into a 64 x 65 LDS tile (33 KB, four blocks per
//     compute unit), each lane runs the recursion over its own row of the tile, and the tile goes
//     back row by row.  A forward sweep over the chunks, then a backward one; the recursion's state
//     crosses chunks in a register.
// The start sum stops after PTV_SPLINE_HORIZON terms (|z|^40 = 1.3e-23 of the line's scale); a line
// that short is summed whole, with scipy's z^n terms.  The recursion's state is a double-double and
// the array holds its rounding: between two passes a coefficient is rounded once.
//
// Sampling.  One lane per point.  Order 3 reads the padded coefficients at coordinate + 12 (scipy
// samples the padded array: the spline's own extrapolation over the replicated edge, not the value
// at the clamped coordinate).  The coordinate is clamped one sample past the padded extent, to
// [-1, N] of the padded index space, and the four indices to [0, N - 1], as scipy does: past the pad
// the fraction still moves the weights over the edge-extended coefficients until the value saturates
// at -1 and at N (cell_of).  The 4 x 4 x 4 block is summed separably, x innermost: 16 row sums, 4
// plane sums, one value, weights and sums in double-double.  Order 1 reads the raw field at the
// coordinate clamped to [0, n - 1].  A non-finite order-1 sample takes its kind (NaN, +Inf, -Inf)
// from the plain float64 sum, since the double-double error terms turn every Inf into NaN; order 3
// over a non-finite coefficient is NaN.
//
// Traction integration.  One lane per triangle, blocks of 256 that never span two labels (the host
// builds the block -> (label, first triangle) table).  A block reduces the 21 terms in a fixed
// order (wave64 DPP tree, then the four waves in order) and writes one partial per key; k_mesh_final
// adds a label's partials in block order.  No floating-point atomics: the sums are the same bits on
// every call.  A zero-area triangle follows the reference into 0 / 0: NaN in the viscous keys and
// in the phase-split force keys of the class it lands in, 0 in the pressure keys and the areas.
#include <algorithm>
#include <cmath>

#include "../../include/ptv_api.h"
#include "ptv_common.hpp"
#include "ptv_mesh.hpp"
#include "ptv_wave.hpp"

namespace ptv {

namespace {

constexpr int kPad = PTV_SPLINE_PAD;
constexpr int kHorizon = PTV_SPLINE_HORIZON;
constexpr int kLineThreads = 256;
constexpr int kTile = 64;  // lines per block and columns per chunk of the x pass

// ---- double-double arithmetic (an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2) ----
// The recursion's state, the spline weights and the tensor sums are carried in it, and every stored
// value is its rounding to float64: a coefficient or a sample is then off by about one rounding of
// the result, not by the accumulated roundings of some hundred float64 operations (which the
// viscous terms amplify through the difference u_interface - u_inner).
struct dd {
    double hi, lo;
};
__host__ __device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ __forceinline__ dd quick_two_sum(double a, double b) {
    const double s = a + b;
    return dd{s, b - (s - a)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return dd{p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    const dd s = two_sum(a.hi, b.hi);
    return quick_two_sum(s.hi, s.lo + (a.lo + b.lo));
}
__device__ __forceinline__ dd dd_add_d(dd a, double b) {
    const dd s = two_sum(a.hi, b);
    return quick_two_sum(s.hi, s.lo + a.lo);
}
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd{-b.hi, -b.lo}); }
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
    const dd p = two_prod(a.hi, b.hi);
    return quick_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
__device__ __forceinline__ dd dd_mul_d(dd a, double b) {
    const dd p = two_prod(a.hi, b);
    return quick_two_sum(p.hi, p.lo + a.lo * b);
}
__device__ __forceinline__ dd dd_div_d(dd a, double b) {
    const double q1 = a.hi / b;
    const dd p = two_prod(q1, b);
    const dd r = dd_sub(a, p);
    return quick_two_sum(q1, r.hi / b);
}

// what the recursion along one axis of padded length n needs, each constant to double-double
struct Pole {
    dd z, gain, zn, start, anti;  // pole, (1-z)(1-1/z), z^n, z / (1 - z^2n), z / (z - 1)
    int whole;                    // the start sum covers the whole line (with the z^n terms)
};

dd split_ld(long double v) {
    const double hi = (double)v;
    return dd{hi, (double)(v - (long double)hi)};
}

Pole make_pole(int64_t n) {
    const long double z = sqrtl(3.0L) - 2.0L, zn = powl(z, (long double)n);
    Pole p;
    p.z = split_ld(z);
    p.gain = split_ld((1.0L - z) * (1.0L - 1.0L / z));
    p.zn = split_ld(zn);
    p.start = split_ld(z / (1.0L - zn * zn));
    p.anti = split_ld(z / (z - 1.0L));
    p.whole = n - 1 <= kHorizon;
    return p;
}

// scipy's reflect start of the causal recursion from the raw samples src(0 .. n-1)
template <typename Src>
__device__ __forceinline__ dd causal_start(int n, const Pole &p, Src src) {
    const dd c0 = dd_mul_d(p.gain, src(0));
    dd s = p.whole ? dd_add(c0, dd_mul(p.zn, dd_mul_d(p.gain, src(n - 1)))) : c0;
    const int K = min(n - 1, kHorizon);
    dd zi = p.z;
    for (int i = 1; i <= K; ++i) {
        dd t = dd_mul_d(p.gain, src(i));
        if (p.whole) t = dd_add(t, dd_mul(p.zn, dd_mul_d(p.gain, src(n - 1 - i))));
        s = dd_add(s, dd_mul(zi, t));
        zi = dd_mul(zi, p.z);
    }
    return dd_add(dd_mul(s, p.start), c0);
}

// One line of n samples: src(i) is the raw input sample (read before put(i)), get / put the line
// in the coefficient array (float64: put stores the state's rounding).
template <typename Src, typename Get, typename Put>
__device__ __forceinline__ void filter_line(int n, const Pole &p, Src src, Get get, Put put) {
    dd c = causal_start(n, p, src);
    put(0, c.hi);
    for (int i = 1; i < n; ++i) {
        c = dd_add(dd_mul_d(p.gain, src(i)), dd_mul(p.z, c));
        put(i, c.hi);
    }
    c = dd_mul(c, p.anti);
    put(n - 1, c.hi);
    for (int i = n - 2; i >= 0; --i) {
        c = dd_mul(p.z, dd_add_d(c, -get(i)));
        put(i, c.hi);
    }
}

__device__ __forceinline__ int clampi(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

// axis 0: lane = padded (y, x) column; reads the raw field through clamped indices
template <typename T>
__global__ __launch_bounds__(kLineThreads) void k_prefilter_z(SplineDims d, Pole p, const T *__restrict__ in,
                                                             double *__restrict__ C) {
    const int64_t Nx = d.px(), Ny = d.py();
    const int64_t col = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (col >= Nx * Ny) return;
    const int y = (int)(col / Nx), x = (int)(col - (int64_t)y * Nx);
    const int64_t plane_in = (int64_t)d.nx * d.ny, plane = Nx * Ny;
    const T *src0 = in + (int64_t)clampi(y - kPad, d.ny - 1) * d.nx + clampi(x - kPad, d.nx - 1);
    double *dst = C + col;
    const int nzm = d.nz - 1;
    filter_line((int)d.pz(), p,
                [&](int i) { return (double)src0[(int64_t)clampi(i - kPad, nzm) * plane_in]; },
                [&](int i) { return dst[(int64_t)i * plane]; },
                [&](int i, double v) { dst[(int64_t)i * plane] = v; });
}

// axis 1: lane = (z, x) column of the padded array, in place
__global__ __launch_bounds__(kLineThreads) void k_prefilter_y(SplineDims d, Pole p, double *__restrict__ C) {
    const int64_t Nx = d.px(), Ny = d.py(), Nz = d.pz();
    const int64_t idx = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (idx >= Nx * Nz) return;
    const int64_t z = idx / Nx, x = idx - z * Nx;
    double *dst = C + z * Ny * Nx + x;
    filter_line((int)Ny, p, [&](int i) { return dst[(int64_t)i * Nx]; },
                [&](int i) { return dst[(int64_t)i * Nx]; }, [&](int i, double v) { dst[(int64_t)i * Nx] = v; });
}

// axis 2: one wave per 64 lines, 64-column chunks staged in LDS
__global__ __launch_bounds__(kTile) void k_prefilter_x(SplineDims d, Pole p, double *__restrict__ C) {
    __shared__ double tile[kTile][kTile + 1];
    const int n = (int)d.px();
    const int64_t nrows = d.py() * d.pz();
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int lane = (int)threadIdx.x;
    const int rows = (int)min((int64_t)kTile, nrows - r0);
    const bool mine = lane < rows;
    const int nchunks = (n + kTile - 1) / kTile;
    double *base = C + r0 * n;
    dd c{0.0, 0.0};
    for (int ch = 0; ch < nchunks; ++ch) {  // forward
        const int c0 = ch * kTile, w = min(kTile, n - c0);
        for (int r = 0; r < rows; ++r)
            if (lane < w) tile[r][lane] = base[(int64_t)r * n + c0 + lane];
        __syncthreads();
        if (mine) {
            int i = 0;
            if (ch == 0) {  // the horizon lies inside the first chunk; a whole line (n <= 41) is one chunk
                c = causal_start(n, p, [&](int k) { return tile[lane][k]; });
                tile[lane][0] = c.hi;
                i = 1;
            }
            for (; i < w; ++i) {
                c = dd_add(dd_mul_d(p.gain, tile[lane][i]), dd_mul(p.z, c));
                tile[lane][i] = c.hi;
            }
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            if (lane < w) base[(int64_t)r * n + c0 + lane] = tile[r][lane];
        __syncthreads();
    }
    for (int ch = nchunks - 1; ch >= 0; --ch) {  // backward
        const int c0 = ch * kTile, w = min(kTile, n - c0);
        for (int r = 0; r < rows; ++r)
            if (lane < w) tile[r][lane] = base[(int64_t)r * n + c0 + lane];
        __syncthreads();
        if (mine) {
            int i = w - 1;
            if (ch == nchunks - 1) {
                c = dd_mul(c, p.anti);  // c still holds this sample unrounded: the forward sweep ended on it
                tile[lane][i] = c.hi;
                --i;
            }
            for (; i >= 0; --i) {
                c = dd_mul(p.z, dd_add_d(c, -tile[lane][i]));
                tile[lane][i] = c.hi;
            }
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            if (lane < w) base[(int64_t)r * n + c0 + lane] = tile[r][lane];
        __syncthreads();
    }
}

// ---- sampling ----
// a coordinate clamped to [0, hi]; NaN gives 0, so that every index below is in bounds
__device__ __forceinline__ double clampc(double c, double hi) {
    c = c > 0.0 ? c : 0.0;
    return c < hi ? c : hi;
}

// Where a coordinate a + b of the raw field's index space falls in an array of extent N that
// starts `pad` samples before it: the index of floor and the fraction, clamped to [-over, N - 1 +
// over] in the array's own index space.  Order 1 samples the raw field with over = 0: the cell is an
// index.  Order 3 samples the padded coefficients with over = 1, which is scipy's rule: one sample
// past either end the fraction is kept and only the four indices are edge-extended (cubic_axis), at
// -1 and at N the value saturates, and any coordinate beyond (however large) gives that same cell.
// The fraction is (a - floor) + b as a double-double, so the rounding of a + b (at the magnitude of
// the coordinate) does not enter the weights; a - floor is exact for a float32-born a.  NaN gives
// the low end.
struct Cell {
    int64_t i;
    dd t;
};
__device__ __forceinline__ Cell cell_of(double a, double b, int pad, int64_t N, int over) {
    const double c = a + b;
    if (!(c > -(double)(pad + over))) return Cell{-(int64_t)over, dd{0.0, 0.0}};
    if (c >= (double)(N - 1 - pad + over)) return Cell{N - 1 + over, dd{0.0, 0.0}};
    const double f = floor(c);
    return Cell{(int64_t)f + pad, two_sum(a - f, b)};
}

// the cubic B-spline weights at fraction t and the four clamped indices from i - 1
struct Cubic {
    dd w[3][4];
    int64_t ix[3][4];
};
__device__ __forceinline__ void cubic_axis(Cubic &q, int a, Cell c, int64_t N) {
    const dd t = c.t, u = dd_sub(dd{1.0, 0.0}, t);
    const dd tt = dd_mul(t, t), uu = dd_mul(u, u);
    q.w[a][0] = dd_div_d(dd_mul(uu, u), 6.0);
    q.w[a][1] = dd_div_d(dd_add_d(dd_mul_d(dd_mul(tt, dd_add_d(t, -2.0)), 3.0), 4.0), 6.0);
    q.w[a][2] = dd_div_d(dd_add_d(dd_mul_d(dd_mul(uu, dd_add_d(u, -2.0)), 3.0), 4.0), 6.0);
    q.w[a][3] = dd_div_d(dd_mul(tt, t), 6.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = c.i - 1 + k;
        q.ix[a][k] = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    }
}

// order 3 on the padded coefficients C (Nz, Ny, Nx): 16 row sums, 4 plane sums, one value
__device__ __forceinline__ dd sample3(const double *__restrict__ C, int64_t Ny, int64_t Nx, const Cubic &q) {
    dd sz{0.0, 0.0};
#pragma unroll
    for (int kz = 0; kz < 4; ++kz) {
        dd sy{0.0, 0.0};
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const double *row = C + (q.ix[0][kz] * Ny + q.ix[1][ky]) * Nx;
            dd sx = dd_mul_d(q.w[2][0], row[q.ix[2][0]]);
#pragma unroll
            for (int kx = 1; kx < 4; ++kx) sx = dd_add(sx, dd_mul_d(q.w[2][kx], row[q.ix[2][kx]]));
            sy = dd_add(sy, dd_mul(q.w[1][ky], sx));
        }
        sz = dd_add(sz, dd_mul(q.w[0][kz], sy));
    }
    return sz;
}

// order 1 on the raw field F (nz, ny, nx) at the cells c[3] (pad 0)
template <typename T>
__device__ __forceinline__ dd sample1(const T *__restrict__ F, int nz, int ny, int nx, const Cell c[3]) {
    const int N[3] = {nz, ny, nx};
    int64_t i1[3];
    dd w0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        i1[a] = min(c[a].i + 1, (int64_t)N[a] - 1);
        w0[a] = dd_sub(dd{1.0, 0.0}, c[a].t);
    }
    dd sz{0.0, 0.0};
#pragma unroll
    for (int kz = 0; kz < 2; ++kz) {
        dd sy{0.0, 0.0};
#pragma unroll
        for (int ky = 0; ky < 2; ++ky) {
            const T *row = F + ((kz ? i1[0] : c[0].i) * ny + (ky ? i1[1] : c[1].i)) * nx;
            const dd sx = dd_add(dd_mul_d(w0[2], (double)row[c[2].i]), dd_mul_d(c[2].t, (double)row[i1[2]]));
            sy = dd_add(sy, dd_mul(ky ? c[1].t : w0[1], sx));
        }
        sz = dd_add(sz, dd_mul(kz ? c[0].t : w0[0], sy));
    }
    if (sz.hi - sz.hi == 0.0) return sz;
    // A non-finite sample among the eight: the products' error terms are Inf - Inf, so the sum above is
    // NaN whatever the kind.  scipy's plain sum, corner by corner, keeps +-Inf under a positive weight
    // and gives NaN under a zero one; its kind is the result's.
    double plain = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int kz = k >> 2, ky = (k >> 1) & 1, kx = k & 1;
        const double v = (double)F[((kz ? i1[0] : c[0].i) * ny + (ky ? i1[1] : c[1].i)) * nx + (kx ? i1[2] : c[2].i)];
        plain += ((v * (kz ? c[0].t.hi : w0[0].hi)) * (ky ? c[1].t.hi : w0[1].hi)) * (kx ? c[2].t.hi : w0[2].hi);
    }
    return dd{plain, 0.0};
}

// order 0: the linear index of the sample at floor(c + 0.5), clamped
__device__ __forceinline__ int64_t index0(int nz, int ny, int nx, double cz, double cy, double cx) {
    const int64_t iz = (int64_t)floor(clampc(cz, (double)(nz - 1)) + 0.5);
    const int64_t iy = (int64_t)floor(clampc(cy, (double)(ny - 1)) + 0.5);
    const int64_t jx = (int64_t)floor(clampc(cx, (double)(nx - 1)) + 0.5);
    return (iz * ny + iy) * nx + jx;
}

template <typename T, int ORDER>
__global__ __launch_bounds__(kLineThreads) void k_map_coordinates(SplineDims d, const T *__restrict__ src,
                                                                  const double *__restrict__ coords, int64_t n,
                                                                  double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (i >= n) return;
    const double co[3] = {coords[i], coords[n + i], coords[2 * n + i]};
    const bool bad = co[0] != co[0] || co[1] != co[1] || co[2] != co[2];
    if constexpr (ORDER == 3) {
        const int64_t N[3] = {d.pz(), d.py(), d.px()};
        Cubic q;
#pragma unroll
        for (int a = 0; a < 3; ++a) cubic_axis(q, a, cell_of(co[a], 0.0, kPad, N[a], 1), N[a]);
        out[i] = bad ? nan("") : sample3((const double *)src, N[1], N[2], q).hi;
    } else if constexpr (ORDER == 1) {
        const Cell c[3] = {cell_of(co[0], 0.0, 0, d.nz, 0), cell_of(co[1], 0.0, 0, d.ny, 0),
                           cell_of(co[2], 0.0, 0, d.nx, 0)};
        out[i] = bad ? nan("") : sample1<T>(src, d.nz, d.ny, d.nx, c).hi;
    } else {
        out[i] = (double)src[index0(d.nz, d.ny, d.nx, co[0], co[1], co[2])];
    }
}

// ---- traction integration ----
template <typename T, typename VT>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_terms(
    MeshArgs a, const T *__restrict__ U, const T *__restrict__ V, const T *__restrict__ W, const T *__restrict__ P,
    const uint8_t *__restrict__ bg, const double *__restrict__ CU, const double *__restrict__ CV,
    const double *__restrict__ CW, const VT *__restrict__ verts, const int32_t *__restrict__ faces,
    const int64_t *__restrict__ tri_offsets, const int32_t *__restrict__ blk_label,
    const int64_t *__restrict__ blk_first, double *__restrict__ part) {
    __shared__ double sh[kMeshSums][kMeshThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lab = blk_label[blockIdx.x];
    const int64_t tri = blk_first[blockIdx.x] + tid;
    double term[kMeshSums];
#pragma unroll
    for (int k = 0; k < kMeshSums; ++k) term[k] = 0.0;
    if (tri < tri_offsets[lab + 1]) {
        const int nz = a.d.nz, ny = a.d.ny, nx = a.d.nx;
        VT vt[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            int64_t vi = faces[tri * 3 + j];
            vi = vi < 0 ? 0 : (vi > a.n_verts - 1 ? a.n_verts - 1 : vi);
#pragma unroll
            for (int c = 0; c < 3; ++c) vt[j][c] = verts[vi * 3 + c];
        }
        // the centroid and the edge differences in the vertices' own dtype, as numpy keeps them
        double cen[3], e1[3], e2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const VT sum = (vt[0][c] + vt[1][c]) + vt[2][c];
            cen[c] = (double)(sum / (VT)3);
            e1[c] = (double)(VT)(vt[1][c] - vt[0][c]) * a.h[c];
            e2[c] = (double)(VT)(vt[2][c] - vt[0][c]) * a.h[c];
        }
        double ns[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]),
                        0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
        const double area = sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]);
        const double den = area > 1e-20 ? area : 1e-20;
        double nph[3], nvx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nph[c] = ns[c] / den;
            nvx[c] = nph[c] / a.h[c];
        }
        const double nn = sqrt((nvx[0] * nvx[0] + nvx[1] * nvx[1]) + nvx[2] * nvx[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) nvx[c] = nvx[c] / nn;  // 0 / 0 for a zero-area triangle
        const double q0 = nvx[0] * a.h[0], q1 = nvx[1] * a.h[1], q2 = nvx[2] * a.h[2];
        const double dphys = 0.25 * sqrt((q0 * q0 + q1 * q1) + q2 * q2);
        double off[3], outc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            off[c] = 0.25 * nvx[c];
            outc[c] = cen[c] - off[c];
        }
        const int64_t N[3] = {a.d.pz(), a.d.py(), a.d.px()};
        const int n3[3] = {nz, ny, nx};
        Cubic q;
        Cell at[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cubic_axis(q, c, cell_of(cen[c], off[c], kPad, N[c], 1), N[c]);  // the offset sample: centroid + 0.25 n
            at[c] = cell_of(cen[c], 0.0, 0, n3[c], 0);                      // the centroid
        }
        const T *fld[3] = {U, V, W};
        const double *cf[3] = {CU, CV, CW};
        double tv[3];  // x, y, z
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const dd inner = sample3(cf[k], N[1], N[2], q);
            const dd diff = dd_sub(sample1<T>(fld[k], nz, ny, nx, at), inner);
            tv[k] = dd_div_d(dd_mul_d(diff, a.viscosity), dphys).hi;  // rounded once, after the difference
        }
        const double p = P ? sample1<T>(P, nz, ny, nx, at).hi : 0.0;
        const bool water = bg ? bg[index0(nz, ny, nx, outc[0], outc[1], outc[2])] != 0 : true;
        const double nrm[3] = {nph[2], nph[1], nph[0]};             // x, y, z
        const double dot = (tv[0] * nrm[0] + tv[1] * nrm[1]) + tv[2] * nrm[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double tp = p * nrm[c];
            const double nor = dot * nrm[c];
            const double tan = tv[c] - nor;
            const double both = (tv[c] + tp) * area;
            term[c] = tv[c] * area;
            term[3 + c] = tan * area;
            term[6 + c] = nor * area;
            term[9 + c] = tp * area;
            term[13 + c] = water ? both : 0.0;
            term[16 + c] = water ? 0.0 : both;
        }
        term[12] = area;
        term[19] = water ? area : 0.0;
        term[20] = water ? 0.0 : area;
    }
#pragma unroll
    for (int k = 0; k < kMeshSums; ++k) {
        const double v = group_reduce<0x3f>(term[k], OpAdd{});
        if (lane == 0) sh[k][wave] = v;
    }
    __syncthreads();
    if (tid < kMeshSums) {
        double s = sh[tid][0];
#pragma unroll
        for (int k = 1; k < kMeshThreads / 64; ++k) s += sh[tid][k];
        part[(int64_t)blockIdx.x * kMeshSums + tid] = s;
    }
}

// block (label, key) adds the label's partials in a fixed order: thread t takes its blocks t,
// t + 256, ...; then the wave tree and the four waves in order
__global__ __launch_bounds__(kMeshThreads) void k_mesh_final(const double *__restrict__ part,
                                                             const int64_t *__restrict__ lab_blk0,
                                                             double *__restrict__ res) {
    __shared__ double sh[kMeshThreads / 64];
    const int lab = (int)blockIdx.x, key = (int)blockIdx.y;
    const int64_t b0 = lab_blk0[lab], b1 = lab_blk0[lab + 1];
    double v = 0.0;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += kMeshThreads) v += part[b * kMeshSums + key];
    v = group_reduce<0x3f>(v, OpAdd{});
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = sh[0];
    for (int k = 1; k < kMeshThreads / 64; ++k) s += sh[k];
    res[(int64_t)lab * kMeshSums + key] = s;
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <typename T>
int prefilter_t(const SplineDims &d, const T *field, double *coef, hipStream_t s) {
    const Pole pz = make_pole(d.pz()), py = make_pole(d.py()), px = make_pole(d.px());
    hipLaunchKernelGGL((k_prefilter_z<T>), dim3(blocks_of(d.px() * d.py(), kLineThreads)), dim3(kLineThreads), 0, s, d,
                       pz, field, coef);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_prefilter_y, dim3(blocks_of(d.px() * d.pz(), kLineThreads)), dim3(kLineThreads), 0, s, d, py,
                       coef);
    PTV_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_prefilter_x, dim3(blocks_of(d.py() * d.pz(), kTile)), dim3(kTile), 0, s, d, px, coef);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

template <typename T>
int map_t(const SplineDims &d, int order, const T *src, const double *coords, int64_t n, double *out, hipStream_t s) {
    const dim3 grid(blocks_of(n, kLineThreads)), block(kLineThreads);
    if (order == 3) hipLaunchKernelGGL((k_map_coordinates<T, 3>), grid, block, 0, s, d, src, coords, n, out);
    else if (order == 1) hipLaunchKernelGGL((k_map_coordinates<T, 1>), grid, block, 0, s, d, src, coords, n, out);
    else hipLaunchKernelGGL((k_map_coordinates<T, 0>), grid, block, 0, s, d, src, coords, n, out);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

template <typename T, typename VT>
int mesh_t(const MeshArgs &a, const void *U, const void *V, const void *W, const void *P, const uint8_t *bg,
           const double *const coef[3], const void *verts, const int32_t *faces, const int64_t *tri_offsets,
           const int32_t *blk_label, const int64_t *blk_first, const int64_t *lab_blk0, int64_t nblocks, double *part,
           double *res, hipStream_t s) {
    if (nblocks > 0) {
        hipLaunchKernelGGL((k_mesh_terms<T, VT>), dim3((unsigned)nblocks), dim3(kMeshThreads), 0, s, a, (const T *)U,
                           (const T *)V, (const T *)W, (const T *)P, bg, coef[0], coef[1], coef[2], (const VT *)verts,
                           faces, tri_offsets, blk_label, blk_first, part);
        PTV_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mesh_final, dim3((unsigned)a.n_labels, kMeshSums), dim3(kMeshThreads), 0, s, part, lab_blk0,
                       res);
    PTV_HIP(hipGetLastError());
    return PTV_OK;
}

}  // namespace

int launch_spline_prefilter(const SplineDims &d, const void *field, bool f32, double *coef, hipStream_t s) {
    if (f32) return prefilter_t<float>(d, (const float *)field, coef, s);
    return prefilter_t<double>(d, (const double *)field, coef, s);
}

int launch_map_coordinates(const SplineDims &d, int order, const void *src, bool f32, const double *coords, int64_t n,
                           double *out, hipStream_t s) {
    if (n == 0) return PTV_OK;
    if (order == 3 || !f32) return map_t<double>(d, order, (const double *)src, coords, n, out, s);
    return map_t<float>(d, order, (const float *)src, coords, n, out, s);
}

int64_t mesh_blocks(const int64_t *tri_offsets, int n_labels) {
    int64_t nb = 0;
    for (int l = 0; l < n_labels; ++l) nb += (tri_offsets[l + 1] - tri_offsets[l] + kMeshThreads - 1) / kMeshThreads;
    return nb;
}

int launch_mesh_drag(const MeshArgs &a, const void *U, const void *V, const void *W, const void *P, const uint8_t *bg,
                     const double *const coef[3], const void *verts, const int32_t *faces, const int64_t *tri_offsets,
                     const int32_t *blk_label, const int64_t *blk_first, const int64_t *lab_blk0, int64_t nblocks,
                     double *part, double *res, hipStream_t s) {
#define PTV_MESH_ARGS a, U, V, W, P, bg, coef, verts, faces, tri_offsets, blk_label, blk_first, lab_blk0, nblocks, part, res, s
    if (a.field_f32) return a.vert_f32 ? mesh_t<float, float>(PTV_MESH_ARGS) : mesh_t<float, double>(PTV_MESH_ARGS);
    return a.vert_f32 ? mesh_t<double, float>(PTV_MESH_ARGS) : mesh_t<double, double>(PTV_MESH_ARGS);
#undef PTV_MESH_ARGS
}

}  // namespace ptv
