// ptv_knn_epilogue.hpp — the weight-and-sum epilogue of the packed-key lists (13 <= k <= 127).
//
// A part of ptv_knn_impl.hpp, included there after the helpers it uses (KnnKernelArgs, sqrt_cr,
// np_pow, div_by, div_by_ok) and before the kernel.  Each pass of the reference is written once:
// interpolator.py:102-122 (Sibson, four passes), :142-153 (IDW, two).  What depends on the list
// length is how a pass walks its blocks of neighbours and where a block's distances come from
// (KeyBlocks below).
#pragma once

#include <type_traits>

namespace ptv {

// __forceinline__ for the epilogue's lambdas (the pass bodies handed to for_blocks and their
// helpers): none may stay a call, their arrays are registers only once everything is one function
#define PTV_LAMBDA_INLINE __attribute__((always_inline))

// numpy's pairwise sum (see pairwise()) of n >= 8 values fed in index order in blocks of 8: block m
// holds a[m .. m + 7] (entries at or past n ignored).  Key lists serve k >= 13 only (kmax_for), so
// numpy's sequential sum of fewer than 8 values is not needed here.
struct PairwiseStream {
    double r[8];
    double res;  // n >= 8: the tail block or finish() assigns it before anything reads it
    // W entries of block m, m + W h .. m + W h + W - 1: the whole block (W = 8, h = 0) or one of its
    // halves (W = 4, h = 0 then 1).  Each entry meets the same accumulator or running sum in the same
    // order either way.
    template <int W>
    __device__ __forceinline__ void add(int m, int h, int n, const double (&a)[W]) {
        const int stop = n - (n & 7);
        if (m == 0) {
#pragma unroll
            for (int i = 0; i < W; ++i) r[W * h + i] = a[i];
        } else if (m < stop) {
#pragma unroll
            for (int i = 0; i < W; ++i) r[W * h + i] += a[i];
        } else {  // the tail block (n % 8 entries), after the tree of the accumulators
            if (h == 0) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (m + W * h + i < n) res += a[i];
        }
    }
    __device__ __forceinline__ double finish(int n) {
        if ((n & 7) == 0) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        return res;
    }
};

// How the epilogue of a KMAX-slot key list walks its blocks of 8 neighbours:
//   KMAX <= 32 (the 3-wave lists): unrolled, every block in two halves of W = 4 (spilled VGPRs at
//     24 / 32 slots: 30 / 98 -> 0 / 22; IDW k = 24 46.0 -> 45.0 ms, Sibson k = 30 unchanged);
//   up to PTV_KNN_UNROLL_MAX (the 2-wave lists): unrolled, whole blocks (IDW / Sibson k = 50 +1.3 /
//     +2.6 % in halves; profiles/r06_ab/value_half_blocks_ab.txt).  Unrolled, the loads of different
//     blocks overlap: Sibson k = 30 79 vs 92 ms rolled at 3 waves per SIMD, Sibson k = 50 100 vs 137
//     at 2;
//   longer lists: one rolled loop per pass (unrolled they are tens of KB of straight-line code per
//     wave and spill: see PTV_KNN_UNROLL_MAX).
// The unrolled forms keep every entry's distance (then weight) in registers between the passes and
// read each slot where it is used; the rolled form fetches a block's 8 slots once, gathers its
// records again in every pass and derives d and w from d2 each time.
template <int KMAX>
struct KeyBlocks {
    static constexpr bool ROLLED = KMAX > PTV_KNN_UNROLL_MAX;
    static constexpr int W = !ROLLED && KMAX <= 32 ? 4 : 8;
};

// body(m, h) for every block m = 0, 8, .. below k, and every part h of it (W entries from m + W h)
template <int KMAX, class Body>
__device__ __forceinline__ void for_blocks(int k, Body &&body) {
    if constexpr (KeyBlocks<KMAX>::ROLLED) {
#pragma unroll 1
        for (int m = 0; m < k; m += 8) body(m, 0);
    } else {
#pragma unroll
        for (int m = 0; m < KMAX; m += 8) {
            if (m < k) {
#pragma unroll
                for (int h = 0; h < 8 / KeyBlocks<KMAX>::W; ++h) body(m, h);
            }
        }
    }
}

// Key-list interpolation (k >= 13) of one voxel: the weights are streamed in blocks of 8 neighbours
// from the exact d2, recomputed from the records (the keys hold truncated d2), in the reference's
// order.  slot_at(j): the slot of list entry j (0 .. k - 1 ascending; up to KMAX - 1 readable).
// False (wave-uniform): some lane's list is ambiguous (amb) or came out of order, the tile goes
// to the exact repair launch and out is not set.
template <int KMAX, class SlotAt>
__device__ __forceinline__ bool keylist_interp(const KnnKernelArgs &a, const double4 *prec, const double4 *pval,
                                               double qx, double qy, double qz, const SlotAt &slot_at, bool amb,
                                               double (&out)[3]) {
    constexpr bool ROLLED = KeyBlocks<KMAX>::ROLLED;
    constexpr int W = KeyBlocks<KMAX>::W;
    const int k = a.k;
    double dk[ROLLED ? 1 : KMAX];  // unrolled: the kept entries (Sibson: d_j, then w_j; IDW: d2_j)
    auto keep = [&](int j, double v) PTV_LAMBDA_INLINE {
        if constexpr (!ROLLED) {
            if (j < KMAX) dk[min(j, KMAX - 1)] = v;
        }
    };
    // rolled: the slots of block m from the LDS slot list (entries past k: entry 0's, a valid slot)
    struct Slots {
        int s[ROLLED ? 8 : 1];
    };
    auto block_slots = [&](int m, Slots &b) PTV_LAMBDA_INLINE {
        if constexpr (ROLLED) {
            const int s0 = slot_at(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) b.s[i] = m + i < k ? slot_at(m + i) : s0;
        }
    };
    // the slot of entry j, the i-th of its block
    auto slot = [&](const Slots &b, int j, int i) PTV_LAMBDA_INLINE -> int {
        if constexpr (ROLLED) return b.s[i];
        else return j < k ? slot_at(min(j, KMAX - 1)) : slot_at(0);
    };
    // x, y, z (or u, v, w) of the W records from entry j0: 24 of each record's 32 bytes (at W = 8,
    // 48 registers in flight, not 64)
    auto xyz_block = [&](const double4 *src, const Slots &b, int j0, double (&x)[W], double (&y)[W], double (&z)[W]) PTV_LAMBDA_INLINE {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const double *r = reinterpret_cast<const double *>(src + slot(b, j0 + i, i));
            const double2 xy = *reinterpret_cast<const double2 *>(r);
            x[i] = xy.x;
            y[i] = xy.y;
            z[i] = r[2];
        }
    };
    // exact d2 from this lane's query, bit-identical to the search's
    auto d2_of = [&](double x, double y, double z) PTV_LAMBDA_INLINE {
        const double dx = qx - x, dy = qy - y, dz = qz - z;
        return (dx * dx + dy * dy) + dz * dz;
    };
    auto d2_block = [&](const Slots &b, int j0, double (&d2)[W]) PTV_LAMBDA_INLINE {
        if constexpr (ROLLED) {
            double x[W], y[W], z[W];
            xyz_block(prec, b, j0, x, y, z);
#pragma unroll
            for (int i = 0; i < W; ++i) d2[i] = d2_of(x[i], y[i], z[i]);
        } else {
            double4 rc[W];
#pragma unroll
            for (int i = 0; i < W; ++i) rc[i] = prec[slot(b, j0 + i, i)];
#pragma unroll
            for (int i = 0; i < W; ++i) d2[i] = d2_of(rc[i].x, rc[i].y, rc[i].z);
        }
    };
    // what the passes after the first start from: the kept entries, or (rolled) d2 gathered again
    auto reload = [&](const Slots &b, int j0, double (&x)[W]) PTV_LAMBDA_INLINE {
        if constexpr (ROLLED) {
            d2_block(b, j0, x);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) x[i] = dk[min(j0 + i, KMAX - 1)];
        }
    };
    // The last pass of either method: normalised weights times the values, three pairwise sums.
    // wn_of(x, fast): the normalised weight from an entry of reload().  Unrolled, the value gathers
    // go first and every product follows its weight; rolled, one gather is in flight at a time (d2,
    // the weights, then the values), and with hoist the loop branches on fast once per block.
    auto value_pass = [&](auto hoist, bool fast, auto &&wn_of) PTV_LAMBDA_INLINE {
        PairwiseStream pu, pv, pw;
        for_blocks<KMAX>(k, [&](int m, int h) PTV_LAMBDA_INLINE {
            const int j0 = m + W * h;
            Slots b;
            block_slots(m, b);
            double x[W], wn[W], tu[W], tv[W], tw[W];
            auto scale = [&](int i) PTV_LAMBDA_INLINE {
                tu[i] = wn[i] * tu[i];
                tv[i] = wn[i] * tv[i];
                tw[i] = wn[i] * tw[i];
            };
            if constexpr (ROLLED) {
                reload(b, j0, x);
                if constexpr (decltype(hoist)::value) {
                    if (fast) {
#pragma unroll
                        for (int i = 0; i < W; ++i) wn[i] = wn_of(x[i], true);
                    } else {
#pragma unroll
                        for (int i = 0; i < W; ++i) wn[i] = wn_of(x[i], false);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < W; ++i) wn[i] = wn_of(x[i], fast);
                }
                xyz_block(pval, b, j0, tu, tv, tw);
#pragma unroll
                for (int i = 0; i < W; ++i) scale(i);
            } else {
                xyz_block(pval, b, j0, tu, tv, tw);
                reload(b, j0, x);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    wn[i] = wn_of(x[i], fast);
                    scale(i);
                }
            }
            pu.add<W>(m, h, k, tu);
            pv.add<W>(m, h, k, tv);
            pw.add<W>(m, h, k, tw);
        });
        out[0] = pu.finish(k);
        out[1] = pv.finish(k);
        out[2] = pw.finish(k);
    };
    bool ok = true;
    double prev = -1.0;
    if (a.method == PTV_METHOD_SIBSON) {
        // pass 1: d, 1/(d + eps) -> sum (pairwise), sum d -> mean; the order check
        PairwiseStream ps_inv, ps_d;
        double ivmin = INFINITY, dmax = 0.0, dmin_nz = INFINITY;  // operand ranges for div_by below
        for_blocks<KMAX>(k, [&](int m, int h) PTV_LAMBDA_INLINE {
            const int j0 = m + W * h;
            Slots b;
            block_slots(m, b);
            double d2[W], dv[W], iv[W];
            d2_block(b, j0, d2);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                dv[i] = sqrt_cr(d2[i]);
                iv[i] = 1.0 / (dv[i] + a.eps);
                if (j0 + i < k) {
                    ok = ok && !(d2[i] < prev);
                    prev = d2[i];
                    ivmin = fmin(ivmin, iv[i]);
                    dmax = fmax(dmax, dv[i]);
                    if (dv[i] > 0.0) dmin_nz = fmin(dmin_nz, dv[i]);
                }
                keep(j0 + i, dv[i]);
            }
            ps_inv.add<W>(m, h, k, iv);
            ps_d.add<W>(m, h, k, dv);
        });
        if (__builtin_amdgcn_ballot_w64(amb || !ok) != 0) return false;
        const double s_inv = ps_inv.finish(k);
        const double mean = ps_d.finish(k) / (double)k;
        // d of an entry of reload()
        auto dist = [&](double x) PTV_LAMBDA_INLINE {
            if constexpr (ROLLED) return sqrt_cr(x);
            else return x;
        };
        // pass 2: std (ddof 0)
        PairwiseStream ps_var;
        for_blocks<KMAX>(k, [&](int m, int h) PTV_LAMBDA_INLINE {
            const int j0 = m + W * h;
            Slots b;
            block_slots(m, b);
            double x[W], t[W];
            reload(b, j0, x);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const double c = dist(x[i]) - mean;
                t[i] = c * c;
            }
            ps_var.add<W>(m, h, k, t);
        });
        const double den = sqrt(ps_var.finish(k) / (double)k) + a.eps;
        // the quotients iv / s_inv and -d / den through one reciprocal each (div_by: correctly
        // rounded for normal operands and quotients; d = 0 gives 0 exactly) when every lane's
        // operands are in range, IEEE division otherwise
        const bool fdiv = __builtin_amdgcn_ballot_w64(!(div_by_ok(ivmin, s_inv, s_inv) && div_by_ok(dmin_nz, dmax, den))) == 0;
        const double rsi = 1.0 / s_inv, rden = 1.0 / den;
        auto w_of = [&](double d) PTV_LAMBDA_INLINE {
            const double iv = 1.0 / (d + a.eps);
            return fdiv ? div_by(iv, s_inv, rsi) * exp(div_by(-d, den, rden)) : iv / s_inv * exp(-d / den);
        };
        // pass 3: the exponential weights (unrolled: kept in place of the distances, pass 4 reads
        // them back) and their sum
        PairwiseStream ps_w;
        double wmin = INFINITY;
        for_blocks<KMAX>(k, [&](int m, int h) PTV_LAMBDA_INLINE {
            const int j0 = m + W * h;
            Slots b;
            block_slots(m, b);
            double x[W], w[W];
            reload(b, j0, x);
#pragma unroll
            for (int i = 0; i < W; ++i) w[i] = w_of(dist(x[i]));
#pragma unroll
            for (int i = 0; i < W; ++i) {
                if (j0 + i < k && w[i] > 0.0) wmin = fmin(wmin, w[i]);  // exp underflow: 0 / s2 exact
                keep(j0 + i, w[i]);
            }
            ps_w.add<W>(m, h, k, w);
        });
        const double s2 = ps_w.finish(k);
        // w / s2 through one reciprocal when s2, the nonzero w and every quotient are normal
        const bool fast = __builtin_amdgcn_ballot_w64(!div_by_ok(wmin, s2, s2)) == 0;
        const double rs2 = 1.0 / s2;
        // pass 4: normalised weights times the values
        value_pass(std::false_type{}, fast, [&](double x, bool f) PTV_LAMBDA_INLINE {
            double w = x;
            if constexpr (ROLLED) w = w_of(dist(x));
            return f ? div_by(w, s2, rs2) : w / s2;
        });
    } else {
        // pass 1: w = 1/(d**p + eps) -> sum (pairwise); the order check
        auto w_of = [&](double d2) PTV_LAMBDA_INLINE { return 1.0 / (np_pow(sqrt_cr(d2), a.power) + a.eps); };
        PairwiseStream ps;
        double wmin = INFINITY;
        for_blocks<KMAX>(k, [&](int m, int h) PTV_LAMBDA_INLINE {
            const int j0 = m + W * h;
            Slots b;
            block_slots(m, b);
            double d2[W], w[W];
            d2_block(b, j0, d2);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                if (j0 + i < k) {
                    ok = ok && !(d2[i] < prev);
                    prev = d2[i];
                }
                keep(j0 + i, d2[i]);
                w[i] = w_of(d2[i]);
                if (j0 + i < k) wmin = fmin(wmin, w[i]);
            }
            ps.add<W>(m, h, k, w);
        });
        if (__builtin_amdgcn_ballot_w64(amb || !ok) != 0) return false;
        const double s = ps.finish(k);
        // w_j / s through one reciprocal when every quotient is normal (see the k <= 12 path)
        const bool fast = __builtin_amdgcn_ballot_w64(!div_by_ok(wmin, s, s)) == 0;
        const double rs = 1.0 / s;
        // pass 2: normalised weights times the values
        value_pass(std::true_type{}, fast, [&](double d2, bool f) PTV_LAMBDA_INLINE {
            const double w = w_of(d2);
            return f ? div_by(w, s, rs) : w / s;
        });
    }
    return true;
}

#undef PTV_LAMBDA_INLINE

}  // namespace ptv
