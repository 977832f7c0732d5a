// Host check of rcp_in (ptv_knn_impl.hpp): the gfx9 f64 division expansion for 1 / b, emulated with
// fma, in its full form (v_div_scale pair, v_div_fmas, v_div_fixup, written out from the ISA
// manual's pseudo-code) and in the short in-range form, over b in [2^-750, 2^750].
//
//     c++ -O2 -std=c++17 -ffp-contract=off tools/rcp_guard_check.cpp -o rcp_guard_check && ./rcp_guard_check [millions]
//
// The hardware reciprocal seed is not reproduced: half the operands take a seed anywhere within
// 2^-22 of 1 / b, the other half the correctly rounded one.  Checked per operand: both scale steps
// return their operand and leave vcc clear, the fixup passes the quotient through, and the full
// and the short form give the same bits (the claim rcp_in rests on: it is the compiler's own
// sequence for 1.0 / b less its identities); with the rounded seed both also equal 1.0 / b.  With
// a perturbed seed the last step can miss the IEEE quotient next to a power of two, in both forms
// alike; that count is printed for information.  Exit 1 on any miss.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static int expo(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return (int)((b >> 52) & 0x7ff);
}
static bool denorm(double x) { return x != 0.0 && expo(x) == 0; }

// V_DIV_SCALE_F64 D, S0, S1 (denominator), S2 (numerator); S0 is S1 or S2
static double div_scale(double s0, double s1, double s2, bool &vcc) {
    vcc = false;
    if (s2 == 0.0 || s1 == 0.0) return NAN;
    if (expo(s2) - expo(s1) >= 768) {
        vcc = true;
        return s0 == s1 ? std::ldexp(s0, 128) : s0;
    }
    if (denorm(s1)) return std::ldexp(s0, 128);
    const bool rcp_dn = denorm(1.0 / s1), q_dn = denorm(s2 / s1);
    if (rcp_dn && q_dn) {
        vcc = true;
        return s0 == s1 ? std::ldexp(s0, -128) : s0;
    }
    if (rcp_dn) return std::ldexp(s0, -128);
    if (q_dn) {
        vcc = true;
        return s0 == s2 ? std::ldexp(s0, 128) : s0;
    }
    if (expo(s2) <= 53) return std::ldexp(s0, 128);
    return s0;
}
static double div_fmas(double a, double b, double c, bool vcc) {
    const double r = std::fma(a, b, c);
    return vcc ? std::ldexp(r, 128) : r;  // (the scale direction does not matter here: vcc must be clear)
}
// V_DIV_FIXUP_F64 for finite, nonzero, normal S1 (denominator) and S2 (numerator)
static double div_fixup(double q, double s1, double s2) {
    const int d = expo(s2) - expo(s1);
    if (d < -1075) return 0.0;
    if (d > 1023) return INFINITY;
    return std::signbit(s1) != std::signbit(s2) ? -std::fabs(q) : std::fabs(q);
}

static bool scale_id = true;
static double full(double b, double seed_err) {
    bool v0, v1;
    const double d0 = div_scale(b, b, 1.0, v0);
    const double n0 = div_scale(1.0, b, 1.0, v1);
    if (d0 != b || n0 != 1.0 || v0 || v1) scale_id = false;
    double r = (1.0 / d0) * (1.0 + seed_err);
    r = std::fma(r, std::fma(-d0, r, 1.0), r);
    r = std::fma(r, std::fma(-d0, r, 1.0), r);
    const double q = n0 * r;
    const double e = std::fma(-d0, q, n0);
    const double f = div_fmas(e, r, q, v1);
    const double o = div_fixup(f, b, 1.0);
    if (o != f) scale_id = false;
    return o;
}
static double in_range(double b, double seed_err) {
    double r = (1.0 / b) * (1.0 + seed_err);
    r = std::fma(std::fma(-b, r, 1.0), r, r);
    r = std::fma(std::fma(-b, r, 1.0), r, r);
    return std::fma(std::fma(-b, r, 1.0), r, r);
}

int main(int argc, char **argv) {
    const long long n = (argc > 1 ? std::atoll(argv[1]) : 400) * 1000000LL;
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> mant(1.0, 2.0), serr(-0x1p-22, 0x1p-22);
    std::uniform_int_distribution<int> ex(-750, 749);
    long long bad = 0, done = 0, off_ieee = 0;
    auto one = [&](double b, double se) {
        const double want = 1.0 / b, f = full(b, se), s = in_range(b, se);
        if (se != 0.0 && f == s && f != want) ++off_ieee;
        if (f != s || !scale_id || (se == 0.0 && f != want)) {
            if (bad < 10) std::printf("miss: b=%a seed_err=%a full=%a short=%a want=%a scale_id=%d\n", b, se, f, s, want, (int)scale_id);
            ++bad;
            scale_id = true;
        }
        ++done;
    };
    // edges of the range and the neighbours of every power of two in it
    for (int e = -750; e <= 750; ++e) {
        const double p = std::ldexp(1.0, e);
        for (double b : {p, std::nextafter(p, INFINITY), e > -750 ? std::nextafter(p, 0.0) : p, e < 750 ? p * (2.0 - 0x1p-52) : p})
            for (double se : {0.0, 0x1p-22, -0x1p-22, 0x1p-30, -0x1p-30}) one(b, se);
    }
    while (done < n) one(std::ldexp(mant(rng), ex(rng)), (done & 1) ? serr(rng) : 0.0);
    std::printf("rcp_in guard [2^-750, 2^750]: %lld operands, %lld misses (%lld perturbed-seed results off the IEEE quotient, both forms alike)\n", done, bad, off_ieee);
    return bad != 0;
}
