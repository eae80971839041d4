// rk_divmath.h -- the binary logarithm and the binary exponential of the per-sample diversity measures (include/rappas_place.h holds
// the definition), one text for the kernel (rk_diversity.h), the host twin (rk_samples_host.h) and, operation by
// operation, tests/diversity_ref.py.  The platform's log and pow round differently on the device and on the host; these are written
// with + - * /, comparisons and integer operations on the bits of a binary64 alone, so under -ffp-contract=off every implementation
// gives the same bits.  No libm call, no fma, no table.  Not part of the C ABI.
//
//   rk_log2(x)   x = 2^e * m with m in [sqrt(1/2), sqrt(2)) from the exponent bits; s = (m - 1) / (m + 1), z = s * s;
//                ln m = 2 atanh s = 2 s (1 + z/3 + z^2/5 + ... + z^11/23): the series as it is, cut where the next term is below
//                2^-60 of the sum (z <= 0.02944); log2 x = e + (s + s * q) * (2 / ln 2).  m = 1 gives s = 0 and the result e exactly:
//                rk_log2(1.0) is +0.0, rk_log2(0.5) is -1.0.  Domain: normal x in (0, 2]; anything else gives what the bit
//                operations give (a finite number or a NaN, never a trap): the definition selects such a term away.
//   rk_exp2(y)   k = the integer nearest to y (y + 1024.5 truncated, so no rounding mode and no floor()), r = y - k exactly, t = r * ln 2,
//                e^t by its Taylor series to t^14 / 14! (|t| <= 0.3466: the next term is below 2^-62), times 2^k built from the
//                exponent bits.  rk_exp2(+-0.0) is exactly 1.0.  Domain [-512, 8]; beyond it, one rule for both sides: y that is
//                not >= -1022 (NaN included) gives +0.0 -- no subnormal result is ever formed from a k below -1022 --, y > 1023 is taken as 1023.
//   rk_pw(x, lg, theta)   x^theta from lg = rk_log2(x): rk_exp2(theta * lg) for x > 0; for x <= 0 -- reachable only where 1 - D
//                rounds to 0 -- the limit: 1.0 for theta == 0, +0.0 otherwise.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_DIVMATH_FN __host__ __device__ inline
#else
#define RK_DIVMATH_FN inline
#endif

namespace rk {

RK_DIVMATH_FN uint64_t divmath_bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
RK_DIVMATH_FN double divmath_double(uint64_t b) {
    double x;
    memcpy(&x, &b, 8);
    return x;
}

constexpr double DIV_SQRT2 = 0x1.6a09e667f3bcdp+0;     // the binary64 nearest to sqrt 2: mantissas above it are halved
constexpr double DIV_LN2 = 0x1.62e42fefa39efp-1;       // RK_LN2: the binary64 nearest to ln 2
constexpr double DIV_2_OVER_LN2 = 0x1.71547652b82fep+1;  // the binary64 nearest to 2 / ln 2

RK_DIVMATH_FN double rk_log2(double x) {
    const uint64_t b = divmath_bits(x);
    int64_t e = (int64_t)((b >> 52) & 0x7FFu) - 1023;
    double m = divmath_double((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);  // [1, 2)
    if (m > DIV_SQRT2) {
        m = m * 0.5;
        e = e + 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double q = 1.0 / 23.0;
    q = q * z + 1.0 / 21.0;
    q = q * z + 1.0 / 19.0;
    q = q * z + 1.0 / 17.0;
    q = q * z + 1.0 / 15.0;
    q = q * z + 1.0 / 13.0;
    q = q * z + 1.0 / 11.0;
    q = q * z + 1.0 / 9.0;
    q = q * z + 1.0 / 7.0;
    q = q * z + 1.0 / 5.0;
    q = q * z + 1.0 / 3.0;
    q = q * z;
    const double r = s + s * q;
    return (double)e + r * DIV_2_OVER_LN2;
}

RK_DIVMATH_FN double rk_exp2(double y) {
    if (!(y >= -1022.0)) return 0.0;
    if (y > 1023.0) y = 1023.0;
    const int64_t k = (int64_t)((y + 1024.0) + 0.5) - 1024;
    const double t = (y - (double)k) * DIV_LN2;
    double p = 1.0 / 87178291200.0;  // 1 / 14!
    p = p * t + 1.0 / 6227020800.0;
    p = p * t + 1.0 / 479001600.0;
    p = p * t + 1.0 / 39916800.0;
    p = p * t + 1.0 / 3628800.0;
    p = p * t + 1.0 / 362880.0;
    p = p * t + 1.0 / 40320.0;
    p = p * t + 1.0 / 5040.0;
    p = p * t + 1.0 / 720.0;
    p = p * t + 1.0 / 120.0;
    p = p * t + 1.0 / 24.0;
    p = p * t + 1.0 / 6.0;
    p = p * t + 0.5;
    p = p * t + 1.0;
    p = p * t + 1.0;
    return p * divmath_double((uint64_t)(k + 1023) << 52);
}

RK_DIVMATH_FN double rk_pw(double x, double lg, double theta) {
    if (x > 0.0) return rk_exp2(theta * lg);
    return theta == 0.0 ? 1.0 : 0.0;
}

constexpr uint32_t DIVERSITY_FIXED = 5, DIVERSITY_MAX_THETA = 8, DIVERSITY_LANES = 256;  // RK_DIVERSITY_*
constexpr uint64_t DIVERSITY_NAN = 0x7FF8000000000000ull;                                // the row of a sample without mass

// The terms of one half-edge of length h with distal mass a in a sample of total T (T != 0), NT thetas: term[0 .. 5 + 2 NT).  The
// indicators are tested on the integers; a term whose indicator is false is +0.0.  a == 0 leaves both false: nothing is computed.
template <uint32_t NT>
RK_DIVMATH_FN void diversity_half(uint64_t a, uint64_t T, double h, const double *theta, double *term) {
    if (a == 0) {
        for (uint32_t i = 0; i < DIVERSITY_FIXED + 2 * NT; i++) term[i] = 0.0;
        return;
    }
    const bool split = a < T;
    const double D = (double)a / (double)T;
    const double E = 1.0 - D;
    const double M = 2.0 * (E < D ? E : D);
    const double lgD = rk_log2(D);
    term[0] = h;
    term[1] = split ? h : 0.0;
    term[2] = split ? h * M : 0.0;
    term[3] = split ? h * (D * E) : 0.0;
    term[4] = h * (-(D * lgD) * DIV_LN2);
    if (NT > 0) {
        const double lgM = rk_log2(M);
        for (uint32_t i = 0; i < NT; i++) {
            term[DIVERSITY_FIXED + 2 * i] = h * rk_pw(D, lgD, theta[i]);
            term[DIVERSITY_FIXED + 2 * i + 1] = split ? h * rk_pw(M, lgM, theta[i]) : 0.0;
        }
    }
}

// One node of a sample: acc = (acc + the proximal half's term) + the distal half's, column by column
template <uint32_t NT>
RK_DIVMATH_FN void diversity_node(uint64_t c, uint64_t m, uint64_t T, double h, const double *theta, double *acc) {
    double prox[DIVERSITY_FIXED + 2 * NT], dist[DIVERSITY_FIXED + 2 * NT];
    diversity_half<NT>(c, T, h, theta, prox);
    diversity_half<NT>(c - m, T, h, theta, dist);
    for (uint32_t i = 0; i < DIVERSITY_FIXED + 2 * NT; i++) acc[i] = (acc[i] + prox[i]) + dist[i];
}

}  // namespace rk
