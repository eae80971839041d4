// rk_samplemath.h -- the terms and the chunk rule of the sample-level sums (include/rappas_place.h holds the definitions; DESIGN.md
// 4.9 - 4.11, 4.13 - 4.15), one text for the kernels (rk_samples.h, rk_epca.h, rk_kmeans.h, rk_diversity.h, rk_edgestat.h) and the
// host twins (rk_samples_host.h, rk_edgestat_host.h), in the manner of rk_divmath.h.  Each line is one rounding: under -ffp-contract=off, and from a compiler that
// forms no fma of its own, every implementation gives the same bits.  No libm call beyond fabs.  Not part of the C ABI.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_SAMPLEMATH_FN __host__ __device__ inline
#else
#define RK_SAMPLEMATH_FN inline
#endif

namespace rk {

// The KR term: what one node with half length h adds to the sum between the profiles (us, vs) and (ut, vt) -- a difference, a
// product and an add for u, then the same for v: three FP64 operations each, every one rounded by itself
RK_SAMPLEMATH_FN double kr_term(double acc, double h, double us, double ut, double vs, double vt) {
    const double term1 = h * std::fabs(us - ut);
    const double term2 = h * std::fabs(vs - vt);
    return (acc + term1) + term2;
}

// The Gram term: two roundings
RK_SAMPLEMATH_FN double gram_term(double acc, double a, double b) {
    const double term = a * b;
    return acc + term;
}

// The zero rule of edge PCA's step 6: the largest fabs that a column of S entries may have after its projections on `applied`
// columns and still count as rounding, against `scale` -- the larger of the largest fabs the product delivered it with and those of
// the live columns before it.  Per projection
// S * 2^13 * 2^-53 (include/rappas_place.h derives it): S * 2^-40 and its product with a small integer are exact, so the whole is
// one rounding.  applied == 0 gives +0.0: the plain zero test.
RK_SAMPLEMATH_FN double epca_noise_bound(uint32_t S, uint32_t applied, double scale) {
    const double per_projection = (double)S * 0x1p-40;
    return (per_projection * (double)applied) * scale;
}

// The two profiles of the edge statistics for an active sample on an edge other than the root's: the mass share
// from the integers -- one division --, and the imbalance of edge PCA's step 2 -- two divisions, an add and a subtraction
RK_SAMPLEMATH_FN double edgestat_share(uint64_t m, uint64_t T) { return (double)m / (double)T; }
RK_SAMPLEMATH_FN double edgestat_imbalance(uint64_t c, uint64_t m, uint64_t T) {
    const double t = (double)T;
    const double u = (double)c / t, v = (double)(c - m) / t;
    return (u + v) - 1.0;
}
// a centred entry: +0.0 for a sample without mass
RK_SAMPLEMATH_FN double edgestat_centre(bool on, double a, double mean) { return on ? a - mean : 0.0; }
// d = rank2 - (n + 1) from the number of active entries below a (`less`) and not above it (`upto`): rank2 = less + upto + 1
RK_SAMPLEMATH_FN int32_t edgestat_rank_dev(uint32_t less, uint32_t upto, uint32_t n) { return (int32_t)(less + upto) - (int32_t)n; }

// The chunk rule: a sum over the node ids is one partial per chunk of RK_KR_CHUNK ids, each from +0.0 in ascending id, and the
// partials are added in chunk order, the first one as it is (not onto +0.0: a partial of -0.0 or NaN stays what it is).
// chunk_fold is one step of it, for whoever meets the partials one by one; chunk_sum the whole of it over p(0 .. n_chunks - 1).
RK_SAMPLEMATH_FN double chunk_fold(bool first, double d, double p) { return first ? p : d + p; }

template <class P>
RK_SAMPLEMATH_FN double chunk_sum(uint32_t n_chunks, P &&p) {
    double d = chunk_fold(true, 0.0, p(0));
    for (uint32_t c = 1; c < n_chunks; c++) d = chunk_fold(false, d, p(c));
    return d;
}

}  // namespace rk
