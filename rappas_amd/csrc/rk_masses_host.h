// rk_masses_host.h -- the host twins of masses_kernel and masses_samples_kernel (rk_masses.h) behind rk_masses_accumulate_host and
// rk_masses_accumulate_samples_host: the per-branch LWR sums of a result set, whole or per sample from a membership list, plain C++
// (DESIGN.md 4.7).  Header-only, like rk_translate_host.h.  Not part of the C ABI.
//
// Written as the definition reads, read by read and row by row.  The sums are integers (an LWR enters as its 30-bit fixed-point
// value), so the order of the adds -- threads here, atomics on the device -- plays no part in the result.  The reference has no
// counterpart: it writes one jplace record per read and leaves the per-edge table to the tools behind it.
#pragma once
#include <cmath>
#include <cstdint>

namespace rk {

// q(l): an LWR as an integer of 2^-30 -- llrint(min(l, 1) * 2^30) for l >= 0 (ties to even, the product is exact in binary64),
// 0 for negatives and NaN.  At most 2^30, so one weighted add stays below 2^62.
inline uint32_t mass_q30(double l) { return l >= 0.0 ? (uint32_t)std::llrint(std::fmin(l, 1.0) * 1073741824.0) : 0u; }

// read r of a result set, with weight w, added into `m` (2 * B + 4 words: mass_q30[B] | best[B] | the four totals)
inline void masses_add_read(uint32_t B, uint32_t K, uint64_t r, uint64_t w, const uint8_t *n_rows, const uint16_t *branch, const double *lwr, uint64_t *m) {
    uint64_t *mass = m, *best = m + B, *tot = m + 2 * (uint64_t)B;
    const uint32_t rows = n_rows[r] < K ? n_rows[r] : K;
    uint32_t counted = 0;
    for (uint32_t e = 0; e < rows; e++) {
        const uint32_t x = branch[r * K + e];
        if (x >= B) { tot[3]++; continue; }  // never an index: skipped and counted
        mass[x] += w * mass_q30(lwr[r * K + e]);
        if (e == 0) best[x] += w;
        counted++;
    }
    tot[0] += w;
    if (counted) tot[1] += w;
    tot[2] += w * counted;
}

// reads [lo, hi) of a result set added into `m`
inline void masses_range(uint32_t B, uint32_t K, uint64_t lo, uint64_t hi, const uint8_t *n_rows, const uint16_t *branch, const double *lwr,
                         const uint32_t *weights, uint64_t *m) {
    for (uint64_t r = lo; r < hi; r++) masses_add_read(B, K, r, weights ? weights[r] : 1u, n_rows, branch, lwr, m);
}

// Entries [lo, hi) of a membership list added into `m` (S * (2B + 4) + 1 words), those of the samples [s_lo, s_hi) alone: an entry of
// sample s is one read of the result set gathered for s, added into the words of s.  An entry with sample >= S or read >= n_reads is
// never an index: with count_bad it is counted in the last word, and it adds nowhere else.
// member_read == nullptr: entry i is read i.  member_weight == nullptr: 1.
inline void masses_samples_range(uint32_t B, uint32_t K, uint32_t S, uint64_t n_reads, const uint8_t *n_rows, const uint16_t *branch, const double *lwr,
                                 uint64_t lo, uint64_t hi, const uint32_t *member_read, const uint32_t *member_sample, const uint32_t *member_weight,
                                 uint32_t s_lo, uint32_t s_hi, bool count_bad, uint64_t *m) {
    const uint64_t W = 2 * (uint64_t)B + 4;
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t r = member_read ? member_read[i] : i;
        const uint32_t s = member_sample[i];
        if (s >= S || r >= n_reads) {
            if (count_bad) m[S * W]++;
            continue;
        }
        if (s >= s_lo && s < s_hi) masses_add_read(B, K, r, member_weight ? member_weight[i] : 1u, n_rows, branch, lwr, m + s * W);
    }
}

}  // namespace rk
