// rk_masses_samples_host.h -- the host twin of masses_samples_kernel (rk_kernels.hip) behind rk_masses_accumulate_samples_host: one
// mass buffer per sample from a membership list of (read, sample, weight) entries, plain C++.  Header-only, like
// rk_masses_host.h.  Not part of the C ABI.
//
// Written as the definition reads, entry by entry: an entry of sample s is one row of the result set gathered for s, so it adds
// what masses_range adds for one read, into the words of s.  The sums are integers: the order of the adds plays no part.
#pragma once
#include <cstdint>

#include "rk_masses_host.h"

namespace rk {

// Entries [lo, hi) of a membership list added into `m` (S * (2B + 4) + 1 words), those of the samples [s_lo, s_hi) alone.  An entry
// with sample >= S or read >= n_reads is never an index: with count_bad it is counted in the last word, and it adds nowhere else.
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
        if (s < s_lo || s >= s_hi) continue;
        // one row of the gathered set of sample s: what masses_range adds for a read, with the entry's weight
        const uint64_t w = member_weight ? member_weight[i] : 1u;
        uint64_t *mass = m + s * W, *best = mass + B, *tot = mass + 2 * (uint64_t)B;
        const uint32_t rows = n_rows[r] < K ? n_rows[r] : K;
        uint32_t counted = 0;
        for (uint32_t e = 0; e < rows; e++) {
            const uint32_t x = branch[r * K + e];
            if (x >= B) { tot[3]++; continue; }
            mass[x] += w * mass_q30(lwr[r * K + e]);
            if (e == 0) best[x] += w;
            counted++;
        }
        tot[0] += w;
        if (counted) tot[1] += w;
        tot[2] += w * counted;
    }
}

}  // namespace rk
