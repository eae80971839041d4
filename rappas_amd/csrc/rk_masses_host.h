// rk_masses_host.h -- the host twin of masses_kernel (rk_kernels.hip) behind rk_masses_accumulate_host: the per-branch LWR sums
// of a result set, plain C++.  Header-only, like rk_translate_host.h.  Not part of the C ABI.
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

// reads [lo, hi) of a result set added into `m` (2 * B + 4 words: mass_q30[B] | best[B] | the four totals)
inline void masses_range(uint32_t B, uint32_t K, uint64_t lo, uint64_t hi, const uint8_t *n_rows, const uint16_t *branch, const double *lwr,
                         const uint32_t *weights, uint64_t *m) {
    uint64_t *mass = m, *best = m + B, *tot = m + 2 * (uint64_t)B;
    for (uint64_t r = lo; r < hi; r++) {
        const uint64_t w = weights ? weights[r] : 1u;
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
}

}  // namespace rk
