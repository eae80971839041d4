// rk_translate_host.h -- the host twin of translate_frame_kernel (rk_kernels.hip) behind rk_translate_packed_host: one reading
// frame of 2-bit DNA records -> 5-bit amino-acid records, plain C++.  Header-only, so that every build that compiles
// rk_engine.hip next to rk_pack_host.cpp -- the library's, the developer variants' under scripts/ -- links as before.  Not part of the C ABI.
//
// Written as the definition reads, base by base: frame f < 3 starts at base f of the read as given, frame 3 + o at base o of its
// reverse complement (base i of that = base R-1-i of the read, state ^ 1); codons go through the standard code; the record of a frame
// is its longest stop-free run of residues, the first of equal ones.  The reference has no counterpart (it places a read as given);
// the states are DNAStatesShifted.java:182-209 and AAStates.java:48-197.
#pragma once
#include "rk_translate.h"

namespace rk {

namespace translate_host {
constexpr unsigned char kCodon[64] = RK_CODON_TABLE;

inline uint32_t base_at(const uint32_t *rec, uint32_t i) { return (rec[i >> 4] >> (2u * (i & 15u))) & 3u; }
}  // namespace translate_host

// frame `frame` (0..5) of reads [lo, hi): the longest stop-free run of residues of each, packed at 5 bits from bit 0 into
// aa[r * aa_words ..] (zero beyond the run), its length into aa_lens[r]: word for word what translate_frame_kernel writes.
inline void translate_range(uint32_t frame, const uint32_t *dna, uint32_t dna_words, const uint32_t *dna_lens, uint32_t fixed_len, uint64_t lo, uint64_t hi,
                            uint32_t *aa, uint32_t aa_words, uint32_t *aa_lens) {
    const bool rev = frame >= 3;
    const uint32_t o = rev ? frame - 3 : frame, cap = dna_words * 16u;
    for (uint64_t r = lo; r < hi; r++) {
        const uint32_t *rec = dna + r * dna_words;
        uint32_t R = dna_lens ? dna_lens[r] : fixed_len;
        if (R > cap) R = cap;  // never read past the record
        const uint32_t n_codons = R >= o + 3 ? (R - o) / 3 : 0;
        auto residue = [&](uint32_t j) -> uint32_t {
            uint32_t b[3];
            for (uint32_t t = 0; t < 3; t++) {
                const uint32_t i = o + 3 * j + t;  // base of the frame's strand
                b[t] = rev ? translate_host::base_at(rec, R - 1 - i) ^ 1u : translate_host::base_at(rec, i);
            }
            return translate_host::kCodon[b[0] | b[1] << 2 | b[2] << 4];
        };
        uint32_t best_s = 0, best_l = 0, cur_s = 0;
        for (uint32_t j = 0; j <= n_codons; j++) {
            if (j == n_codons || residue(j) == RK_CODON_STOP) {
                if (j - cur_s > best_l) { best_l = j - cur_s; best_s = cur_s; }
                cur_s = j + 1;
            }
        }
        uint32_t *out = aa + r * aa_words;
        for (uint32_t w = 0; w < aa_words; w++) out[w] = 0;
        for (uint32_t i = 0; i < best_l; i++) {
            const uint32_t st = residue(best_s + i), bit = 5 * i, w = bit >> 5, sh = bit & 31u;
            if (w < aa_words) out[w] |= st << sh;
            if (sh > 27 && w + 1 < aa_words) out[w + 1] |= st >> (32 - sh);
        }
        aa_lens[r] = best_l;
    }
}

}  // namespace rk
