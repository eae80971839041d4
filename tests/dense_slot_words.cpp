// The slot words of the dense 24-entry row units (rappas_amd/csrc/rk_slots24.h) swept over their fields: for every unit of 24 slots
// the 16 lanes of a group must get exactly the slots the format in rk_device.h (ROW_UNIT24) defines -- lane li < 8: slot(li) and
// slot(16 + li); lane li >= 8: slot(li) and the scratch word.  Built and run by tests/test_dense_slot_words.py; no GPU, no HIP.
//   dense_slot_words [SEED N]      sweep the edge grid and N seeded random units; prints one line per kind of failure, exit 1
#include "rk_slots24.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace rk_slots24;

namespace {

unsigned long long checked = 0, failed = 0;

// slot[0..23] of one unit -> the second dword of each of the 16 lanes, as the format packs them; lanes 0..7 hold an increment
// there (any bit pattern: `noise`), which no lane may read a slot from
void pack(const uint32_t (&slot)[24], uint32_t noise, uint32_t (&w)[16]) {
    for (uint32_t j = 0; j < 8; j++) {
        w[j] = noise * (j + 1) + 0x9E3779B9u;
        w[8 + j] = slot[j] | slot[j + 8] << 10 | slot[16 + j] << 20;
    }
}

void check_unit(const uint32_t (&slot)[24], uint32_t noise) {
    uint32_t w[16];
    pack(slot, noise, w);
    for (uint32_t li = 0; li < 16; li++) {
        const uint32_t want_a = slot[li], want_b = li < 8 ? slot[16 + li] : 0u;
        const uint32_t r = masked_ror8(li, w[li], w[li ^ 8]);
        const Slots s = lane_slots(lane_shifts(li), r);  // the kernel's form: loop-invariant shifts, the DPP's result
        const Slots t = lane_slots(li, w[li], w[li ^ 8]);
        checked++;
        if (s.a != want_a || s.b != want_b || t.a != want_a || t.b != want_b) {
            if (!failed++)
                std::printf("lane %u: got (%u, %u) / (%u, %u), want (%u, %u); own word %08x, across %08x\n", li, s.a, s.b, t.a, t.b, want_a, want_b,
                            w[li], w[li ^ 8]);
        }
    }
}

}  // namespace

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    const long n_random = argc > 2 ? std::strtol(argv[2], nullptr, 10) : 100000;
    const uint32_t edge[6] = {0, 1, 511, 512, 1022, 1023};
    uint32_t slot[24];
    // every triple of edge values in the three fields of one word, in each of the eight words, the other words all zero / all ones
    for (uint32_t fill : {0u, SLOT_MASK})
        for (uint32_t j = 0; j < 8; j++)
            for (uint32_t a : edge)
                for (uint32_t b : edge)
                    for (uint32_t c : edge) {
                        for (uint32_t &s : slot) s = fill;
                        slot[j] = a, slot[j + 8] = b, slot[16 + j] = c;
                        check_unit(slot, a * 65599u + b * 257u + c);
                    }
    // the same triple in all eight words
    for (uint32_t a : edge)
        for (uint32_t b : edge)
            for (uint32_t c : edge) {
                for (uint32_t j = 0; j < 8; j++) slot[j] = a, slot[j + 8] = b, slot[16 + j] = c;
                check_unit(slot, 0xFFFFFFFFu);
            }
    // all-zero padding: every lane updates the scratch word twice
    for (uint32_t &s : slot) s = 0;
    check_unit(slot, 0u);
    {
        uint32_t w[16] = {0};
        for (uint32_t li = 0; li < 16; li++) {
            const Slots s = lane_slots(li, w[li], w[li ^ 8]);
            checked++;
            if ((s.a | s.b) && !failed++) std::printf("lane %u of an all-zero unit: (%u, %u)\n", li, s.a, s.b);
        }
    }
    std::mt19937 rng(seed);
    for (long i = 0; i < n_random; i++) {
        for (uint32_t &s : slot) s = rng() & SLOT_MASK;
        check_unit(slot, rng());
    }
    std::printf("%llu lanes checked, %llu wrong\n", checked, failed);
    return failed ? 1 : 0;
}
