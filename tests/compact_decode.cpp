// The 32-bit compact-table lookup (rappas_amd/csrc/rk_compact32.h) swept over a block: for every position of a block of unit counts
// -- j = 0..23 in the nibble form, 0..11 in the byte form -- locate_*() must give the block and position the layout rule of
// rk_device.h defines, and decode_*() the row (first unit = block base + plain prefix sum of the counts before it, units = its own
// count).  Built and run by tests/test_compact_decode_host.py; no GPU, no HIP: the dot products take the header's plain-loop form.
//   compact_decode [SEED N]      sweep the pattern grid and N seeded random blocks per form; one line per kind of failure, exit 1
#include "rk_compact32.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace rk_compact32;

namespace {

unsigned long long checked = 0, failed = 0;

// a block of the table from its base and its counts, as the layout packs them
void pack_nib(uint32_t base, const uint32_t (&cnt)[24], uint32_t (&blk)[4]) {
    blk[0] = base, blk[1] = blk[2] = blk[3] = 0;
    for (uint32_t j = 0; j < 24; j++) blk[1 + (j >> 3)] |= cnt[j] << (4 * (j & 7));
}
void pack_byte(uint32_t base, const uint32_t (&cnt)[24], uint32_t (&blk)[4]) {  // (cnt[0..11])
    blk[0] = base, blk[1] = blk[2] = blk[3] = 0;
    for (uint32_t i = 0; i < 12; i++) blk[1 + (i >> 2)] |= cnt[i] << (8 * (i & 3));
}

void check_block(bool nib, uint32_t base, const uint32_t (&cnt)[24]) {
    uint32_t blk[4];
    if (nib) pack_nib(base, cnt, blk);
    else pack_byte(base, cnt, blk);
    uint32_t prefix = 0;
    for (uint32_t j = 0; j < (nib ? 24u : 12u); j++) {
        const Row r = nib ? decode_nib(blk[0], blk[1], blk[2], blk[3], j) : decode_byte(blk[0], blk[1], blk[2], blk[3], j);
        checked++;
        if (r.unit != base + prefix || r.n != cnt[j]) {
            if (!failed++)
                std::printf("%s form, position %u: got (prefix %u, n %u), want (%u, %u); block %08x %08x %08x\n", nib ? "nibble" : "byte", j,
                            r.unit - base, r.n, prefix, cnt[j], blk[1], blk[2], blk[3]);
        }
        prefix += cnt[j];
    }
}

void check_locate(uint32_t idx) {
    const Pos n = locate_nib(idx), b = locate_byte(idx);
    checked++;
    if (n.blk != idx / 24 || n.j != idx % 24 || b.blk != idx / 12 || b.j != idx % 12) {
        if (!failed++) std::printf("index %u: nibble form (%u, %u), byte form (%u, %u)\n", idx, n.blk, n.j, b.blk, b.j);
    }
}

void sweep_form(bool nib, uint32_t seed, long n_random) {
    const uint32_t top = nib ? 15u : 255u, len = nib ? 24u : 12u;
    uint32_t cnt[24];
    auto fill = [&](uint32_t v) { for (uint32_t &c : cnt) c = v; };
    fill(0), check_block(nib, 0u, cnt), check_block(nib, 0x01FFFFFFu, cnt);
    fill(top), check_block(nib, 1u, cnt);  // nibble form: prefix up to 23 x 15 = 345 > 255; byte form: 11 x 255
    if (!nib) fill(15), check_block(nib, 1u, cnt);
    for (uint32_t at = 0; at < len; at++)  // a single non-zero entry at each position, in its lowest, a middle and its highest value
        for (uint32_t v : {1u, top / 2 + 1, top}) {
            fill(0), cnt[at] = v;
            check_block(nib, 7u, cnt);
        }
    for (uint32_t at = 0; at < len; at++) {  // a single zero among full counts
        fill(top), cnt[at] = 0;
        check_block(nib, 7u, cnt);
    }
    for (uint32_t step : {1u, 3u, 7u, 11u})  // ramps up and down
        for (uint32_t from = 0; from <= top; from += (nib ? 1u : 17u)) {
            for (uint32_t j = 0; j < len; j++) cnt[j] = (from + j * step) % (top + 1);
            check_block(nib, 1000u, cnt);
            for (uint32_t j = 0; j < len; j++) cnt[j] = (from + (len - 1 - j) * step) % (top + 1);
            check_block(nib, 1000u, cnt);
        }
    std::mt19937 rng(seed + (nib ? 0u : 1u));
    for (long i = 0; i < n_random; i++) {
        const uint32_t sparse = rng() & 3u;  // a quarter of the blocks dense, the others with runs of absent k-mers
        for (uint32_t &c : cnt) c = (sparse && (rng() & 3u) < sparse) ? 0u : rng() & top;
        check_block(nib, rng() & 0x01FFFFFFu, cnt);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    const long n_random = argc > 2 ? std::strtol(argv[2], nullptr, 10) : 1000;
    sweep_form(true, seed, n_random);
    sweep_form(false, seed, n_random);
    // the index split: the first blocks, the values around 2^24 blocks (the 24-bit product of locate_nib), the top of the range
    for (uint32_t idx = 0; idx < 4096; idx++) check_locate(idx);
    for (uint32_t q : {(1u << 24) - 1, 1u << 24, (1u << 24) + 1, (1u << 26) + 5, (0x7FFFFFFFu / 24) - 1, 0x7FFFFFFFu / 24})
        for (uint32_t j = 0; j < 24; j++)
            if ((unsigned long long)q * 24 + j < (1ull << 31)) check_locate(q * 24 + j);
    std::mt19937 rng(seed ^ 0x5bd1e995u);
    for (long i = 0; i < 100 * n_random; i++) check_locate(rng() & 0x7FFFFFFFu);
    std::printf("%llu positions checked, %llu wrong\n", checked, failed);
    return failed ? 1 : 0;
}
