// The chunk rule and the flag counters of the host path (rappas_amd/csrc/rk_chunks.h) checked against their definitions.  Whole batches
// are walked with next_chunk() and every chunking is held against the rule as it is stated: the chunks partition [0, n); a chunk keeps
// both limits unless it is a single read; it is maximal (the next read would break a limit); max_len is its longest read.  count_flags()
// is held against a per-bit recount, add() against the sum of two such recounts.  Built and run by tests/test_chunks_host.py; no GPU,
// no HIP.
//   chunks [SEED N]      the planted shapes and N seeded ragged batches; one line per kind of failure, exit 1
#include "rk_chunks.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

unsigned long long checked = 0, failed = 0;
constexpr uint64_t MAX_READS = 8, MAX_BYTES = 64;

void wrong(const char *what, uint64_t n, uint64_t from, uint64_t r1) {
    if (!failed++) std::printf("batch of %llu reads, chunk [%llu, %llu): %s\n", (unsigned long long)n, (unsigned long long)from, (unsigned long long)r1, what);
}

// lens: the reads' lengths, or null for packed input (no offsets)
void check_batch(const std::vector<uint64_t> *lens, uint64_t n) {
    std::vector<uint64_t> off(n + 1, 0);
    if (lens)
        for (uint64_t r = 0; r < n; r++) off[r + 1] = off[r] + (*lens)[r];
    const uint64_t *seq_off = lens ? off.data() : nullptr;
    uint64_t from = 0, chunks = 0;
    while (from < n) {
        const rk::Chunk c = rk::next_chunk(seq_off, from, n, MAX_READS, MAX_BYTES);
        checked++;
        chunks++;
        if (c.r1 <= from || c.r1 > n) { wrong("not a step forward inside the batch", n, from, c.r1); return; }  // (the partition: each chunk starts where the last ended)
        const uint64_t reads = c.r1 - from, bytes = lens ? off[c.r1] - off[from] : 0;
        if (reads > MAX_READS) wrong("more reads than the limit", n, from, c.r1);
        if (bytes > MAX_BYTES && reads != 1) wrong("more bytes than the limit in a chunk of several reads", n, from, c.r1);
        if (c.r1 < n && reads < MAX_READS && (!lens || off[c.r1 + 1] - off[from] <= MAX_BYTES)) wrong("not maximal: the next read fits", n, from, c.r1);
        uint64_t longest = 0;
        if (lens)
            for (uint64_t r = from; r < c.r1; r++) longest = (*lens)[r] > longest ? (*lens)[r] : longest;
        if (c.max_len != longest) wrong("max_len is not the longest read", n, from, c.r1);
        from = c.r1;
    }
    if (n == 0) {  // nothing to cut: the rule gives an empty chunk and the pipeline never asks
        const rk::Chunk c = rk::next_chunk(seq_off, 0, 0, MAX_READS, MAX_BYTES);
        checked++;
        if (c.r1 != 0 || c.max_len != 0) wrong("an empty batch must give an empty chunk", 0, 0, c.r1);
    }
    if (!lens && chunks != (n + MAX_READS - 1) / MAX_READS) wrong("packed input: chunks of the read limit only", n, 0, n);
}

void planted_batches() {
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, MAX_READS - 1, MAX_READS, MAX_READS + 1, 3 * MAX_READS + 7}) {
        check_batch(nullptr, n);  // no offsets
        for (uint64_t len : {(uint64_t)0, (uint64_t)1, (uint64_t)3, MAX_BYTES / MAX_READS, MAX_BYTES / MAX_READS + 1}) {  // all-empty reads; 8 x 8 = the byte limit exactly
            const std::vector<uint64_t> lens(n, len);
            check_batch(&lens, n);
        }
        // a read of exactly the byte limit, and one byte more, at the start, in the middle and at the end
        for (uint64_t big : {MAX_BYTES, MAX_BYTES + 1})
            for (uint64_t other : {(uint64_t)0, (uint64_t)2})
                for (uint64_t at : {(uint64_t)0, n / 2, n ? n - 1 : 0}) {
                    if (!n) continue;
                    std::vector<uint64_t> lens(n, other);
                    lens[at] = big;
                    check_batch(&lens, n);
                }
    }
    // runs whose bytes hit the limit exactly: 4 x 16, then 2 x 32, then 1 x 64, then 63 + 1, then 63 + 2 (one byte over)
    const std::vector<uint64_t> exact = {16, 16, 16, 16, 32, 32, 64, 63, 1, 63, 2, 0, 0, 64, 0};
    check_batch(&exact, exact.size());
}

void ragged_batches(uint32_t seed, long n_batches) {
    std::mt19937 rng(seed);
    for (long b = 0; b < n_batches; b++) {
        const uint64_t n = rng() % (5 * MAX_READS), top = 1 + rng() % (2 * MAX_BYTES);  // mostly short reads, mostly long ones, or a mix
        std::vector<uint64_t> lens(n);
        for (uint64_t &l : lens) l = (rng() & 3u) ? rng() % top : rng() % 4;
        check_batch(&lens, n);
    }
}

// the five low flag bits in every combination -- four are counted, BELOW_NSBOUND must change nothing -- under bits nobody reads
void check_counters(uint32_t seed) {
    const uint32_t read_bits[4] = {RK_FLAG_PLACED, RK_FLAG_BAD_CHAR, RK_FLAG_TOO_SHORT, RK_FLAG_AMBIGUOUS};
    const uint32_t ignored = RK_FLAG_BELOW_NSBOUND | RK_FLAG_REVERSE | RK_FLAG_TOO_LONG | 0xFFFFFF80u;
    std::mt19937 rng(seed);
    std::vector<uint32_t> flags;
    for (uint32_t combo = 0; combo < 32; combo++)
        for (uint32_t rep = 0; rep <= combo % 3; rep++) flags.push_back((combo & 15u) | ((combo & 16u) ? RK_FLAG_BELOW_NSBOUND : 0u) | (rep ? rng() & ignored : 0u));
    auto recount = [&](size_t lo, size_t hi) {
        rk_counters c{};
        uint64_t per_bit[4] = {0, 0, 0, 0};
        for (size_t i = lo; i < hi; i++)
            for (int b = 0; b < 4; b++) per_bit[b] += (flags[i] & read_bits[b]) != 0;
        c.reads = hi - lo; c.placed = per_bit[0]; c.unplaced = c.reads - per_bit[0];
        c.bad_char = per_bit[1]; c.too_short = per_bit[2]; c.ambiguous = per_bit[3];
        return c;
    };
    auto same = [](const rk_counters &a, const rk_counters &b) {
        return a.reads == b.reads && a.placed == b.placed && a.unplaced == b.unplaced && a.bad_char == b.bad_char && a.too_short == b.too_short && a.ambiguous == b.ambiguous;
    };
    for (size_t cut = 0; cut <= flags.size(); cut++) {  // two chunks of every split, counted into one set and added from two
        rk_counters one{}, lo{}, hi{};
        rk::count_flags(flags.data(), cut, one);
        rk::count_flags(flags.data() + cut, flags.size() - cut, one);
        rk::count_flags(flags.data(), cut, lo);
        rk::count_flags(flags.data() + cut, flags.size() - cut, hi);
        checked += 2;
        if (!same(one, recount(0, flags.size())) || !same(lo, recount(0, cut)) || !same(hi, recount(cut, flags.size())))
            if (!failed++) std::printf("count_flags differs from the per-bit recount at split %zu\n", cut);
        rk::add(lo, hi);
        if (!same(lo, one))
            if (!failed++) std::printf("add differs from counting into one set at split %zu\n", cut);
    }
}

}  // namespace

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    const long n_batches = argc > 2 ? std::strtol(argv[2], nullptr, 10) : 300;
    planted_batches();
    ragged_batches(seed, n_batches);
    check_counters(seed);
    std::printf("%llu chunks and counts checked, %llu wrong\n", checked, failed);
    return failed ? 1 : 0;
}
