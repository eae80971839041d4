// rk_chunks.h -- the pure rules of the host path (rk_hostpath_impl.h): how a batch is cut into chunks, and how a chunk's flags become
// the counters of the call.  Integer arithmetic without HIP: the pipeline cuts every batch with it, and tests/chunks.cpp walks whole
// batches with it on any machine.  Not part of the C ABI.
#pragma once
#include <cstdint>

#include "../../include/rappas_place.h"  // rk_counters, RK_FLAG_*

namespace rk {

// Chunks of 2^18 reads: the kernel still fills the chip (2^16 tiles for 2 048 waves) and the part of a call that nothing overlaps --
// the first chunk's upload, the last chunk's download and drain -- stays short.  128 MiB of characters bound the staging of long reads.
constexpr uint64_t CHUNK_MAX_READS = 1ull << 18, CHUNK_MAX_BYTES = 128ull << 20;
constexpr uint64_t CHUNK_MIN_READS_KNOB = 1024;  // the smallest value the developer knob RK_CHUNK_READS may set

struct Chunk {
    uint64_t r1;       // the chunk is the reads [from, r1)
    uint64_t max_len;  // its longest read in characters (0 without offsets)
};

// The longest run of reads from `from` with at most max_reads reads whose characters span at most max_bytes; a single read larger
// than max_bytes is still a chunk of its own.  seq_off == nullptr (packed input): only the read limit applies.
inline Chunk next_chunk(const uint64_t *seq_off, uint64_t from, uint64_t n_reads, uint64_t max_reads, uint64_t max_bytes) {
    if (!seq_off) return Chunk{from + max_reads < n_reads ? from + max_reads : n_reads, 0};
    Chunk c{from, 0};
    while (c.r1 < n_reads && c.r1 - from < max_reads && (seq_off[c.r1 + 1] - seq_off[from] <= max_bytes || c.r1 == from)) {
        const uint64_t len = seq_off[c.r1 + 1] - seq_off[c.r1];
        if (len > c.max_len) c.max_len = len;
        c.r1++;
    }
    return c;
}

// per-batch counters, taken chunk by chunk while the flags are cache-hot
inline void count_flags(const uint32_t *flags, uint64_t n, rk_counters &ct) {
    for (uint64_t r = 0; r < n; r++) {
        const uint32_t f = flags[r];
        ct.reads++;
        if (f & RK_FLAG_PLACED) ct.placed++; else ct.unplaced++;
        if (f & RK_FLAG_BAD_CHAR) ct.bad_char++;
        if (f & RK_FLAG_TOO_SHORT) ct.too_short++;
        if (f & RK_FLAG_AMBIGUOUS) ct.ambiguous++;
    }
}

inline void add(rk_counters &to, const rk_counters &c) {
    to.reads += c.reads; to.placed += c.placed; to.unplaced += c.unplaced;
    to.bad_char += c.bad_char; to.too_short += c.too_short; to.ambiguous += c.ambiguous;
}

}  // namespace rk
