// rk_compact32.h -- the compact direct table (rk_device.h, COMPACT_KMERS) looked up in 32-bit arithmetic: from the dense index of a
// k-mer to the 16-byte block to gather and the k-mer's position in it, and from the gathered block to the row -- its first 128-byte
// unit and its number of units.  Pure integer arithmetic without HIP: place_packed16_kernel (rk_kernels.hip) probes with it on the
// device, and tests/compact_decode.cpp sweeps it on any machine.
//
// The two forms of a block {x, y, z, w} (x = first unit of the block's first row; rows of a block are consecutive in the blob):
//   byte form    12 k-mers a block, y z w = 12 x u8 units per row, little-endian: k-mer i of the block in byte i & 3 of word i >> 2;
//   nibble form  24 k-mers a block (no row of the database exceeds 15 units), y z w = 24 x u4: k-mer j in nibble j & 7 of word j >> 3.
// Row of k-mer j: unit = x + (sum of the counts before j), n = count j; n == 0 <=> the k-mer is absent.
//
// Everything is cut out of idx once: q = idx / 24 and j = idx - 24 q serve both forms (the byte form's block is 2 q or 2 q + 1).
// The prefix sums are dot products with a vector of ones -- v_dot8_u32_u4 over nibbles, v_sad_u8 over bytes -- masked below j; a block's
// prefix can exceed 255 (24 x 15 = 360), the accumulator is a full word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RK_COMPACT32_HD __host__ __device__ inline
#else
#define RK_COMPACT32_HD inline
#endif

namespace rk_compact32 {

constexpr uint32_t NIB_KMERS = 24, BYTE_KMERS = 12, NIB_ONES = 0x11111111u;

struct Pos {  // where a k-mer's count sits
    uint32_t blk, j;  // 16-byte block of the table; position in the block (nibble form 0..23, byte form 0..11)
};
struct Row {
    uint32_t unit, n;  // first 128-byte unit of the row; units of the row, 0 = absent
};

// acc + sum of the eight nibbles of w under the 0/1 nibble mask `ones`
RK_COMPACT32_HD uint32_t nib_sum(uint32_t w, uint32_t ones, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot8(w, ones, acc, false);
#else
    for (int i = 0; i < 8; i++) acc += ((w >> (4 * i)) & 15u) * ((ones >> (4 * i)) & 15u);
    return acc;
#endif
}
// acc + sum of the four bytes of w
RK_COMPACT32_HD uint32_t byte_sum(uint32_t w, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(w, 0u, acc);
#else
    for (int i = 0; i < 4; i++) acc += (w >> (8 * i)) & 0xFFu;
    return acc;
#endif
}
// bits [at, at + width) of w, at + width <= 32 (v_bfe_u32)
RK_COMPACT32_HD uint32_t field(uint32_t w, uint32_t at, uint32_t width) { return (w >> at) & ((1u << width) - 1u); }

// idx < 2^31.  j = idx - 24 q lies in 0..23, so five bits of it are all of it: the product may drop q's bits above 24 (they change it
// by a multiple of 2^24 * 24) and is one v_mul_u32_u24
RK_COMPACT32_HD Pos locate_nib(uint32_t idx) {
    const uint32_t q = idx / NIB_KMERS;
    return Pos{q, (idx - (q & 0xFFFFFFu) * NIB_KMERS) & 31u};
}
RK_COMPACT32_HD Pos locate_byte(uint32_t idx) {
    const Pos p = locate_nib(idx);
    const uint32_t odd = p.j >= BYTE_KMERS ? 1u : 0u;
    return Pos{2u * p.blk + odd, p.j - odd * BYTE_KMERS};
}

RK_COMPACT32_HD Row decode_nib(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t j) {
    const uint32_t c0 = nib_sum(y, NIB_ONES, 0u);
    const uint32_t c1 = nib_sum(z, NIB_ONES, c0);
    const uint32_t word = j >> 3, sh = (j & 7u) * 4u;
    const uint32_t wsel = word == 0 ? y : (word == 1 ? z : w);
    const uint32_t csel = word == 0 ? 0u : (word == 1 ? c0 : c1);
    const uint32_t prefix = nib_sum(wsel, NIB_ONES & ((1u << sh) - 1u), csel);
    return Row{x + prefix, field(wsel, sh, 4)};
}
RK_COMPACT32_HD Row decode_byte(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t i) {
    const uint32_t c0 = byte_sum(y, 0u);
    const uint32_t c1 = byte_sum(z, c0);
    const uint32_t word = i >> 2, sh = (i & 3u) * 8u;
    const uint32_t wsel = word == 0 ? y : (word == 1 ? z : w);
    const uint32_t csel = word == 0 ? 0u : (word == 1 ? c0 : c1);
    const uint32_t prefix = byte_sum(wsel & ((1u << sh) - 1u), csel);
    return Row{x + prefix, field(wsel, sh, 8)};
}

}  // namespace rk_compact32
