// rk_slots24.h -- the slot words of the dense 24-entry row units (rk_device.h, ROW_UNIT24): which two score-vector words a lane of a
// 16-lane group updates in one accumulate step.  Pure integer arithmetic without HIP: accumulate_units (rk_kernels.hip) unpacks with
// it on the device, and tests/dense_slot_words.cpp sweeps it on any machine.
//
// The format: lane 8 + j (j = 0..7) of the group loads the word  slot(j) | slot(j + 8) << 10 | slot(16 + j) << 20,  bits 30..31 zero;
// lanes 0..7 load an increment there instead.  Lane li applies entry li, and lanes 0..7 entry 16 + li as well; the second update of
// lanes 8..15 goes to the scratch word (slot 0).  All-zero padding gives slot 0 everywhere.
//
// The step: one masked DPP, v_mov_b32_dpp row_ror:8 bank_mask:0x3 with the lane's own word as `old`, leaves r = the word of lane
// li + 8 in lanes 0..7 and the lane's own word in lanes 8..15 -- a slot word in every lane.  Each lane then cuts two ten-bit fields out
// of r at offsets that depend on the lane alone (loop-invariant): 0 and 20 in lanes 0..7, 10 and 30 in lanes 8..15.  A field at bit 30
// reads the two zero bits of the format and nothing beyond the word, so it IS the scratch slot: no select on the lane number.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RK_SLOTS24_HD __host__ __device__ inline
#else
#define RK_SLOTS24_HD inline
#endif

namespace rk_slots24 {

constexpr uint32_t SLOT_BITS = 10, SLOT_MASK = (1u << SLOT_BITS) - 1;

struct Shifts {  // where the lane's two fields sit in r
    uint32_t a, b;
};
struct Slots {  // word indices in the score vector: a = the slot of entry li; b = the slot of entry 16 + li, or 0 (scratch)
    uint32_t a, b;
};

RK_SLOTS24_HD Shifts lane_shifts(uint32_t li) {  // li = lane within its 16-lane group
    const uint32_t hi = li < 8 ? 0u : SLOT_BITS;
    return Shifts{hi, 2 * SLOT_BITS + hi};
}

// What the masked DPP leaves in lane li: `own` = the lane's second dword of the unit, `across` = that of lane li ^ 8.  (The kernel has
// the instruction; the host test models it with this.)
RK_SLOTS24_HD uint32_t masked_ror8(uint32_t li, uint32_t own, uint32_t across) { return li < 8 ? across : own; }

// ten bits of w from bit `at` (at <= 31; bits beyond the word read as zero): v_bfe_u32 on the device
RK_SLOTS24_HD uint32_t field(uint32_t w, uint32_t at) { return (w >> at) & SLOT_MASK; }

RK_SLOTS24_HD Slots lane_slots(Shifts sh, uint32_t r) { return Slots{field(r, sh.a), field(r, sh.b)}; }

// the whole step of one lane from its own word and the word a plain row_ror:8 brings (that of lane li ^ 8)
RK_SLOTS24_HD Slots lane_slots(uint32_t li, uint32_t own, uint32_t across) { return lane_slots(lane_shifts(li), masked_ror8(li, own, across)); }

}  // namespace rk_slots24
