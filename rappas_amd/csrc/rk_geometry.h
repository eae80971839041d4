// rk_geometry.h -- launch geometry of the placement kernels: how much LDS a block gets, how it is cut up, how many blocks a CU is asked to
// hold and how many go out; and which image a database gets (windows, the large-tree index).  Pure host arithmetic without HIP and without
// getenv: rk_engine.hip launches and names its kernels (rk_kernel_name) with it, and tests/geometry_grid.cpp sweeps it on any machine.
// A function that can refuse returns a Status; the engine turns it into the error code and text of the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include "rk_plan.h"  // RK_WSTREAM_MAX_UNITS

#ifndef RK_WG_MIN_BRANCHES
#define RK_WG_MIN_BRANCHES 8192u  // above this a single-wave score vector leaves <= 4 waves per CU: use place_wg_kernel
#endif
#ifndef RK_WG_MIN_MEAN_ROW
#define RK_WG_MIN_MEAN_ROW 320.0    // ... for rows at least this long on average (scripts/long_rows_big_tree.py: up to ~300 entries the windowed kernel is ahead:
                                    // 15 999 branches, mean row 70 / 150 / 300: 54 / 36 / 19 against 22 / 19 / 17 Mreads/s) ...
#endif
#ifndef RK_WG_ALWAYS_BRANCHES
#define RK_WG_ALWAYS_BRANCHES 65535u  // ... or, whatever the rows, above this many branches (none: the windowed kernel's 64 windows of 1 024 cover every tree)
#endif
#ifndef RK_WINDOW_MIN_BRANCHES
#define RK_WINDOW_MIN_BRANCHES 1276u  // the dense 16-lane geometry keeps eight waves per CU up to 1 116 branches and seven up to 1 276; the switch sits where the seventh wave goes (round 3, scripts/tree_size_sweep.py, dense against windowed Mreads/s: 1 117 branches 291 / 247, 1 200: 257 / ~245, 1 290 (six waves): 219 / 242, 1 400: 218 / 242, 2 800: 110 / 188)
#endif
#ifndef RK_RING
#define RK_RING 8  // depth of the row-chunk register ring (chunks in flight per lane)
#endif
#ifndef RK_RING64
#define RK_RING64 8  // ... and for the 64-lane geometry (one wave per read: large trees with long rows, one or two waves per SIMD)
#endif
#ifndef RK_RING_DENSE
#define RK_RING_DENSE 12  // ... and of the dense 24-entry instances of place_packed16_kernel (even, 8 .. 16: a block's items are the 16 lanes of one register; 14 and 16 spill, DESIGN.md 5 "Round 11")
#endif

namespace rk_geom {

// what a geometry can refuse: keep_at_most beyond the lanes of a read's group; one read's score vector and list beyond a CU's LDS
// (Geometry::lds_per_wave); no branch-range pass of the workgroup kernel, or not one wave of a windowed kernel, fits a CU; the ambiguity
// kernel without a score vector
enum Status { GEOM_OK = 0, KEEP_NEEDS_LANES, READ_EXCEEDS_LDS, NO_WG_WINDOW, WINDOWED_NO_FIT, NO_SCORE_VECTOR };
// the developer knobs (RK_*) the geometry reads, as the engine found them (the defaults in the product library)
struct Knobs {
    uint32_t list_cap = 0, waves_per_cu = 0;             // RK_LIST_CAP, RK_WAVES_PER_CU (0: none)
    int wg_passes = 1;                                   // RK_WG_PASSES
    uint32_t hash_waves = ~0u;                           // RK_HASH_WAVES
    bool window_always = false, wstream_always = false;  // RK_WINDOW_ALWAYS, RK_WSTREAM_ALWAYS
};
constexpr uint32_t ROW_ENTRIES = 16;        // entries per 128-byte row unit (rk_device.h: ROW_UNIT)

// ---- persistent grids: one block per slot a CU really has ----
// Blocks a CU holds: the fewer of what the launch asks for (by LDS size) and what the runtime's occupancy query says.  And
// the LDS is handed out in granules of 512 bytes, which the occupancy query does not count in: 23 232 B per block -- seven by
// division and by the query -- are 23 552 B each, and six are resident (round 3, scripts/tree_size_sweep.py at 1 290 branches:
// the seventh block of every CU ran in a second round, 140 instead of 250 Mreads/s).
static inline uint64_t resident_per_cu(uint64_t by_lds, uint64_t by_query, size_t lds) {
    uint64_t out = by_lds < by_query ? by_lds : by_query;
    if (lds) {
        const uint64_t by_granule = (160ull * 1024) / ((lds + 511) & ~(size_t)511);
        if (by_granule >= 1 && by_granule < out) out = by_granule;
    }
    return out;
}
static inline uint64_t grid_blocks(int cu_count, uint64_t per_cu, uint64_t work) { return (uint64_t)cu_count * per_cu > work ? work : (uint64_t)cu_count * per_cu; }

// ---- dense kernels: one lane group per read, the whole score vector in the LDS ----
struct Geometry { uint32_t G, NG, s_stride, list_cap, pu; size_t lds_per_wave; uint32_t waves_per_cu; };
// PU*G >= 144 positions per probe batch.  Amino acids through the 16-lane kernels: a packed record of <= 16 words holds <= 102
// residues, so seven rounds of sixteen are a whole read (nine made C4 look up 48 k-mers per read that do not exist)
static constexpr uint32_t probe_unroll(uint32_t G, uint32_t bits) { return G <= 16 ? (bits == 5 && G == 16 ? 7 : 9) : (G == 32 ? 5 : 3); }
static inline Status choose_geometry(uint32_t nb, uint32_t bits, size_t lds_per_cu, uint32_t lanes_per_read, uint32_t keep_at_most, const Knobs &kn, Geometry &g) {
    const uint32_t s_stride = (nb + 4) & ~3u;  // >= nb + 1 (word nb is the scratch slot of apply_entry), multiple of 4 (b128 scans)
    const size_t target = lds_per_cu / 8;  // aim for >= 8 waves per CU
    const size_t fixed = (size_t)s_stride * 4;  // per read, besides the hit list
    auto bytes_for = [&](uint32_t G, uint32_t cap) { return (size_t)(64 / G) * (fixed + (size_t)cap * 8); };
    uint32_t G = lanes_per_read;
    if (G == 0) {
        // Throughput follows the reads in flight per CU (LDS capacity / score-vector size) and, at equal reads in flight, prefers
        // narrower groups as long as enough waves remain to hide latency.  Measured on C2-like DBs (scripts/tree_size_sweep.py):
        // 999 branches: 16 lanes (8 waves) 335 Mreads/s; 1300 / 1500: 16 lanes (6 waves) 219 / 214 vs 32 lanes (11 / 10 waves) 156 / 141;
        // 1999: 32 lanes (8 waves) 199 vs 16 lanes (4 waves) 165 vs 64 lanes 120; 3999: 32 lanes (4 waves) 88 vs 64 lanes (9 waves) 62;
        // 7999: 64 lanes (4 waves) 46 vs 32 lanes (2 waves) 35.  (Between 1 117 and 16 000 branches these dense geometries only serve
        // what the windowed kernel does not take: records of more than 16 words, a forced lane width.)
        G = 64;
        if (keep_at_most <= 16 && bytes_for(16, 16 + 3 * RK_RING + 40) <= lds_per_cu / 6) G = 16;
        else if (keep_at_most <= 32 && bytes_for(32, 32 + 3 * RK_RING + 40) <= lds_per_cu / 4) G = 32;
    }
    if (G < keep_at_most) return KEEP_NEEDS_LANES;
    const uint32_t NG = 64 / G, pu = probe_unroll(G, bits);
    const uint32_t min_cap = G + 3 * (G == 64 ? RK_RING64 : RK_RING) + 40;  // one sub-batch of rows + sentinel, ring slack, 16 winner slots + margin
    // list capacity: whatever is left of the per-wave LDS target, clamped to [min_cap, 256]
    size_t per_group_target = target / NG;
    uint32_t cap = min_cap;
    if (per_group_target > fixed + (size_t)min_cap * 8) {
        size_t c = (per_group_target - fixed) / 8;
        cap = (uint32_t)(c > 256 ? 256 : c);
        if (cap < min_cap) cap = min_cap;
    }
    if (kn.list_cap >= min_cap && kn.list_cap <= 4096) cap = kn.list_cap;  // developer knob: trade hit-list room for occupancy
    cap &= ~1u;  // keeps every group's score vector 16-byte aligned
    g.G = G; g.NG = NG; g.s_stride = s_stride; g.list_cap = cap; g.pu = pu;
    g.lds_per_wave = bytes_for(G, cap);
    if (g.lds_per_wave > lds_per_cu) return READ_EXCEEDS_LDS;
    uint32_t w = (uint32_t)(lds_per_cu / g.lds_per_wave);
    g.waves_per_cu = w > 32 ? 32 : w;
    if (kn.waves_per_cu >= 1 && kn.waves_per_cu < g.waves_per_cu) g.waves_per_cu = kn.waves_per_cu;  // developer knob for occupancy experiments
    return GEOM_OK;
}
// The dense 24-entry instances of place_packed16_kernel (ring of U = RK_RING_DENSE row units, a block's U items in the lanes of one
// register): the flush of a tile writes fillers behind the longest list as far as the step loop reads items -- two turns of the ring,
// or the end of the 16-item read of the last whole block, U + 16 -- and a read's list takes items up to what that leaves of its
// 2 * list_cap words (less one pair).  min_cap above leaves at least 126: more than the 2U an early start asks for.
static constexpr uint32_t dense_list_fillers(uint32_t U) { return U + 16 > 2 * U ? U + 16 : 2 * U; }
static constexpr uint32_t dense_cap_items(uint32_t list_cap, uint32_t U) { return 2 * list_cap - dense_list_fillers(U) - 2; }

// ---- windowed images and their kernels ----
// mid-size trees: the score vector of a read is held one window of W branches at a time (place_packed16w_kernel)
constexpr uint32_t RK_MAX_WINDOWS = 64;  // 6-bit window ids in winspec and in the item tags
// winspec byte of a row that reaches the windows first .. last: first | span << 6, span 3 = "at least three more: to the last window"
static inline unsigned char winspec_byte(uint32_t first, uint32_t last) {
    const uint32_t span = last - first;
    return (unsigned char)(first | ((span < 3u ? span : 3u) << 6));
}
constexpr uint64_t RK_WINDOW_MAX_BLOB = 1ull << 31;  // list items carry a 24-bit index of 128-byte units
// The windowed kernel holds a read's row units in a list of a few hundred items: beyond ~2.2 units per k-mer code (a 150-bp read
// then brings ~300) a read is emitted in many window ranges and the dense kernels are ahead (scripts/row_length_sweep.py, 3 999
// branches, mean row 100 / 250 entries: 113 / 35 against 87 / 49 Mreads/s) -- unless the tree is so large that they hold one read
// in two or three waves per CU (beyond 8 192 branches; scripts/dense_rows_mid_tree.py, every k-mer present with rows of 30 / 60
// entries: 9 001 branches 66 / 45 against 41 / 36, 15 999: 49 / 36 against 17 / 15; longer rows there take the large-tree image)
static inline bool windows_pay(uint32_t nb, uint64_t blob_units, uint64_t space, const Knobs &kn) {
    if (kn.window_always) return true;  // developer / test knob: the windowed kernel whatever the row density
    return 5 * blob_units <= 11 * space || nb > RK_WG_MIN_BRANCHES;
}
struct WindowPlan {
    uint32_t W = 0, n_win = 0, s_stride = 0, main_cap = 0, work_cap = 0;
    bool stream = false;          // place_packed16s_kernel first (decided when the image is built: its windows are narrower)
    double units_per_code = 0.0;  // row units / k-mer codes of the alphabet: what a read's k-mer brings on average
};
// The dense 16-lane geometry keeps eight waves per CU up to 1 116 branches (choose_geometry); beyond that -- and up to the
// 65 535 branches of the reference -- the tree is cut into windows of <= 1 024 branches, at most 64 of them
// (6-bit window ids in winspec and in the item tags), sized so that a wave's four reads fit 20 KB of LDS: 8 waves per CU again.
#ifndef RK_WSTREAM_MIN_BRANCHES
#define RK_WSTREAM_MIN_BRANCHES 4500u
#endif
// (RK_WSTREAM_MAX_UNITS: rk_plan.h)
static inline bool wstream_tree(uint32_t nb, uint32_t bits, double units_per_code, double units_per_row, const Knobs &kn) {  // images whose tiles go to place_packed16s_kernel first
    if (kn.wstream_always) return true;  // developer / test knob: the sorted-stream kernel on every windowed tree
    if (150.0 * units_per_code > RK_WSTREAM_MAX_UNITS) return false;
    // rows of several units (70 entries: 5) put few, long runs of slots into a window -- three or four rounds at its end -- and few
    // units per window and read, so that most of the list is padding: 9 001 / 15 999 / 25 001 branches 73 / 44 / 28 Mreads/s against
    // 77 / 53 / 39 (same profile); short rows only
    if (units_per_row > 2.5) return false;
    // amino acids: every windowed tree (the first kernel runs with register spills to keep two waves per SIMD: 274 / 248 / 194
    // Mreads/s at 1 400 / 1 999 / 3 999 branches against 280 / 272 / 241, C4-like rows; profiles/r03_wstream_crossover.txt)
    return bits == 5 || nb > RK_WSTREAM_MIN_BRANCHES;
}
static inline bool window_plan(uint32_t nb, uint32_t bits, double units_per_code, double units_per_row, const Knobs &kn, WindowPlan &wp) {
    if (nb <= RK_WINDOW_MIN_BRANCHES || nb > RK_WG_ALWAYS_BRANCHES) return false;
    // up to ~4 500 branches place_packed16w_kernel is ahead (windows of <= 1 024 branches, as few as possible: it pays per window);
    // beyond, place_packed16s_kernel (round 3: a window's cost follows what the read touches in it, so more and smaller windows --
    // about 500 branches, one bitmap word a lane -- cost little and leave the LDS to the list).  At most 64 windows: up to 1 024
    // branches each on the largest trees.  scripts/wstream_crossover.py, Mreads/s at 3 999 / 4 999 / 5 999 / 7 999 branches:
    // 164 / 147 / 132 / 113 with the first kernel, 159 / 150 / 144 / 135 with the second (profiles/r03_wstream_crossover.txt)
    wp.stream = wstream_tree(nb, bits, units_per_code, units_per_row, kn);
    wp.units_per_code = units_per_code;
    uint32_t n_win = wp.stream ? (nb + 511) / 512 : (nb + 895) / 896;
    if (n_win > RK_MAX_WINDOWS) n_win = RK_MAX_WINDOWS;
    wp.n_win = n_win;
    wp.W = ((nb + n_win - 1) / n_win + 3) & ~3u;
    wp.s_stride = wp.W + 4;
    const uint32_t per_group_words = 160 * 1024 / 8 / 4 / 4;  // 1280 u32 words per read = eight waves per CU
    // place_packed16w_kernel: the main list has to hold a whole read (C2-like reads: 145 row units on average, 250 at the tail); what
    // is left goes to the per-window work list, so that a window is normally applied in one accumulate call
    const uint32_t avail = per_group_words - wp.s_stride;
    // (88 words = the 44 keys the exact select of a window needs as scratch)
    uint32_t work = avail > 256 + 88 ? avail - 256 : 88;
    if (work > 200) work = 200;
    wp.work_cap = work & ~1u;
    wp.main_cap = (avail - wp.work_cap) & ~1u;
    if (wp.main_cap > 640) wp.main_cap = 640;
    return wp.main_cap >= 160;
}
// Which image a database gets, from its row lengths alone (slot_units = sum of ceil(len / 16) + 1, max_len, mean_len):
//   windowed (slot-offset rows + winspec, place_packed16w_kernel) when window_plan has a plan, the compact table applies (`direct`:
//     DIRECT, or AUTO over a small enough key space; no row beyond 255 units), the blob stays below 2 GB and windows_pay says so;
//   large-tree (indexed rows, place_wg_kernel) beyond 8 192 branches when the rows are long (mean >= RK_WG_MIN_MEAN_ROW), or when
//     no windowed image is possible beyond 16 000 branches (there the dense kernels hold one read per CU, or none at all beyond
//     ~39 000);
//   the plain slot-offset image of the dense kernels otherwise.
struct ImageKind { bool indexed, windowable; };
static inline ImageKind image_kind(uint32_t nb, uint32_t bits, bool direct, uint64_t space, uint64_t slot_units, uint32_t max_len, double mean_len, const Knobs &kn) {
    WindowPlan wp;
    // Just beyond 8 192 branches the dense 64-lane kernel (one wave per read, the whole score vector in the LDS) still holds three or
    // four reads per CU, and with rows of a few hundred entries it is ahead of both its neighbours (scripts/long_rows_big_tree.py,
    // scripts/long_rows_lanes64.py, profiles/r03_long_rows_big_tree.txt; Mreads/s, dense against the other):
    //   the windowed kernel, rows of 150 / 300: 9 001 branches 46.7 / 36.3 against 45.6 / 20.6; 13 001: 30.4 / 24.5 against 39.3 / 19.1;
    //   the workgroup-per-read kernel between its two regimes (slices of a row shorter than a turn of the ring), rows of 400 / 1 000:
    //   9 001 branches 31.0 / 14.3 against 16.2 / 12.3; 11 001: 22.2 / 11.0 against 16.0 / 12.1; 13 001: 21.3 / 10.7 against 15.9 / 12.1;
    //   15 999: 13.5 / 7.2 against 15.8 / 11.9
    const bool dense64_ahead = nb > RK_WG_MIN_BRANCHES && ((nb <= 9900u && mean_len >= 200.0 && mean_len < 1200.0) || (nb <= 13300u && mean_len >= 250.0 && mean_len < 750.0));
    const bool windowable = (!dense64_ahead || kn.window_always) && window_plan(nb, bits, space ? (double)slot_units / (double)space : 0.0, mean_len / ROW_ENTRIES + 0.5, kn, wp) && direct &&
                            (max_len + ROW_ENTRIES - 1) / ROW_ENTRIES <= 255 && slot_units * 128 < RK_WINDOW_MAX_BLOB && windows_pay(nb, slot_units, space, kn);
    const bool long_rows = mean_len >= RK_WG_MIN_MEAN_ROW;
    const bool indexed = nb > RK_WG_MIN_BRANCHES && ((long_rows && !dense64_ahead) || (!windowable && !dense64_ahead && nb > 16000u));
    return {indexed, windowable && !indexed};
}
// what one wave of a windowed kernel is launched with: four reads' slots, main list and work list (PlaceArgs of the same names)
struct WaveGeometry {
    uint32_t s_stride = 0, main_cap = 0, work_cap = 0, list_cap = 0, waves_cu = 0;
    size_t lds_wave = 0;
    bool wide = false;  // place_packed16s_kernel: two bitmap words a lane
};
static inline size_t lds_of_four_reads(uint32_t s_stride, uint32_t main_cap, uint32_t work_cap) { return (size_t)4 * (s_stride + main_cap + work_cap) * 4; }
static inline Status waves_that_fit(size_t lds_per_cu, uint32_t max_waves, WaveGeometry &o) {
    o.lds_wave = lds_of_four_reads(o.s_stride, o.main_cap, o.work_cap);
    o.waves_cu = (uint32_t)(lds_per_cu / o.lds_wave);
    if (o.waves_cu < 1) return WINDOWED_NO_FIT;
    if (o.waves_cu > max_waves) o.waves_cu = max_waves;
    return GEOM_OK;
}

// ---- place_packed16w_kernel: the image's plan, re-balanced for the launch ----
static inline Status windowed_geometry(const WindowPlan &plan, uint32_t keep_at_most, uint32_t words_per_read, size_t lds_per_cu, WaveGeometry &o) {
    // 88 words = the 44 keys the exact select of a window needs as scratch for keep_at_most <= 8 (K + 16 candidates + 16 winners); 96 beyond
    const uint32_t work_min = keep_at_most > 8 ? 96u : 88u;
    // the work list gets that at least -- and no more for reads beyond ~160 bases: a whole read in the main list matters more than one
    // accumulate call per window --, the main list the rest of what the plan gave the two
    o.work_cap = plan.work_cap < work_min || words_per_read > 10 ? work_min : plan.work_cap;
    o.main_cap = plan.main_cap + plan.work_cap - o.work_cap;
    o.s_stride = plan.s_stride; o.list_cap = o.work_cap / 2;
    return waves_that_fit(lds_per_cu, 8u, o);  // two waves per SIMD: the kernel's register budget
}

// ---- place_packed16s_kernel: the sorted list of a tile's four reads + their touched bitmaps.  Seven waves per CU on
//      the largest windows, eight otherwise; the list holds a C2-like read (145 units, 250 at the tail) with the padding of
//      its window segments ----
static inline bool sorted_wide(const WindowPlan &wp) { return wp.W > 512; }  // two bitmap words a lane
static inline Status sorted_geometry(const WindowPlan &wp, size_t lds_per_cu, WaveGeometry &o) {
    const uint32_t work_min = 96u;  // scratch of the second pass: 48 candidate keys
    // ring of row loads: eight deep, a window's segment padded to half turns of it (four deep it left the stream waiting
    // on HBM: ~280 cycles a step; segments padded to whole turns of eight made the largest trees' lists half filler)
    const uint32_t ring = 8u;
    uint32_t work = work_min > 64u + 3u * ring ? work_min : 64u + 3u * ring;  // (also: the 64 window counters of the emit, the touched bitmap of the stream)
    work = (work + 1) & ~1u;
    // the list: a C2-like read's 145 units (250 at the tail) + the padding of its window segments to the tile's longest
    const uint32_t need = 200 + 5 * wp.n_win + 3 * ring;
    const uint32_t s_str = wp.W + 16;  // a scratch word per lane in front of the window's slots
    uint32_t budget = 0;
    // two waves per SIMD (182 registers for DNA, 255 for amino acids).  Tried: three (167 registers, 28 bytes of scratch) and
    // the nine to eleven waves per CU the LDS then allows -- T8k 137 -> 97, T20k 102 -> 93 Mreads/s: the kernel is bound by
    // instruction issue, not by latency
    const uint32_t max_waves = 8u;
    for (uint32_t waves = max_waves; waves >= 5u; waves--) {
        budget = (160 * 1024 / waves / 512 * 512) / 4 / 4;  // (whole 512-byte granules per wave: see resident_per_cu)
        if (budget >= s_str + work + need) break;
    }
    uint32_t mainc = budget - s_str - work;
    if (mainc > 640) mainc = 640;
    mainc &= ~3u;  // (the list is read four items at a time)
    o.s_stride = s_str; o.main_cap = mainc; o.work_cap = work; o.list_cap = work / 2; o.wide = sorted_wide(wp);
    return waves_that_fit(lds_per_cu, max_waves, o);
}

// ---- place_hash64_kernel (rk_plan.h: RK_HASH_LOG_SLOTS, RK_HASH_KEY_SLACK): 2^log_slots slots twice, a word per lane and a list of 320
//      items a lane; a read's table takes key_limit keys (rk_plan::hash_key_limit) ----
constexpr uint32_t RK_HASH_MAIN_CAP = 320;
static inline WaveGeometry hash_geometry(uint32_t log_slots, uint32_t key_limit, size_t lds_per_cu, const Knobs &kn) {
    WaveGeometry o;
    o.s_stride = 1u << log_slots; o.main_cap = RK_HASH_MAIN_CAP; o.work_cap = key_limit; o.list_cap = 0;
    o.lds_wave = (size_t)(2 * o.s_stride + 64 + o.main_cap) * 4;
    const uint64_t want = lds_per_cu / o.lds_wave;
    o.waves_cu = want < kn.hash_waves ? (uint32_t)want : kn.hash_waves;  // developer knob
    return o;
}

// ---- large trees: one workgroup per read ----
struct WgGeometry { uint32_t nw, s_stride, list_cap, wgs_per_cu, n_pass; size_t lds; };
// The score vector of one read (4 bytes per branch) is shared by the NW waves of a workgroup.  While it fits, one pass:
// two workgroups of 8 waves per CU when two vectors fit (C5: 19 999 branches = 80 KB), else one of 16 waves.  Trees beyond one
// CU's LDS (about 39 000 branches; the reference's limit is the 16-bit id: 65 534) take 2 or 4 branch-range passes per read.
static inline Status choose_wg_geometry(uint32_t nb, size_t lds_per_cu, uint32_t keep_at_most, const Knobs &kn, WgGeometry &g) {
    const uint32_t min_pass = (uint32_t)kn.wg_passes;  // developer / test knob: force 2 or 4 passes on a tree that fits in one
    for (uint32_t P : {1u, 2u, 4u}) {
        if (P < min_pass) continue;
        const uint32_t span = 32 / P;
        uint32_t win = 0;
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t lo = (uint32_t)(((uint64_t)p * span * nb) / 32), hi = (uint32_t)(((uint64_t)(p + 1) * span * nb) / 32);
            if (hi - lo > win) win = hi - lo;
        }
        const uint32_t s_stride = (win + 4) & ~3u;  // >= win + 1 (word win is the scratch slot), multiple of 4 (b128 scans)
        const size_t s_bytes = (size_t)s_stride * 4;
        for (uint32_t wgs : {2u, 1u}) {
            if (P > 1 && wgs == 2) continue;  // (a tree that needs passes with 8 waves fits whole with 16)
            const uint32_t nw = wgs == 2 ? 8 : 16;
            const size_t budget = lds_per_cu / wgs;
            // P == 1: the wave winners of the level-1 select go to the hit list (free once every wave has its slices of the batch's rows);
            // P > 1: a region of their own.  (C5's two workgroups of 80 000-byte score vectors per CU leave ~1.9 KB)
            const size_t cand = P > 1 ? (size_t)(P * nw * keep_at_most + 16 + 2) * 8 : 0;
            const size_t extra = 256 + cand;  // per-wave hit counters
            const size_t wave_winners = (size_t)nw * keep_at_most + 18;
            const size_t min_list = P > 1 || wave_winners < 66 ? 66 : wave_winners;
            if (budget < s_bytes + extra + min_list * 8) continue;
            size_t cap = (budget - s_bytes - extra) / 8;
            if (cap > 512) cap = 512;
            g.nw = nw; g.s_stride = s_stride; g.list_cap = (uint32_t)cap & ~1u; g.wgs_per_cu = wgs; g.n_pass = P;
            g.lds = s_bytes + (size_t)g.list_cap * 8 + extra;
            return GEOM_OK;
        }
    }
    return NO_WG_WINDOW;
}

// ---- the ambiguity kernel (place_ascii_kernel), one wave per block ----
struct AmbGeometry { uint32_t s_stride = 0, amb_chunk = 0, s_win = 0; size_t lds = 0; uint32_t waves_cu = 0; };
// LDS: S[s_stride] + candidate list + Samb/Camb windows of `chunk` branches.  S holds the whole tree while that leaves room
// for the list and a minimal Samb/Camb window (then large trees take several ambiguity passes over the alternatives);
// beyond that (about 39 000 branches) S itself becomes a window of the tree and the read is walked once per window.
// list_bytes: the candidate list + the alphabet's tables, behind Camb (rk_kernels.hip: ASCII_LIST_CAP * 8 + ASCII_TABLE_BYTES)
static inline Status amb_geometry(uint32_t nb, size_t lds_per_cu, bool indexed, size_t list_bytes, const Knobs &kn, AmbGeometry &o) {
    uint32_t s_win = nb;
    size_t chunk;
    const bool force_windows = indexed && kn.wg_passes > 1;  // same test knob
    if (!force_windows && (size_t)((nb + 4) & ~3u) * 4 + list_bytes + 8 * 64 <= lds_per_cu) {
        o.s_stride = (nb + 4) & ~3u;
        const size_t fixed = (size_t)o.s_stride * 4 + list_bytes;
        chunk = o.s_stride;
        const size_t budget = 64 * 1024;  // prefer several waves per CU; grow only if a single pass would not fit
        if (fixed + 8 * chunk > budget) {
            size_t avail = (fixed + 8 * 64 <= budget ? budget : lds_per_cu) - fixed;
            chunk = avail / 8;
            if (chunk > o.s_stride) chunk = o.s_stride;
        }
    } else {
        // 12 bytes per branch of the window (S + Samb + Camb): the window is as large as one CU allows, split evenly
        const size_t per = (lds_per_cu - list_bytes - 64) / 12;
        uint32_t n_win = (uint32_t)((nb + per - 1) / per);
        if (force_windows && n_win < 3) n_win = 3;
        s_win = ((nb + n_win - 1) / n_win + 3) & ~3u;
        o.s_stride = s_win + 4;
        chunk = s_win;
    }
    if (chunk == 0 || o.s_stride == 0) return NO_SCORE_VECTOR;
    o.amb_chunk = (uint32_t)chunk;
    o.s_win = s_win;
    o.lds = (size_t)o.s_stride * 4 + list_bytes + 8 * chunk;  // S | list | Samb | Camb | tables
    const uint64_t waves_cu = lds_per_cu / o.lds;
    o.waves_cu = waves_cu > 32 ? 32u : (uint32_t)waves_cu;
    return GEOM_OK;
}

}  // namespace rk_geom
