// rk_plan.h -- which kernels place a batch on a windowed tree with short rows: the first kernel of each class of
// batch, the launches that follow from it and the tiles place_packed16w_kernel takes.  Pure host arithmetic without HIP: rk_engine.hip
// (launch_windowed, rk_kernel_name) decides with it, and tests/plan_grid.cpp sweeps it on any machine.
#pragma once
#include <cstdint>
#include <initializer_list>

// Row units a 150-symbol read brings (its ~150 k-mers x the row units per k-mer CODE of the image) beyond which the sorted list of
// place_packed16s_kernel stops fitting and place_packed16w_kernel alone is ahead: scripts/long_rows_big_tree.py, 9 001 branches,
// a quarter of the 9-mers present, rows of 70 / 150 / 300 entries (~170 / 350 / 680 units a read): 73 / 35 / 15 Mreads/s with the
// second kernel first, 77 / 46 / 21 without (profiles/r03_long_rows_big_tree.txt)
#ifndef RK_WSTREAM_MAX_UNITS
#define RK_WSTREAM_MAX_UNITS 220.0
#endif
// place_hash64_kernel's geometry: NS = 2 048 slots (16 KB) + a word per lane + a list of 320 items = 17 920 B per wave, nine waves per CU
#ifndef RK_HASH_LOGS
#define RK_HASH_LOGS 11
#endif
constexpr uint32_t RK_HASH_LOG_SLOTS = RK_HASH_LOGS;
#ifndef RK_HASH_KEY_SLACK
#define RK_HASH_KEY_SLACK 48u  // slots kept free: a read's table takes NS - this many keys (the kernel counts a step's entries before it takes the step)
#endif
// From this many branches on place_hash64_kernel is ahead of place_packed16s_kernel, whose cost grows with the windows a tree is cut
// into (profiles/r04_hash_crossover.txt and DESIGN.md 4.1d; C2-like rows, Mreads/s hash / sorted-stream: uniform reads 19 999 branches
// 94 / 108, 28 001: 95 / 95, 39 999: 95 / 71, 65 535: 94 / 35; clade-shaped reads 82 / 119 at 28 001, 81 / 95 at 39 999, 82 / 47 at
// 65 535; 92 / 81 at 50 001, 84 / 81 at 55 001, 48 / 81 at 60 001).  Uniform reads cross at ~28 000 branches, clade-shaped ones at ~56 000: in between BOTH kernels are launched and the
// batch's shape -- what the re-tiling pre-pass found, on the device -- says which of them runs (PlaceArgs::only_if); a batch without
// the pre-pass (fewer than 32 768 reads) goes by the single rule in the middle.
#ifndef RK_HASH_MIN_BRANCHES_CLADE
#define RK_HASH_MIN_BRANCHES_CLADE 56000u
#endif

namespace rk_plan {

// the developer knobs (RK_*) the plan reads, as the engine found them (all false in the product library)
struct Knobs {
    bool hash_always = false;       // RK_HASH_ALWAYS
    bool hash_big_table = false;    // RK_HASH_BIG_TABLE
    bool hash_small_table = false;  // RK_HASH_SMALL_TABLE
    bool hash_clade_small = false;  // RK_HASH_CLADE_SMALL
    bool wstream_always = false;    // RK_WSTREAM_ALWAYS
    bool no_wstream = false;        // RK_NO_WSTREAM
    uint32_t key_slack = RK_HASH_KEY_SLACK;  // RK_HASH_KEY_SLACK
};

// amino acids (k = 5, 100 residues, C4-like rows: a quarter of the k-mers present, ~300 entries a read): the hash kernel runs 196 Mreads/s
// at any size, place_packed16s_kernel 231 / 205 / 177 / 119 / 51 at 9 001 / 12 001 / 15 999 / 33 001 / 65 535 branches -- they cross at
// ~13 500; reads cut from the sequence the k-mers come from 107 against 198 / 168 / 136 / 65 at 9 001 / 25 001 / 46 001 / 60 001: ~56 000
// as for DNA (profiles/r04_hash_crossover_aa.txt).
// The hash kernel's cost follows a read's row units, place_packed16s_kernel's the units AND the windows: through the two measured
// crossings -- 145 units a read (C2, 150 bp) at 28 000 branches, 33 (C4-like, 100 residues) at 13 500 -- the uniform crossing is taken as
// 130 branches per unit + 9 250 for other row densities and read lengths; batches too small for the pre-pass go by that + 8 000
// (36 000 for C2-like rows).  -DRK_HASH_MIN_BRANCHES_UNIFORM_FIXED=n replaces the fit by a constant.
// Reads that bring few row entries even when every k-mer of theirs has a row take the table of 1 024 slots (hash_small_table): sixteen waves
// per CU, half the reset and the scan.  Forced onto the protein sweep above (RK_HASH_SMALL_TABLE; its reads hit a quarter of their k-mers, a real
// read would overflow that table) it gives 310 Mreads/s on uniform reads and 170 on clade-shaped ones at every size, and the crossings move to ~2 600 branches
// (place_packed16s_kernel: 329 / 297 at 2 001 / 3 100) and ~24 000 (181 / 168 / 151 at 15 999 / 25 001 / 33 001).  One measured crossing only in
// this regime: 19 branches per unit + 2 000 (a tree of four windows: the table's reset and scan do not shrink with the read) passes through it.
// (clade-shaped batches through the 1 024-slot table with the large one behind it: DNA 96 - 100 Mreads/s at any size against place_packed16s_kernel's
//  128 / 106 / 95 / 92 / 84 / 48 at 19 999 / 33 001 / 46 001 / 50 001 / 55 001 / 60 001 branches -- they cross at ~42 000; amino acids 170 against
//  181 / 168 / 151 at 15 999 / 25 001 / 33 001: ~24 000.  Through both: 160 branches per row unit of a read + 18 700)
static inline uint32_t hash_min_clade_small(double est_units) {
#ifdef RK_HASH_MIN_BRANCHES_CLADE_SMALL
    (void)est_units;
    return RK_HASH_MIN_BRANCHES_CLADE_SMALL;
#else
    const double nb = 160.0 * est_units + 18700.0;
    return nb > 65535.0 ? 65535u : (uint32_t)nb;
#endif
}
static inline uint32_t hash_min_clade(bool small_table) { return small_table ? 24000u : RK_HASH_MIN_BRANCHES_CLADE; }
static inline uint32_t hash_min_uniform(double est_units, bool small_table) {
#ifdef RK_HASH_MIN_BRANCHES_UNIFORM_FIXED
    (void)est_units;
    return RK_HASH_MIN_BRANCHES_UNIFORM_FIXED;
#else
    const double nb = small_table ? 19.0 * est_units + 2000.0 : 130.0 * est_units + 9250.0;
    return nb > (double)hash_min_clade(small_table) ? hash_min_clade(small_table) : (uint32_t)nb;
#endif
}
static inline uint32_t hash_min_single(double est_units, bool small_table) {
    const uint32_t u = hash_min_uniform(est_units, small_table) + 8000u;
    return u > hash_min_clade(small_table) ? hash_min_clade(small_table) : u;
}
static inline uint32_t hash_key_limit(const Knobs &kn, uint32_t log_slots = RK_HASH_LOG_SLOTS) {
    uint32_t slack = kn.key_slack;
    const uint32_t ns = 1u << log_slots;
    if (slack < 16u) slack = 16u;
    if (slack > ns - 64u) slack = ns - 64u;
    return ns - slack;
}
// The table of 1 024 slots: full_hit_entries < 0 asks "in no case"; otherwise it holds the row ENTRIES of a read all of whose k-mers have a
// row (mean row length x its k-mers) -- what a read from an organism of the reference brings, four times the uniform estimate of C4-like
// rows -- and the small table is taken only when even that fits: a read that overflows costs a tile of place_packed16w_kernel.
static inline bool hash_small_table(double full_hit_entries, const Knobs &kn) {
    if (kn.hash_big_table || full_hit_entries < 0.0) return false;  // (developer knob: A/B)
    return kn.hash_small_table || full_hit_entries <= 0.8 * hash_key_limit(kn, RK_HASH_LOG_SLOTS - 1);
}
static inline double full_hit_entries(uint32_t symbols, uint32_t k, uint64_t n_keys, uint64_t n_entries) {
    const double kmers = symbols > k ? (double)(symbols - k + 1) : 0.0;
    return n_keys ? kmers * (double)n_entries / (double)n_keys : 0.0;
}

// ---- the reads of a batch: the longest read its records hold (the reads may be longer than the 150 symbols the image was judged for),
//      the row units that brings (its k-mers x the image's row units per code), and whether a read of one known length has its k-mers
//      in one probe batch (reads that do not would all be handed over: no first kernel is launched for those) ----
struct ReadShape {
    uint32_t max_syms;
    double est_units;
    bool one_batch;
};
static inline ReadShape read_shape(uint32_t bits_per_symbol, uint32_t k, uint32_t words_per_read, bool lens_given, uint32_t fixed_len, double units_per_code) {
    ReadShape s;
    s.max_syms = lens_given ? words_per_read * 32 / bits_per_symbol : fixed_len;
    s.est_units = (s.max_syms > k ? s.max_syms - k + 1 : 0) * units_per_code;
    const uint32_t probe_cap = (bits_per_symbol == 5 ? 7u : 9u) * 16u;
    s.one_batch = lens_given || fixed_len < k || fixed_len - k + 1 <= probe_cap;
    return s;
}

struct In {
    uint32_t n_branches = 0;
    double est_units = 0.0;         // ReadShape::est_units
    double full_hit_entries = 0.0;  // full_hit_entries() of ReadShape::max_syms
    bool hash_capable = false;      // the image's tiles can go to place_hash64_kernel first (rk_engine.hip: hash_capable)
    uint32_t words_per_read = 0;
    bool one_batch = false;         // ReadShape::one_batch
    bool stream = false;            // WindowPlan::stream: place_packed16s_kernel first (decided when the image was built)
    bool verdict = false;           // the batch went through the re-tiling pre-pass: its class is judged on the device
    bool first_ok = false;          // scratch for the tile marks: a first kernel can hand tiles over
    bool marked_list = false;       // ... and for the list of the marked tiles (the queue of a second launch)
    Knobs knobs;
};

// what may go first at all: place_hash64_kernel on images of short rows (the rule place_packed16s_kernel had), for reads whose distinct
// branches -- at most their entries, ~9.3 a unit with C2-like rows -- fit the table (profiles/r04_lsize_hist.txt); reads of few row units
// (a protein database: ~300 entries a read) on the table of 1 024 slots -- half the reset and the scan, 9.7 KB a wave, sixteen waves per
// CU instead of nine; place_packed16s_kernel for records of <= 16 words whose k-mers fit one probe batch and its list
struct Fit {
    bool hash_fits, hash_small, sorted_fits;
    bool want_marks() const { return hash_fits || sorted_fits; }
};
static inline Fit plan_fit(const In &in) {
    const Knobs &kn = in.knobs;
    Fit f;
    f.hash_fits = !kn.no_wstream && in.hash_capable && (in.est_units * 9.3 <= 0.8 * hash_key_limit(kn) || kn.hash_always);
    f.hash_small = hash_small_table(in.full_hit_entries, kn);
    f.sorted_fits = in.words_per_read <= 16 && !kn.no_wstream && in.stream && in.one_batch && (in.est_units <= 1.25 * RK_WSTREAM_MAX_UNITS || kn.wstream_always);
    return f;
}

// ---- which kernel goes first on a windowed tree with short rows, per class of batch ----
enum First { F_NONE, F_SORTED, F_HASH_BIG, F_HASH_SMALL };
struct FirstPlan { First for_uniform, for_sparse, for_clade; };
static inline FirstPlan first_kernel_plan(const In &in, const Fit &fit) {
    const Knobs &kn = in.knobs;
    const uint32_t nb_tree = in.n_branches;
    const double est_units = in.est_units;
    const bool hash_small = fit.hash_small, hash_fits = fit.hash_fits, sorted_fits = fit.sorted_fits, verdict = in.verdict;
    const First table_u = hash_small ? F_HASH_SMALL : F_HASH_BIG;
    FirstPlan p;
    if (kn.hash_always && hash_fits) {
        p.for_uniform = p.for_sparse = p.for_clade = table_u;
        return p;
    }
    // (the single rule of batches without the pre-pass: place_hash64_kernel beyond hash_min_single)
    const bool hash_tree = in.hash_capable && (kn.hash_always || nb_tree > hash_min_single(est_units, hash_small));
    const uint32_t min_u = verdict ? hash_min_uniform(est_units, hash_small) : hash_min_single(est_units, hash_small);
    p.for_uniform = hash_fits && nb_tree > min_u ? table_u : sorted_fits ? F_SORTED : hash_fits && hash_tree ? table_u : F_NONE;
    p.for_clade = p.for_sparse = p.for_uniform;
    if (verdict) {
        // reads of a clade touch a third of the branches uniform reads do (profiles/r04_lsize_hist.txt: ~500 against ~1 300; max 1 135): their
        // tables fit the 1 024-slot instantiation -- sixteen waves per CU -- and the few that do not are placed by the large one, launched
        // behind it on the tiles it hands over
        const bool clade_small = hash_fits && !hash_small && (kn.hash_clade_small || nb_tree > hash_min_clade_small(est_units)) && !kn.hash_big_table;
        p.for_clade = clade_small ? F_HASH_SMALL : hash_fits && nb_tree > hash_min_clade(hash_small) ? table_u : sorted_fits ? F_SORTED : p.for_uniform;
        // uniform batches whose k-mers hit no more often than a random read's (the pre-pass's second verdict): the uniform estimate of a read's
        // entries holds, and where that fits the 1 024-slot table the small instantiation serves them (the large one behind it, as for clades)
        if (hash_fits && !hash_small && !kn.hash_big_table && est_units * 9.3 <= 0.6 * hash_key_limit(kn, RK_HASH_LOG_SLOTS - 1) && nb_tree > hash_min_uniform(est_units, true))
            p.for_sparse = F_HASH_SMALL;
    }
    return p;
}

// one launch of a first kernel: only_if = the classes of batches it serves (PlaceArgs::only_if: bit 0 uniform reads that hit often,
// bit 1 uniform reads that hit like random ones, bit 2 reads of a clade; 0 = unconditional)
struct Launch {
    bool run = false;
    uint32_t only_if = 0;
};
struct Plan {
    Fit fit;
    FirstPlan first;
    Launch hash_small;   // place_hash64_kernel with 1 024 slots
    Launch hash_big;     // place_hash64_kernel with 2 048 slots
    Launch hash_behind;  // ... with 2 048 slots on the tiles the small table handed over (only_marked), ahead of place_packed16w_kernel
    Launch sorted;       // place_packed16s_kernel
    // place_packed16w_kernel, always launched last: every tile, or (only_marked) the tiles the first kernels handed over -- of the batches
    // of the classes in marked_if (PlaceArgs::marked_if, 0 = all three); a batch of any other class had no first kernel: every tile of it
    bool only_marked = false;
    uint32_t marked_if = 0;
};
static inline Plan launch_plan(const In &in) {
    Plan p;
    p.fit = plan_fit(in);
    p.first = first_kernel_plan(in, p.fit);
    const First by_class[3] = {p.first.for_uniform, p.first.for_sparse, p.first.for_clade};
    auto class_mask = [&](First f) -> uint32_t {
        uint32_t m = 0;
        for (int c = 0; c < 3; c++) m |= by_class[c] == f ? 1u << c : 0u;
        return m;
    };
    auto only_if = [](uint32_t m) { return m == 7u ? 0u : m; };
    if (!in.first_ok) return p;  // (no scratch to be had for the marks: place_packed16w_kernel alone)
    uint32_t served = 0;
    bool small_on_trust = false;
    for (First f : {F_HASH_SMALL, F_HASH_BIG}) {
        const uint32_t m = class_mask(f);
        if (!m) continue;
        (f == F_HASH_SMALL ? p.hash_small : p.hash_big) = Launch{true, only_if(m)};
        served |= m;
        small_on_trust = small_on_trust || (f == F_HASH_SMALL && !p.fit.hash_small);
    }
    // the tiles the small table handed over: the large one next, only for the batches the small table took
    if (small_on_trust && in.marked_list) p.hash_behind = Launch{true, only_if(class_mask(F_HASH_SMALL))};
    if (const uint32_t m = class_mask(F_SORTED)) {
        p.sorted = Launch{true, only_if(m)};
        served |= m;
    }
    p.only_marked = served != 0u;
    p.marked_if = only_if(served);
    return p;
}

}  // namespace rk_plan
