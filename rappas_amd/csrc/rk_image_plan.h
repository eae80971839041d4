// rk_image_plan.h -- how a database becomes an HBM image: the scalar tests, the table mode, the layout of the row blob, which kind of
// image it is (plain, windowed, large-tree) and the k-mer table.  Pure host arithmetic without HIP and without getenv: both builders of
// rk_engine.hip (build_image for rk_db_create / rk_db_validate / rk_db_save_desc, and rk_db_create_synth) plan with it, and
// tests/image_plan_grid.cpp sweeps it on any machine.  A function that can refuse returns a Status; the engine turns it into the error
// code and text of the C ABI (image_error).  Nothing here catches std::bad_alloc: the entry points' guards do.
//
// What the two builders give the plan on purpose, and differently ("The image plan"):
//   the density the window plan sees (RowDensity) -- measured from the rows by rk_db_create, taken from the spec by the synthetic builder,
//     which has to know the window width before it has drawn a row;
//   carries_positions -- an image that is not windowed carries position keys (ImageShape::has_pos) when rk_db_create builds it, never
//     when it is generated;
//   ImageShape::mono, which the builder sets itself -- rk_db_create from the scores it reads, the synthetic builder from the sign of
//     the threshold (its scores are T * u, 0 <= u < 1).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "rk_geometry.h"
#include "../../include/rappas_place.h"  // RK_ALPHABET_*, RK_TABLE_*

namespace rk_image {

// (rk_device.h: ROW_UNIT, DESC_LEN_BITS, COMPACT_KMERS -- the engine asserts that they agree)
constexpr uint32_t ROW_ENTRIES = rk_geom::ROW_ENTRIES;  // entries per 128-byte row unit
constexpr int DESC_LEN_BITS = 24;                       // row descriptor: (offset in 8-byte words) << 24 | padded length
constexpr uint32_t DESC_LEN_MASK = (1u << DESC_LEN_BITS) - 1;
constexpr uint32_t COMPACT_KMERS = 12;                  // k-mers per 16-byte block of the compact table (24 in the nibble form)

enum Status { IMAGE_OK = 0, BAD_ALPHABET, K_OUT_OF_RANGE, BAD_BRANCHES, THRESHOLD_NOT_FINITE, DIRECT_TOO_LARGE, BAD_TABLE_MODE, BLOB_TOO_LARGE };
// the developer knobs (RK_*) build_table reads, as the engine found them (both false in the product library)
struct Knobs {
    bool compact_bytes = false;    // RK_COMPACT_BYTES: A/B against the byte form
    bool compact_nibbles = false;  // RK_COMPACT_NIBBLES: the half-size form whatever the density
};

// What an image is, apart from its bytes.  Every producer makes one (build_image, the synthetic builder, shape_of(ImageHeader), a
// handle keeps the one it was installed with) and every consumer reads one (info_of, header_of, install).
struct ImageShape {
    uint32_t alphabet = 0, convert_uo = 0, k = 0, n_branches = 0;  // the scalars every database carries, whatever built its image
    float thr_log10 = 0.0f, thr = 0.0f;
    uint32_t mode = 0, bits = 0, max_len = 0;  // table mode (never AUTO), bits per symbol, longest row
    bool indexed = false;   // rows carry an index line (large trees, place_wg_kernel)
    bool mono = true;       // every score >= thr_log10 (true of every database RAPPAS builds: words below the threshold are not stored)
    bool nib = false;       // the compact table holds 4-bit unit counts
    bool windowed = false;  // place_packed16w_kernel can serve this image: the third section holds a window span per k-mer code
    bool has_pos = false;   // not windowed, but the third section holds the rows' position in the tree (64 ranges): the key reads are grouped by
    uint64_t n_keys = 0, n_entries = 0, slots = 0, hash_mask = 0;
    rk_geom::WindowPlan wp;  // all zero unless windowed
    uint64_t table_bytes = 0, rows_bytes = 0, winspec_bytes = 0;  // the three sections; winspec_bytes = sigma^k when windowed || has_pos, else 0
};

// ---- scalars ----
static inline uint32_t bits_of(uint32_t alphabet) { return alphabet == RK_ALPHABET_DNA ? 2u : 5u; }
// DNA: 2 bits per base in a 64-bit code; from k = 16 on the reference allows two ambiguity codes per k-mer
// (maxAmbigPerMer = floor(k^(1/4)), AmbigSequenceKnife.java:95), three only from k = 81.  AA: 5 bits per residue.
static inline uint32_t max_k(uint32_t alphabet) { return alphabet == RK_ALPHABET_DNA ? 31u : 12u; }
static inline Status check_scalars(uint32_t alphabet, uint32_t k, uint32_t n_branches, float thr_log10, float thr) {
    if (alphabet != RK_ALPHABET_DNA && alphabet != RK_ALPHABET_AA) return BAD_ALPHABET;
    if (k < 2 || k > max_k(alphabet)) return K_OUT_OF_RANGE;
    if (n_branches < 1 || n_branches > 65535) return BAD_BRANCHES;  // (branch ids are 16-bit)
    if (!std::isfinite(thr_log10) || !std::isfinite(thr)) return THRESHOLD_NOT_FINITE;
    return IMAGE_OK;
}
static inline bool ipow_fits(uint64_t base, uint32_t e, uint64_t limit, uint64_t &out) {
    uint64_t v = 1;
    for (uint32_t i = 0; i < e; i++) {
        if (v > limit / base) return false;
        v *= base;
    }
    out = v;
    return true;
}

// ---- table mode ----
// space = sigma^k where it fits `limit` (the key-space cap of the caller: 2^40 for rk_db_create, 2^32 for the synthetic builder, which
// visits every code), else 0 with space_ok false.
struct TableMode { uint32_t mode; uint64_t space; bool space_ok; Status status; };
static inline TableMode resolve_table_mode(uint32_t requested, uint32_t alphabet, uint32_t k, uint64_t limit) {
    TableMode t{requested, 0, false, IMAGE_OK};
    t.space_ok = ipow_fits(alphabet, k, limit, t.space);
    // Direct addressing whenever all sigma^k codes fit 2^28 slots; DIRECT = compact 2-byte-per-k-mer blocks that
    // stay in the XCD L2s (measured on C2: 2.36e8 reads/s vs 2.18e8 with 8-byte descriptors, whose probes push the
    // Infinity Fabric to its ~6e10 requests/s ceiling -- scripts/ubench/gather_rate.hip).
    if (t.mode == RK_TABLE_AUTO) t.mode = (t.space_ok && t.space <= (1ull << 28)) ? RK_TABLE_DIRECT : RK_TABLE_HASH;
    const bool direct = t.mode == RK_TABLE_DIRECT || t.mode == RK_TABLE_DIRECT8;
    if (direct && !(t.space_ok && t.space <= (1ull << 31))) t.status = DIRECT_TOO_LARGE;
    else if (!direct && t.mode != RK_TABLE_HASH) t.status = BAD_TABLE_MODE;
    return t;
}

// ---- key code <-> dense index (the position of a k-mer among all sigma^k; rows and direct tables are in this order) ----
// DNA codes are their own dense index.  Amino acids: 5-bit digits to and from base 20 (dense_index<5> in rk_kernels.hip is the device's
// 32-bit Horner form of the first).
static inline bool code_in_space(uint32_t bits, uint32_t k, uint64_t code) { return !(bits * k < 64 && (code >> (bits * k))); }
static inline bool aa_dense_of_code(uint64_t code, uint32_t k, uint64_t &dense) {  // false: a digit >= 20
    uint64_t idx = 0, pw = 1;
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t dig = (code >> (5 * i)) & 31;
        if (dig >= 20) return false;
        idx += dig * pw;
        pw *= 20;
    }
    dense = idx;
    return true;
}
static inline uint64_t aa_code_of_dense(uint64_t dense, uint32_t k) {
    uint64_t code = 0;
    for (uint32_t j = 0; j < k; j++) { code |= (dense % 20) << (5 * j); dense /= 20; }
    return code;
}
static inline bool dense_of_code(uint32_t bits, uint32_t k, uint64_t code, uint64_t &dense) {  // false: not a k-mer code
    if (!code_in_space(bits, k, code)) return false;
    if (bits == 5) return aa_dense_of_code(code, k, dense);
    dense = code;
    return true;
}
static inline uint64_t code_of_dense(uint32_t bits, uint32_t k, uint64_t dense) { return bits == 5 ? aa_code_of_dense(dense, k) : dense; }

// ---- which kind of image (rk_geometry.h: image_kind, window_plan) ----
// what image_kind asks of the rows: slot_units = 1 + sum of ceil(len / 16), the longest row (clamped to 32 bits) and the mean length
struct RowStats {
    uint64_t n_keys = 0, n_entries = 0, slot_units = 1;
    uint32_t longest = 0;
    void add(uint64_t len) {
        n_keys++; n_entries += len;
        slot_units += (len + ROW_ENTRIES - 1) / ROW_ENTRIES;
        if (len > longest) longest = (uint32_t)(len > 0xFFFFFFFFull ? 0xFFFFFFFFull : len);
    }
    double mean_len() const { return n_keys ? (double)n_entries / (double)n_keys : 0.0; }
};
// what window_plan is told about the rows: row units per k-mer CODE and per row
struct RowDensity { double units_per_code, units_per_row; };
static inline RowDensity measured_density(const RowStats &rs, uint64_t space) {
    return {space ? (double)rs.slot_units / (double)space : 0.0, rs.mean_len() / ROW_ENTRIES + 0.5};
}
// (the rows are not drawn yet: key_fraction of the codes carry a row of mean_row_len entries)
static inline RowDensity spec_density(double key_fraction, double mean_row_len) {
    return {key_fraction * (mean_row_len / (double)ROW_ENTRIES + 0.5), mean_row_len / (double)ROW_ENTRIES + 0.5};
}
struct KindPlan {
    bool indexed = false;       // the large-tree form: sorted rows behind an index line
    bool want_windows = false;  // windowed, if the table stays compact and the blob below RK_WINDOW_MAX_BLOB (finish_shape)
    bool want_pos = false;      // else position keys
    bool carries_positions = false;
    uint32_t key_w = 1;         // branches per window, or per 64th of the tree: what a row's winspec byte counts in
    rk_geom::WindowPlan wp;
};
// Large trees (n_branches > RK_WG_MIN_BRANCHES): the score vector of one read fills most of a CU's LDS, so a whole workgroup shares it
// and every wave owns a branch range (place_wg_kernel) ... unless the rows are short: a workgroup's eight waves then each scan a sliver
// of every row, and one wave per read on a few resident score vectors does better (measured, rows of ~13 entries: 12 001 branches 29 vs
// 20 Mreads/s; the workgroup kernel is ahead again from ~16 000 branches on, where two score vectors fill a CU, and always for long rows).
// Images the dense kernels serve get the winspec byte per k-mer code with the tree cut into 64 equal ranges: not for any window -- the
// kernels hold the whole score vector -- but as the position a batch's reads are grouped by (reads of one clade read the same rows:
// taken together they find them in the L2; scripts/clade_sorted_probe.py: 283 -> 406 Mreads/s on C2's shape).
static inline KindPlan plan_kind(uint32_t n_branches, uint32_t bits, const TableMode &tm, const RowStats &rs, const RowDensity &density,
                                 bool carries_positions, const rk_geom::Knobs &kn) {
    KindPlan p;
    const rk_geom::ImageKind kind = rk_geom::image_kind(n_branches, bits, tm.mode == RK_TABLE_DIRECT, tm.space, rs.slot_units, rs.longest, rs.mean_len(), kn);
    p.indexed = kind.indexed;
    p.carries_positions = carries_positions;
    p.want_windows = kind.windowable && rk_geom::window_plan(n_branches, bits, density.units_per_code, density.units_per_row, kn, p.wp);
    p.want_pos = carries_positions && !p.want_windows && !p.indexed && tm.space_ok && tm.space <= (1ull << 26);
    p.key_w = p.want_windows ? p.wp.W : (n_branches + 63u) / 64u > 1u ? (n_branches + 63u) / 64u : 1u;
    return p;
}

// ---- row blob: every row starts on a 128-byte unit and is padded to whole units (16 entries of {slot offset, score}), so a row of n
//      entries costs exactly ceil(n/16) aligned 128-byte requests; unit 0 is reserved (all padding).  The large-tree form has 64-byte
//      units: rows sorted by branch id as [u16 branch[lenp]][f32 score[lenp]], lenp a multiple of 32 so that the row is whole lines,
//      preceded by one 64-byte INDEX line: u16 split[i-1] = number of entries with branch < floor(i * n_branches / 32), i = 1..32, so a
//      wave finds its slice of a row with two 2-byte loads.  Descriptors point at the first entry line; the other kernels never look at
//      the index line. ----
struct RowLayout {
    bool indexed;
    uint64_t unit_bytes, blob_units = 1, max_units = 0, blob_bytes = 0;
    explicit RowLayout(bool indexed_) : indexed(indexed_), unit_bytes(indexed_ ? 64 : ROW_ENTRIES * 8) {}
    uint64_t add_row(uint64_t len) {  // the next row, in dense-index order: its descriptor
        uint64_t units = (len + ROW_ENTRIES - 1) / ROW_ENTRIES, lenp = units * ROW_ENTRIES;
        if (indexed) {
            blob_units += 1;  // the index line
            lenp = (len + 31) / 32 * 32;
            units = lenp * 6 / 64;
        }
        if (units > max_units) max_units = units;
        const uint64_t desc = ((blob_units * (unit_bytes / 8)) << DESC_LEN_BITS) | lenp;
        blob_units += units;
        return desc;
    }
    Status finish() {
        blob_bytes = blob_units * unit_bytes;
        return (blob_bytes >> 3) >= (1ull << 40) ? BLOB_TOO_LARGE : IMAGE_OK;  // 40-bit word offsets: 8 TiB
    }
};

// ---- k-mer -> row descriptor table, keys given in ascending dense-index order through the accessors (template parameters: they inline) ----
// DIRECT  : compact blocks, 16 bytes per 12 consecutive k-mers {u32 first row unit, 12 x u8 units per row}: 1.33 bytes
//           per k-mer (1.4 MiB at k=10) -- or per 24 k-mers with 4-bit unit counts (see `nib` below) -- small enough to live in the XCD L2s, one dwordx4 gather per probe; a row's
//           offset is the block base plus a byte prefix sum.  Needs rows of <= 255 units (4080 entries) and a blob
//           of < 2^32 units (512 GiB); otherwise DIRECT falls back to DIRECT8.
// DIRECT8 : one 8-byte descriptor per k-mer.
// HASH    : open addressing, linear probing, 16-byte slots {key+1, descriptor}, load <= 0.5.
static inline uint64_t host_mix64(uint64_t x) {  // (rk_device.h: mix64)
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
// fills s.mode (DIRECT may become DIRECT8), s.slots, s.hash_mask, s.nib and `table`; reads s.n_keys
template <class FDense, class FDesc, class FCode>
static inline void build_table(ImageShape &s, uint64_t space, const RowLayout &lay, FDense dense_of, FDesc desc_of, FCode code_of, const Knobs &kn,
                               std::vector<uint64_t> &table) {
    const uint64_t n_keys = s.n_keys;
    if (s.mode == RK_TABLE_DIRECT && (lay.max_units > 255 || lay.blob_units >= (1ull << 32) || lay.indexed)) s.mode = RK_TABLE_DIRECT8;
    s.slots = 0; s.hash_mask = 0;
    // 4-bit unit counts (24 k-mers per block, 0.67 bytes per k-mer) whenever no row exceeds 15 units = 240 entries: half the table
    // means its lines are re-touched twice as often and survive the rows streaming through the same L2 sets (C2: 15 of a read's 141
    // probes missed the L2 with the byte form)
    // ... where rows stream at all: with fewer than one row unit per two k-mer codes (C4: 0.13) the probes outnumber the row lines,
    // nothing evicts the table and the longer decode is all that is left (C4: 5.37e8 against 5.52e8 reads/s)
    s.nib = s.mode == RK_TABLE_DIRECT && lay.max_units <= 15 && (2 * lay.blob_units >= space || kn.compact_nibbles) && !kn.compact_bytes;
    if (s.mode == RK_TABLE_DIRECT) {
        s.slots = space;
        const uint64_t per = s.nib ? 2 * COMPACT_KMERS : COMPACT_KMERS;
        const uint64_t n_blocks = (space + per - 1) / per;
        table.assign(n_blocks * 2, 0);
        unsigned char *tb = (unsigned char *)table.data();
        uint64_t next_unit = 1, ki = 0;
        for (uint64_t blk = 0; blk < n_blocks; blk++) {
            const uint32_t base32 = (uint32_t)next_unit;
            memcpy(tb + blk * 16, &base32, 4);
            while (ki < n_keys && dense_of(ki) / per == blk) {
                const uint64_t units = ((uint32_t)desc_of(ki) & DESC_LEN_MASK) / ROW_ENTRIES;
                const uint64_t j = dense_of(ki) % per;
                if (s.nib) tb[blk * 16 + 4 + j / 2] |= (unsigned char)(units << (4 * (j & 1)));
                else tb[blk * 16 + 4 + j] = (unsigned char)units;
                next_unit += units;
                ki++;
            }
        }
    } else if (s.mode == RK_TABLE_DIRECT8) {
        s.slots = space;
        table.assign(s.slots, 0);
        for (uint64_t i = 0; i < n_keys; i++) table[dense_of(i)] = desc_of(i);
    } else {
        s.slots = 16;
        while (s.slots < 2 * n_keys) s.slots <<= 1;
        s.hash_mask = s.slots - 1;
        table.assign(s.slots * 2, 0);
        for (uint64_t i = 0; i < n_keys; i++) {
            const uint64_t code = code_of(i);
            uint64_t h = host_mix64(code) & s.hash_mask;
            while (table[2 * h]) h = (h + 1) & s.hash_mask;
            table[2 * h] = code + 1;
            table[2 * h + 1] = desc_of(i);
        }
    }
}

// ---- the closing assignments, once the table is built (s.mode is final) ----
// windows need the compact table (rows of <= 255 units) and 32-bit row offsets; an image that wanted windows and cannot have them, or
// wanted positions, carries position keys behind a direct table -- when its builder gives any
static inline void finish_shape(ImageShape &s, const RowLayout &lay, const KindPlan &p, uint64_t table_words, uint32_t max_len, uint64_t space) {
    s.indexed = lay.indexed;
    s.table_bytes = table_words * sizeof(uint64_t);
    s.rows_bytes = lay.blob_bytes;
    s.max_len = max_len;
    s.windowed = p.want_windows && s.mode == RK_TABLE_DIRECT && lay.blob_bytes < rk_geom::RK_WINDOW_MAX_BLOB;
    s.has_pos = p.carries_positions && !s.windowed && (p.want_windows || p.want_pos) && (s.mode == RK_TABLE_DIRECT || s.mode == RK_TABLE_DIRECT8);
    if (s.windowed) s.wp = p.wp;
    s.winspec_bytes = (s.windowed || s.has_pos) ? space : 0;
}

}  // namespace rk_image
