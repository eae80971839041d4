// The image plan (rappas_amd/csrc/rk_image_plan.h) swept over its inputs: the row layout, the three k-mer tables and the amino-acid
// dense index must keep the rules the kernels read an image by.  Built and run by tests/test_image_plan_grid.py; no GPU, no HIP.
//   image_plan_grid      sweep the grid; prints one line per violated rule (the first case of each), then "N rules violated"; exit 1 if N
// Grid: row lengths 1..70, 239..242, 4079..4082 and n_branches (999, 4 500, 65 535); the slot-offset and the large-tree form of the
// layout; DNA (k = 5) and amino acids (k = 2); table modes AUTO, DIRECT, DIRECT8, HASH; keys packed together and spread out; the
// compact table's two developer knobs.
#include "rk_image_plan.h"

#include <cstdio>
#include <map>
#include <string>
#include <vector>

using namespace rk_image;

namespace {

std::map<std::string, std::string> violated;  // rule -> the first case that broke it
std::string where;
void rule(bool ok, const char *name) {
    if (!ok) violated.emplace(name, where);
}

// the device's probe (rk_device.h: mix64; rk_kernels.hip: lookup_desc<TM_HASH>), re-stated: start at mix64(code) & mask, step by one slot,
// stop at the slot that holds code + 1 or at an empty one
uint64_t device_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
uint64_t probe(const std::vector<uint64_t> &table, uint64_t mask, uint64_t code) {
    for (uint64_t h = device_mix64(code) & mask, n = 0; n <= mask; h = (h + 1) & mask, n++) {
        if (table[2 * h] == code + 1) return table[2 * h + 1];
        if (table[2 * h] == 0) return 0;
    }
    return 0;
}

std::vector<uint64_t> lengths(uint32_t n_branches) {
    std::vector<uint64_t> l;
    for (uint64_t v = 1; v <= 70; v++) l.push_back(v);
    for (uint64_t v : {239, 240, 241, 242, 4079, 4080, 4081, 4082}) l.push_back(v);
    l.push_back(n_branches);
    return l;
}

struct Rows {
    std::vector<uint64_t> dense, len, desc;
};

// every descriptor inside the blob, rows apart and on unit boundaries, the index line in the 64 bytes in front of its row
void check_layout(const RowLayout &lay, const Rows &r) {
    uint64_t end = lay.unit_bytes, units = 1;  // unit 0 is reserved
    for (size_t i = 0; i < r.desc.size(); i++) {
        const uint64_t start = (r.desc[i] >> DESC_LEN_BITS) * 8, lenp = r.desc[i] & DESC_LEN_MASK, len = r.len[i];
        const uint64_t bytes = lay.indexed ? lenp * 6 : lenp * 8, pad_to = lay.indexed ? 32 : ROW_ENTRIES;
        rule((r.desc[i] >> DESC_LEN_BITS) < (1ull << 40), "the row offset fits 40 bits");
        rule(lenp >= len && lenp - len < pad_to && lenp % pad_to == 0 && lenp <= DESC_LEN_MASK, "lenp is len padded to the form's step and fits DESC_LEN_MASK");
        rule(start % lay.unit_bytes == 0 && bytes % lay.unit_bytes == 0, "a row starts and ends on a unit boundary");
        rule(start == end + (lay.indexed ? 64 : 0), "a row follows the one before it, behind its own index line");
        rule(start + bytes <= lay.blob_bytes, "a row ends inside the blob");
        units += bytes / lay.unit_bytes + (lay.indexed ? 1 : 0);
        end = start + bytes;
    }
    rule(lay.blob_units == units && lay.blob_bytes == units * lay.unit_bytes && end == lay.blob_bytes, "blob_units is one more than the sum of the rows' units");
}

void check_direct(const ImageShape &s, const RowLayout &lay, const Rows &r, uint64_t space, const std::vector<uint64_t> &table) {
    rule(!lay.indexed && lay.max_units <= 255, "the compact table only holds slot-offset rows of <= 255 units");
    rule(!s.nib || lay.max_units <= 15, "the nibble form only holds rows of <= 15 units");
    const uint64_t per = s.nib ? 2 * COMPACT_KMERS : COMPACT_KMERS, n_blocks = (space + per - 1) / per;
    rule(s.slots == space && table.size() == n_blocks * 2, "the compact table has a block per 12 (24) codes");
    if (table.size() != n_blocks * 2) return;
    const unsigned char *tb = (const unsigned char *)table.data();
    std::vector<uint64_t> unit_of(space, 0), count_of(space, 0);
    uint64_t next = 1;
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint32_t base;
        memcpy(&base, tb + b * 16, 4);
        rule(base == next, "a block's base is one more than the units of every block before it");
        for (uint64_t j = 0; j < per && b * per + j < space; j++) {
            const uint64_t c = s.nib ? (tb[b * 16 + 4 + j / 2] >> (4 * (j & 1))) & 15u : tb[b * 16 + 4 + j];
            unit_of[b * per + j] = next;
            count_of[b * per + j] = c;
            next += c;
        }
    }
    rule(next == lay.blob_units, "the compact table's counts sum to the blob's units");
    uint64_t present = 0;
    for (size_t i = 0; i < r.dense.size(); i++) {
        const uint64_t start = (r.desc[i] >> DESC_LEN_BITS) * 8, lenp = r.desc[i] & DESC_LEN_MASK;
        rule(unit_of[r.dense[i]] * 128 == start && count_of[r.dense[i]] * ROW_ENTRIES == lenp, "the compact table decodes to the row's descriptor");
    }
    for (uint64_t c = 0; c < space; c++) present += count_of[c] != 0;
    rule(present == r.dense.size(), "a code without a row has a count of zero");
}

void check_table(uint32_t requested, const ImageShape &s, const RowLayout &lay, const Rows &r, uint32_t bits, uint32_t k, uint64_t space, const std::vector<uint64_t> &table) {
    const uint64_t n = r.dense.size();
    rule(s.mode == RK_TABLE_DIRECT || s.mode == RK_TABLE_DIRECT8 || s.mode == RK_TABLE_HASH, "the table mode is resolved");
    rule(requested == RK_TABLE_AUTO || requested == s.mode || (requested == RK_TABLE_DIRECT && s.mode == RK_TABLE_DIRECT8), "a requested mode is kept, but for DIRECT falling back to DIRECT8");
    if (s.mode == RK_TABLE_DIRECT) return check_direct(s, lay, r, space, table);
    rule(!s.nib, "only the compact table has a nibble form");
    if (s.mode == RK_TABLE_DIRECT8) {
        rule(s.slots == space && table.size() == space, "DIRECT8 has a descriptor per code");
        if (table.size() != space) return;
        uint64_t filled = 0;
        for (uint64_t c = 0; c < space; c++) filled += table[c] != 0;
        for (uint64_t i = 0; i < n; i++) rule(table[r.dense[i]] == r.desc[i], "DIRECT8 holds the row's descriptor at its dense index");
        rule(filled == n, "DIRECT8 is zero where no row is");
        return;
    }
    rule(s.slots >= 16 && (s.slots & (s.slots - 1)) == 0 && s.hash_mask == s.slots - 1 && table.size() == 2 * s.slots, "the hash table has a power of two of slots");
    rule(2 * n <= s.slots, "the hash table's load is at most 0.5");
    if (table.size() != 2 * s.slots) return;
    uint64_t filled = 0;
    for (uint64_t h = 0; h < s.slots; h++) filled += table[2 * h] != 0;
    rule(filled == n, "the hash table holds every key once");
    for (uint64_t i = 0; i < n; i++) rule(probe(table, s.hash_mask, code_of_dense(bits, k, r.dense[i])) == r.desc[i], "the device's probe finds every key");
    rule(probe(table, s.hash_mask, code_of_dense(bits, k, space - 1) + (1ull << 62)) == 0, "the device's probe finds no key that is not there");
}

void sweep_images() {
    for (uint32_t alphabet : {(uint32_t)RK_ALPHABET_DNA, (uint32_t)RK_ALPHABET_AA})
        for (uint32_t n_branches : {999u, 4500u, 65535u})
            for (bool indexed : {false, true})
                for (uint64_t stride : {1ull, 5ull}) {
                    const uint32_t k = alphabet == RK_ALPHABET_DNA ? 5 : 2, bits = bits_of(alphabet);
                    Rows r;
                    r.len = lengths(n_branches);
                    RowLayout lay(indexed);
                    uint64_t space = 0;
                    ipow_fits(alphabet, k, 1ull << 40, space);
                    for (size_t i = 0; i < r.len.size(); i++) {
                        r.dense.push_back(3 + i * stride);
                        r.desc.push_back(lay.add_row(r.len[i]));
                    }
                    char buf[160];
                    snprintf(buf, sizeof(buf), "alphabet=%u n_branches=%u indexed=%d stride=%llu", alphabet, n_branches, (int)indexed, (unsigned long long)stride);
                    where = buf;
                    rule(r.dense.back() < space, "the grid's keys lie inside the key space");
                    rule(lay.finish() == IMAGE_OK, "a small blob is accepted");
                    check_layout(lay, r);
                    // the same rows cut at every length of the list: the tables of few and many keys, of short rows only (nibbles) and of long ones
                    for (size_t n : {(size_t)0, (size_t)1, (size_t)15, (size_t)70, (size_t)72, (size_t)74, (size_t)76, r.len.size()})
                        for (uint32_t requested : {(uint32_t)RK_TABLE_AUTO, (uint32_t)RK_TABLE_DIRECT, (uint32_t)RK_TABLE_DIRECT8, (uint32_t)RK_TABLE_HASH})
                            for (int knob = 0; knob < 3; knob++) {
                                Rows part{{r.dense.begin(), r.dense.begin() + n}, {r.len.begin(), r.len.begin() + n}, {}};
                                RowLayout pl(indexed);
                                for (uint64_t len : part.len) part.desc.push_back(pl.add_row(len));
                                pl.finish();
                                const TableMode tm = resolve_table_mode(requested, alphabet, k, 1ull << 40);
                                snprintf(buf, sizeof(buf), "alphabet=%u n_branches=%u indexed=%d stride=%llu keys=%zu mode=%u knob=%d", alphabet, n_branches, (int)indexed,
                                         (unsigned long long)stride, n, requested, knob);
                                where = buf;
                                rule(tm.status == IMAGE_OK && tm.space == space && tm.space_ok, "a small key space takes every table mode");
                                ImageShape s;
                                s.mode = tm.mode;
                                s.n_keys = n;
                                std::vector<uint64_t> table;
                                build_table(s, space, pl, [&](uint64_t i) { return part.dense[i]; }, [&](uint64_t i) { return part.desc[i]; },
                                            [&](uint64_t i) { return code_of_dense(bits, k, part.dense[i]); }, Knobs{knob == 1, knob == 2}, table);
                                check_table(requested, s, pl, part, bits, k, space, table);
                                if (s.mode == RK_TABLE_DIRECT)
                                    rule(s.nib == (knob != 1 && pl.max_units <= 15 && (knob == 2 || 2 * pl.blob_units >= space)),
                                         "rows of <= 15 units take the nibble form where there is a unit per two codes (or the knob says so)");
                            }
                }
}

void sweep_scalars() {
    where = "scalars";
    rule(check_scalars(4, 2, 1, -1.0f, 0.1f) == IMAGE_OK && check_scalars(4, 31, 65535, -1.0f, 0.1f) == IMAGE_OK && check_scalars(20, 12, 9, -1.0f, 0.1f) == IMAGE_OK, "the ends of the ranges are accepted");
    rule(check_scalars(5, 8, 9, -1.0f, 0.1f) == BAD_ALPHABET && check_scalars(4, 1, 9, -1.0f, 0.1f) == K_OUT_OF_RANGE && check_scalars(4, 32, 9, -1.0f, 0.1f) == K_OUT_OF_RANGE &&
             check_scalars(20, 13, 9, -1.0f, 0.1f) == K_OUT_OF_RANGE && check_scalars(4, 8, 0, -1.0f, 0.1f) == BAD_BRANCHES && check_scalars(4, 8, 65536, -1.0f, 0.1f) == BAD_BRANCHES &&
             check_scalars(4, 8, 9, -INFINITY, 0.1f) == THRESHOLD_NOT_FINITE && check_scalars(4, 8, 9, -1.0f, NAN) == THRESHOLD_NOT_FINITE, "what lies outside is refused, each by its own status");
    for (uint32_t k = 2; k <= 31; k++)
        for (uint32_t requested = 0; requested <= 5; requested++)
            for (uint64_t limit : {1ull << 32, 1ull << 40}) {
                const TableMode t = resolve_table_mode(requested, 4, k, limit);
                const bool fits = 2 * k <= (limit >> 33 ? 40u : 32u), direct = t.mode == RK_TABLE_DIRECT || t.mode == RK_TABLE_DIRECT8;
                rule(t.space_ok == fits && t.space == (fits ? 1ull << (2 * k) : 0), "space is sigma^k where it fits the caller's limit");
                if (requested == RK_TABLE_AUTO) rule(t.status == IMAGE_OK && t.mode == (k <= 14 ? RK_TABLE_DIRECT : RK_TABLE_HASH), "AUTO is DIRECT up to 2^28 codes and HASH beyond");
                else if (requested == 3 || requested == 5) rule(t.status == BAD_TABLE_MODE, "a bad mode is refused");
                else rule(t.mode == requested && t.status == (direct && 2 * k > 31 ? DIRECT_TOO_LARGE : IMAGE_OK), "direct modes are refused beyond 2^31 codes");
            }
    RowLayout big(false);
    big.blob_units = (1ull << 36) - 1;
    rule(big.finish() == IMAGE_OK, "a blob of just under 8 TiB is accepted");
    big.blob_units++;
    rule(big.finish() == BLOB_TOO_LARGE, "a blob of 8 TiB is refused");
}

void sweep_amino_acids() {
    for (uint32_t k : {2u, 3u}) {
        where = "amino acids k=" + std::to_string(k);
        uint64_t space = 0, dense = 0, valid = 0;
        ipow_fits(20, k, 1ull << 40, space);
        for (uint64_t c = 0; c < space; c++) rule(aa_dense_of_code(aa_code_of_dense(c, k), k, dense) && dense == c && code_in_space(5, k, aa_code_of_dense(c, k)), "dense -> code -> dense is the identity");
        for (uint64_t code = 0; code < (1ull << (5 * k)); code++) {
            bool digits = true;
            for (uint32_t i = 0; i < k; i++) digits = digits && ((code >> (5 * i)) & 31) < 20;
            const bool ok = dense_of_code(5, k, code, dense);
            rule(ok == digits, "a code is accepted exactly when every digit is below 20");
            if (ok) rule(dense < space && aa_code_of_dense(dense, k) == code, "code -> dense -> code is the identity");
            valid += ok;
        }
        rule(valid == space && !dense_of_code(5, k, 1ull << (5 * k), dense), "sigma^k codes, none beyond 5k bits");
    }
    uint64_t dense = 0;
    where = "DNA";
    rule(dense_of_code(2, 5, 1023, dense) && dense == 1023 && !dense_of_code(2, 5, 1024, dense) && dense_of_code(2, 31, ~0ull >> 2, dense), "DNA codes are their own dense index");
}

}  // namespace

int main() {
    sweep_images();
    sweep_scalars();
    sweep_amino_acids();
    for (const auto &v : violated) printf("violated: %s (first at %s)\n", v.first.c_str(), v.second.c_str());
    printf("%zu rules violated\n", violated.size());
    return violated.empty() ? 0 : 1;
}
