// The host twin of the squash clustering (rappas_amd/csrc/rk_samples_host.h: squash_pick, squash_merge_profiles, squash_row,
// squash_steps) run on its own, so that tests/test_squash_host_cpp.py can build it with the address and undefined-behaviour
// sanitizers: seeded trees of B = 1, 2, 300, 2049, 4097 nodes (random with shuffled ids, caterpillar, star) with S = 2, 3, 6, 33
// samples, an empty sample, two identical ones and 2^62 on one branch.  The rows are held against what the definition promises of
// any run, against a second run whose row step is dealt to three, and against the matrix recomputed from the merged profiles.
#include "rk_samples_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

unsigned long long checked = 0, wrong = 0;
void expect(bool ok, const char *what, unsigned a = 0, unsigned b = 0) {
    checked++;
    if (!ok) {
        wrong++;
        printf("WRONG: %s (%u, %u)\n", what, a, b);
    }
}

struct Run {
    std::vector<double> u, v, D;
    std::vector<uint8_t> active;
    std::vector<rk::SquashMerge> rows;
    uint32_t n = 0;
};

void one_shape(uint32_t B, uint32_t S, int kind, bool special, std::mt19937_64 &rng) {
    std::vector<int32_t> parent(B, -1);
    std::vector<float> bl(B);
    for (uint32_t x = 1; x < B; x++) parent[x] = kind == 1 ? (int32_t)(x - 1) : kind == 2 ? 0 : (int32_t)(rng() % x);
    for (uint32_t x = 0; x < B; x++) bl[x] = (float)(rng() % 4096) / 1024.0f;
    if (kind == 0 && B > 1) {  // ids out of pre-order: swap the root's id with another node's
        const uint32_t y = 1 + (uint32_t)(rng() % (B - 1));
        for (uint32_t x = 0; x < B; x++) parent[x] = parent[x] == 0 ? (int32_t)y : parent[x] == (int32_t)y ? 0 : parent[x];
        std::swap(parent[0], parent[y]);
        std::swap(bl[0], bl[y]);
    }
    char msg[256];
    rk::TreeWalk w;
    if (rk::tree_walk("test", B, parent.data(), bl.data(), true, w, msg, sizeof(msg))) {
        expect(false, msg, B, S);
        return;
    }
    const uint64_t W = 2 * (uint64_t)B + 4;
    std::vector<uint64_t> m(S * W + 1, 0);
    for (uint32_t s = 0; s < S; s++) {
        for (uint32_t x = 0; x < B; x++) m[s * W + x] = rng() % 3 == 0 ? rng() % (1ull << 34) : 0;
        m[s * W + rng() % B] += 1u << 30;  // no sample empty by chance
    }
    if (special) {  // S >= 5: sample 1 empty, 3 a copy of 2, 4 with 2^62 on one branch
        for (uint32_t x = 0; x < B; x++) { m[1 * W + x] = 0; m[3 * W + x] = m[2 * W + x]; m[4 * W + x] = 0; }
        m[4 * W + B / 2] = 1ull << 62;
        m[4 * W + B - 1] += 12345;
    }
    std::vector<uint64_t> clade(S * (uint64_t)B);
    std::vector<double> h(B);
    for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(bl.data(), x, w.root);
    Run base;
    base.u.resize(S * (uint64_t)B);
    base.v.resize(S * (uint64_t)B);
    base.D.assign((uint64_t)S * S, -1.0);
    base.active.resize(S);
    base.rows.resize(S - 1);
    for (uint32_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, parent.data(), m.data() + s * W, clade.data() + (uint64_t)s * B);
        rk::kr_profiles_sample(B, w.root, m.data() + s * W, clade.data() + (uint64_t)s * B, base.u.data() + (uint64_t)s * B, base.v.data() + (uint64_t)s * B);
        base.active[s] = clade[(uint64_t)s * B + w.root] != 0;
    }
    rk::kr_rows(B, S, h.data(), base.u.data(), base.v.data(), 0, 1, base.D.data());
    Run one = base, three = base;
    one.n = rk::squash_steps(B, S, one.u.data(), one.v.data(), one.D.data(), one.active.data(), one.rows.data(), [&](uint32_t a) {
        rk::squash_row(B, S, h.data(), one.u.data(), one.v.data(), one.active.data(), a, 0, 1, one.D.data());
    });
    three.n = rk::squash_steps(B, S, three.u.data(), three.v.data(), three.D.data(), three.active.data(), three.rows.data(), [&](uint32_t a) {
        for (uint32_t th = 3; th-- > 0;) rk::squash_row(B, S, h.data(), three.u.data(), three.v.data(), three.active.data(), a, th, 3, three.D.data());
    });
    expect(one.n == three.n && memcmp(one.rows.data(), three.rows.data(), one.rows.size() * sizeof(rk::SquashMerge)) == 0, "row step dealt to three", B, S);

    uint32_t with_mass = 0;
    for (uint32_t s = 0; s < S; s++) with_mass += base.active[s];
    expect(one.n == (with_mass ? with_mass - 1 : 0), "n_merges", B, S);
    std::vector<uint32_t> size(S, 1);
    std::vector<char> gone(S, 0);
    bool rows_ok = true, fill_ok = true, dist_ok = true;
    for (uint32_t k = 0; k < one.n; k++) {
        const rk::SquashMerge &r = one.rows[k];
        rows_ok = rows_ok && r.a < r.b && r.b < S && r.reserved == 0;
        if (!rows_ok) break;
        rows_ok = rows_ok && base.active[r.a] && base.active[r.b] && !gone[r.a] && !gone[r.b];
        size[r.a] += size[r.b];
        gone[r.b] = 1;
        rows_ok = rows_ok && r.size == size[r.a];
        dist_ok = dist_ok && r.distance >= 0.0 && r.distance == r.distance;
    }
    for (uint32_t k = one.n; k + 1 < S; k++) {
        const rk::SquashMerge &r = one.rows[k];
        uint64_t d_bits;
        memcpy(&d_bits, &r.distance, 8);
        fill_ok = fill_ok && r.a == rk::SQUASH_NONE && r.b == rk::SQUASH_NONE && r.size == 0 && r.reserved == 0 && d_bits == 0;
    }
    expect(rows_ok, "rows", B, S);
    expect(fill_ok, "fillers", B, S);
    expect(dist_ok, "distances", B, S);
    if (one.n) expect(one.rows[one.n - 1].size == with_mass && one.rows[one.n - 1].a < S && !gone[one.rows[one.n - 1].a], "the last cluster holds every sample with mass", B, S);
    if (special) {
        uint64_t d_bits;
        memcpy(&d_bits, &one.rows[0].distance, 8);
        // (on one or two nodes other pairs are at +0.0 as well, and the tie rule takes a smaller a)
        expect(d_bits == 0 && (B < 300 || (one.rows[0].a == 2 && one.rows[0].b == 3 && one.rows[0].size == 2)), "identical samples merge first, at +0.0", B, S);
        bool none = true;
        for (uint32_t k = 0; k < one.n; k++) none = none && one.rows[k].a != 1 && one.rows[k].b != 1;
        expect(none, "the empty sample is in no row", B, S);
    }
    // the first merge again, by hand: the smallest entry of the matrix, the average of the two profiles, the row from them
    if (one.n) {
        const rk::SquashMerge &r = one.rows[0];
        bool first = r.distance == base.D[(uint64_t)r.a * S + r.b];
        for (uint32_t a = 0; a < S; a++)
            for (uint32_t b = a + 1; b < S; b++)
                if (base.active[a] && base.active[b]) {
                    const double d = base.D[(uint64_t)a * S + b];
                    first = first && (r.distance < d || (r.distance == d && (r.a < a || (r.a == a && r.b <= b))));
                }
        expect(first, "the first pick is the smallest entry, ties to the smaller a, then b", B, S);
    }
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    const uint32_t Bs[] = {1, 2, 300, 2049, 4097}, Ss[] = {2, 3, 6, 33};
    for (uint32_t B : Bs)
        for (uint32_t S : Ss)
            for (int kind = 0; kind < 3; kind++) {
                if (S == 33 && B > 2049) continue;  // (the many samples on the large tree add no path)
                one_shape(B, S, kind, false, rng);
                if (S >= 5) one_shape(B, S, kind, true, rng);
            }
    // every sample empty, and one sample with mass: no merge, fillers only (one_shape's masses are never empty, so by hand)
    {
        const uint32_t B = 7, S = 4;
        std::vector<double> u(S * B, 0.0), v(S * B, 0.0), D(S * S, 0.0);
        std::vector<uint8_t> active(S, 0);
        std::vector<rk::SquashMerge> rows(S - 1);
        uint32_t calls = 0;
        uint32_t n = rk::squash_steps(B, S, u.data(), v.data(), D.data(), active.data(), rows.data(), [&](uint32_t) { calls++; });
        expect(n == 0 && calls == 0 && rows[0].a == rk::SQUASH_NONE && rows[2].b == rk::SQUASH_NONE && rows[1].size == 0, "every sample empty");
        active[2] = 1;
        n = rk::squash_steps(B, S, u.data(), v.data(), D.data(), active.data(), rows.data(), [&](uint32_t) { calls++; });
        expect(n == 0 && calls == 0 && rows[0].a == rk::SQUASH_NONE, "one sample with mass");
    }
    printf("%llu checks, %llu wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}
