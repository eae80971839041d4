// The host side of the sample-level calls (rappas_amd/csrc/rk_samples_host.h: the tree checks and the walk, clade sums, KR
// distances) run on its own, so that tests/test_samples_host_cpp.py can build it with the address and undefined-behaviour sanitizers:
// the refused trees, then seeded trees of B = 1, 2, 999, 2047, 2048, 2049, 4097 nodes (random with shuffled ids, caterpillar, star)
// with S = 1, 2, 3, 65 samples, an empty sample, two identical ones and 2^62 on one branch.  The clade sums are held against a
// naive walk up from every node, the matrix against its stated properties and against rows computed in another split.
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

struct Shape {
    std::vector<int32_t> parent;
    std::vector<float> bl;
};

Shape make_tree(uint32_t B, int kind, std::mt19937_64 &rng) {
    Shape t;
    t.parent.assign(B, -1);
    t.bl.resize(B);
    for (uint32_t x = 1; x < B; x++) t.parent[x] = kind == 1 ? (int32_t)(x - 1) : kind == 2 ? 0 : (int32_t)(rng() % x);
    for (uint32_t x = 0; x < B; x++) t.bl[x] = (float)(rng() % 4096) / 1024.0f;
    if (kind == 0) {  // ids out of pre-order: relabel at random
        std::vector<uint32_t> perm(B);
        for (uint32_t i = 0; i < B; i++) perm[i] = i;
        for (uint32_t i = B; i > 1; i--) std::swap(perm[i - 1], perm[rng() % i]);
        Shape s;
        s.parent.assign(B, -1);
        s.bl.resize(B);
        for (uint32_t x = 0; x < B; x++) {
            s.parent[perm[x]] = t.parent[x] < 0 ? -1 : (int32_t)perm[(uint32_t)t.parent[x]];
            s.bl[perm[x]] = t.bl[x];
        }
        return s;
    }
    return t;
}

void bad_trees() {
    char msg[256];
    rk::TreeWalk w;
    auto refused = [&](std::vector<int32_t> p, std::vector<float> b, const char *what) {
        msg[0] = 0;
        const int rc = rk::tree_walk("test", (uint32_t)p.size(), p.data(), b.data(), true, w, msg, sizeof(msg));
        expect(rc != 0 && msg[0] != 0 && w.node_at.empty(), what);
    };
    refused({1, 2, 0}, {1, 1, 1}, "no root");
    refused({-1, -1, 0}, {1, 1, 1}, "two roots");
    refused({-1, 3, 0}, {1, 1, 1}, "parent beyond B");
    refused({-1, -2, 0}, {1, 1, 1}, "parent below -1");
    refused({-1, 1, 0}, {1, 1, 1}, "own parent");
    refused({-1, 2, 1, 0}, {1, 1, 1, 1}, "cycle");
    refused({-1, 0, 0}, {0, -1, 1}, "negative length");
    refused({-1, 0, 0}, {0, 1, NAN}, "NaN length");
    refused({-1, 0, 0}, {0, INFINITY, 1}, "infinite length");
    expect(rk::tree_walk("test", 0, nullptr, nullptr, true, w, msg, sizeof(msg)) != 0, "B = 0");
    expect(rk::tree_walk("test", 65536, nullptr, nullptr, true, w, msg, sizeof(msg)) != 0, "B = 65536");
    std::vector<int32_t> p{-1, 0};
    expect(rk::tree_walk("test", 2, nullptr, nullptr, true, w, msg, sizeof(msg)) != 0, "null parent");
    expect(rk::tree_walk("test", 2, p.data(), nullptr, true, w, msg, sizeof(msg)) != 0, "null lengths");
    expect(rk::tree_walk("test", 2, p.data(), nullptr, false, w, msg, sizeof(msg)) == 0 && w.node_at.size() == 2, "lengths not asked for");
}

void one_shape(uint32_t B, uint32_t S, int kind, std::mt19937_64 &rng) {
    const Shape t = make_tree(B, kind, rng);
    char msg[256];
    rk::TreeWalk w;
    if (rk::tree_walk("test", B, t.parent.data(), t.bl.data(), true, w, msg, sizeof(msg))) {
        expect(false, msg, B, S);
        return;
    }
    // the walk: a permutation, parents before children, intervals nested
    std::vector<char> seen(B, 0);
    bool walk_ok = w.pre[w.root] == 0 && w.size[w.root] == B;
    for (uint32_t p = 0; p < B; p++) {
        const uint32_t x = w.node_at[p];
        walk_ok = walk_ok && x < B && !seen[x] && w.pre[x] == p;
        if (x < B) seen[x] = 1;
        if (x < B && x != w.root) {
            const uint32_t up = (uint32_t)t.parent[x];
            walk_ok = walk_ok && w.pre[up] < p && p + w.size[x] <= w.pre[up] + w.size[up];
        }
    }
    expect(walk_ok, "walk", B, S);

    const uint64_t W = 2 * (uint64_t)B + 4;
    std::vector<uint64_t> m(S * W + 1, 0);
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t x = 0; x < B; x++) m[s * W + x] = rng() % 3 == 0 ? rng() % (1ull << 34) : 0;
    for (uint32_t s = 0; s < S; s++) m[s * W + rng() % B] += 1u << 30;  // no sample empty by chance
    if (S >= 5) {
        for (uint32_t x = 0; x < B; x++) { m[1 * W + x] = 0; m[3 * W + x] = m[2 * W + x]; m[4 * W + x] = 0; }
        m[4 * W + B / 2] = 1ull << 62;
        m[4 * W + B - 1] += 12345;
    }
    std::vector<uint64_t> clade(S * (uint64_t)B), naive(B);
    std::vector<double> u(S * (uint64_t)B), v(S * (uint64_t)B), h(B);
    for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(t.bl.data(), x, w.root);
    bool clade_ok = true;
    for (uint32_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, t.parent.data(), m.data() + s * W, clade.data() + (uint64_t)s * B);
        if (s < 2 && B <= 4097 && kind != 1) {  // every node adds itself to all its ancestors (a caterpillar's B^2 / 2 steps are left out)
            std::fill(naive.begin(), naive.end(), 0);
            for (uint32_t x = 0; x < B; x++)
                for (int32_t y = (int32_t)x; y >= 0; y = t.parent[(uint32_t)y]) naive[(uint32_t)y] += m[s * W + x];
            clade_ok = clade_ok && memcmp(naive.data(), clade.data() + (uint64_t)s * B, B * 8) == 0;
        }
        rk::kr_profiles_sample(B, w.root, m.data() + s * W, clade.data() + (uint64_t)s * B, u.data() + (uint64_t)s * B, v.data() + (uint64_t)s * B);
    }
    expect(clade_ok, "clade sums", B, S);
    std::vector<double> D((uint64_t)S * S, -1.0), D3((uint64_t)S * S, -1.0);
    rk::kr_rows(B, S, h.data(), u.data(), v.data(), 0, 1, D.data());
    for (uint32_t th = 0; th < 3; th++) rk::kr_rows(B, S, h.data(), u.data(), v.data(), th, 3, D3.data());
    expect(memcmp(D.data(), D3.data(), D.size() * 8) == 0, "rows dealt to three", B, S);
    bool sym = true, diag = true, special = true;
    for (uint32_t s = 0; s < S; s++) {
        const bool empty = S >= 5 && s == 1;
        uint64_t d_bits;
        memcpy(&d_bits, &D[(uint64_t)s * S + s], 8);
        diag = diag && (empty ? D[(uint64_t)s * S + s] != D[(uint64_t)s * S + s] : d_bits == 0);
        for (uint32_t q = 0; q < S; q++) {
            sym = sym && memcmp(&D[(uint64_t)s * S + q], &D[(uint64_t)q * S + s], 8) == 0;
            const double d = D[(uint64_t)s * S + q];
            if (S >= 5) special = special && ((s == 1 || q == 1) ? d != d : d >= 0.0);
        }
    }
    if (S >= 5) {
        uint64_t b23;
        memcpy(&b23, &D[2 * (uint64_t)S + 3], 8);
        special = special && b23 == 0;
    }
    expect(sym, "bitwise symmetric", B, S);
    expect(diag, "diagonal", B, S);
    expect(special, "empty, identical and huge samples", B, S);
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    bad_trees();
    const uint32_t Bs[] = {1, 2, 999, 2047, 2048, 2049, 4097}, Ss[] = {1, 2, 3, 65};
    for (uint32_t B : Bs)
        for (uint32_t S : Ss)
            for (int kind = 0; kind < 3; kind++) {
                if (S == 65 && B > 2049) continue;  // (the large matrix on the large tree adds no path)
                one_shape(B, S, kind, rng);
            }
    printf("%llu checks, %llu wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}
