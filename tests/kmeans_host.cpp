// The host twin of the phylogenetic k-means (rappas_amd/csrc/rk_samples_host.h: kmeans_seed, kmeans_distances, kmeans_assign,
// kmeans_update, kmeans_rounds) run on its own, so that tests/test_kmeans_host_cpp.py can build it with the address and
// undefined-behaviour sanitizers: seeded trees of B = 1, 2, 300, 2049, 4097 nodes (random with shuffled ids, caterpillar, star) with
// S = 2, 3, 6, 33, 300 samples and k = 1, 3, 7 clusters, an empty sample, two identical ones and 2^62 on one branch.  A run is held
// against what the definition promises of any run, against a second run whose steps are dealt to three and to two, and -- where it
// converged -- against the distances and the means recomputed from its own centroids and assignment.
#include "rk_samples_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

unsigned long long checked = 0, wrong = 0;
void expect(bool ok, const char *what, unsigned a = 0, unsigned b = 0, unsigned c = 0) {
    checked++;
    if (!ok) {
        wrong++;
        printf("WRONG: %s (%u, %u, %u)\n", what, a, b, c);
    }
}

uint64_t bits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

struct Input {
    uint32_t B, S;
    std::vector<double> h, u, v;
    std::vector<uint8_t> active;
    uint32_t n_active = 0;
};

struct Run {
    std::vector<uint32_t> assign, sizes, seeds;
    std::vector<double> dist, within, centroids, cu, cv;
    uint32_t info[4] = {9, 9, 9, 9};
};

// what rk_kmeans_host does behind its argument checks, the two steps dealt to `dt` and `ut` callers in descending order
Run run(const Input &in, uint32_t k, uint32_t max_rounds, uint32_t dt, uint32_t ut) {
    const uint32_t B = in.B, S = in.S, k_eff = k < in.n_active ? k : in.n_active;
    Run r;
    r.assign.assign(S, 7);
    r.dist.assign(S, 7.0);
    r.sizes.assign(k, 7);
    r.within.assign(k, 7.0);
    r.centroids.assign((uint64_t)k * 2 * B, 7.0);
    r.cu.assign((uint64_t)k * B, -1.0);
    r.cv.assign((uint64_t)k * B, -1.0);
    r.seeds.assign(k_eff, rk::KMEANS_NONE);
    std::vector<double> Dc((uint64_t)k * S, -1.0);
    const rk::KmeansOut o{r.assign.data(), r.dist.data(), r.sizes.data(), r.within.data(), r.info, r.centroids.data()};
    if (!in.n_active) {
        rk::kmeans_fill(B, S, k, k_eff, 0, 0, o);
        return r;
    }
    auto dist_step = [&](uint32_t j_lo, uint32_t j_hi) {
        for (uint32_t th = dt; th-- > 0;)
            rk::kmeans_distances(B, S, in.h.data(), in.u.data(), in.v.data(), in.active.data(), r.cu.data(), r.cv.data(), j_lo, j_hi, th, dt, Dc.data());
    };
    auto update_step = [&]() {
        for (uint32_t th = ut; th-- > 0;) rk::kmeans_update(B, S, k_eff, in.u.data(), in.v.data(), r.assign.data(), th, ut, r.cu.data(), r.cv.data());
    };
    rk::kmeans_seed(B, S, k_eff, in.u.data(), in.v.data(), in.active.data(), r.cu.data(), r.cv.data(), Dc.data(), r.seeds.data(), dist_step);
    rk::kmeans_rounds(B, S, k, k_eff, in.n_active, max_rounds, in.active.data(), r.cu.data(), r.cv.data(), Dc.data(), o, dist_step, update_step);
    return r;
}

bool same(const Run &a, const Run &b) {
    return a.assign == b.assign && a.sizes == b.sizes && a.seeds == b.seeds && memcmp(a.info, b.info, 16) == 0 &&
           memcmp(a.dist.data(), b.dist.data(), a.dist.size() * 8) == 0 && memcmp(a.within.data(), b.within.data(), a.within.size() * 8) == 0 &&
           memcmp(a.centroids.data(), b.centroids.data(), a.centroids.size() * 8) == 0;
}

void one_shape(uint32_t B, uint32_t S, uint32_t k, int kind, bool special, std::mt19937_64 &rng) {
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
        expect(false, msg, B, S, k);
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
    Input in;
    in.B = B;
    in.S = S;
    in.h.resize(B);
    in.u.resize(S * (uint64_t)B);
    in.v.resize(S * (uint64_t)B);
    in.active.resize(S);
    std::vector<uint64_t> clade(B);
    for (uint32_t x = 0; x < B; x++) in.h[x] = rk::kr_half_length(bl.data(), x, w.root);
    for (uint32_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, parent.data(), m.data() + s * W, clade.data());
        rk::kr_profiles_sample(B, w.root, m.data() + s * W, clade.data(), in.u.data() + (uint64_t)s * B, in.v.data() + (uint64_t)s * B);
        in.n_active += in.active[s] = clade[w.root] != 0;
    }
    const uint32_t k_eff = k < in.n_active ? k : in.n_active;
    const Run one = run(in, k, 100, 1, 1), dealt = run(in, k, 100, 3, 2), cut = run(in, k, 1, 1, 1);
    expect(same(one, dealt), "the steps dealt to three and to two", B, S, k);

    expect(one.info[0] == k_eff && one.info[1] == in.n_active && one.info[2] >= 2 && one.info[2] <= 100 && one.info[3] <= 1, "info", B, S, k);
    expect(cut.info[2] == 1 && cut.info[3] == 0 && cut.seeds == one.seeds, "one round: not converged, the same seeds", B, S, k);
    bool seeds_ok = true, assign_ok = true, rows_ok = true;
    for (uint32_t j = 0; j < k_eff; j++) {
        seeds_ok = seeds_ok && one.seeds[j] < S && in.active[one.seeds[j]];
        for (uint32_t i = 0; i < j; i++) seeds_ok = seeds_ok && one.seeds[i] != one.seeds[j];
    }
    uint32_t first = 0;
    while (first < S && !in.active[first]) first++;
    expect(seeds_ok && one.seeds[0] == first, "seeds: active, distinct, the first the smallest active sample", B, S, k);
    std::vector<uint32_t> size(k, 0);
    std::vector<double> within(k, 0.0);
    for (uint32_t s = 0; s < S; s++) {
        if (!in.active[s]) {
            assign_ok = assign_ok && one.assign[s] == rk::KMEANS_NONE && bits(one.dist[s]) == 0;
            continue;
        }
        assign_ok = assign_ok && one.assign[s] < k_eff && one.dist[s] >= 0.0;
        if (!assign_ok) break;
        size[one.assign[s]]++;
        within[one.assign[s]] = within[one.assign[s]] + one.dist[s];
    }
    expect(assign_ok, "assign and dist", B, S, k);
    for (uint32_t j = 0; j < k; j++) {
        rows_ok = rows_ok && one.sizes[j] == size[j] && bits(one.within[j]) == bits(within[j]);
        if (j >= k_eff)
            for (uint64_t i = 0; i < 2 * (uint64_t)B; i++) rows_ok = rows_ok && bits(one.centroids[(uint64_t)j * 2 * B + i]) == 0;
    }
    expect(rows_ok, "sizes, within and the rows behind k_eff", B, S, k);
    if (one.info[3] == 1 && assign_ok) {
        // converged: the centroids are the means of the final clusters, and every sample sits with its nearest centroid at the distance
        // the run reports
        bool near_ok = true, mean_ok = true;
        for (uint32_t s = 0; s < S && near_ok; s++) {
            if (!in.active[s]) continue;
            uint32_t best = 0;
            double bd = 0.0;
            for (uint32_t j = 0; j < k_eff; j++) {
                const double d = rk::kr_pair(B, in.h.data(), one.centroids.data() + (uint64_t)j * 2 * B, one.centroids.data() + ((uint64_t)j * 2 + 1) * B,
                                             in.u.data() + (uint64_t)s * B, in.v.data() + (uint64_t)s * B);
                if (j == 0 || d < bd) {
                    bd = d;
                    best = j;
                }
            }
            near_ok = best == one.assign[s] && bits(bd) == bits(one.dist[s]);
        }
        expect(near_ok, "converged: every sample with its nearest centroid", B, S, k);
        for (uint32_t j = 0; j < k_eff && mean_ok; j++) {
            if (!size[j]) continue;
            for (uint32_t x = 0; x < B && mean_ok; x += 1 + B / 16) {  // a sample of the nodes
                double su = 0.0, sv = 0.0;
                uint32_t n = 0;
                for (uint32_t g0 = 0; g0 < S; g0 += rk::KMEANS_GROUP) {
                    double pu = 0.0, pv = 0.0;
                    uint32_t in_group = 0;
                    for (uint32_t s = g0; s < S && s < g0 + rk::KMEANS_GROUP; s++)
                        if (one.assign[s] == j) {
                            pu = pu + in.u[(uint64_t)s * B + x];
                            pv = pv + in.v[(uint64_t)s * B + x];
                            in_group++;
                        }
                    if (!in_group) continue;
                    su = n ? su + pu : pu;
                    sv = n ? sv + pv : pv;
                    n += in_group;
                }
                mean_ok = bits(one.centroids[(uint64_t)j * 2 * B + x]) == bits(su / (double)n) && bits(one.centroids[((uint64_t)j * 2 + 1) * B + x]) == bits(sv / (double)n);
            }
        }
        expect(mean_ok, "converged: a centroid is the ordered mean of its members", B, S, k);
    }
    if (special) {
        expect(one.assign[1] == rk::KMEANS_NONE && one.info[1] == S - 1, "the empty sample is in no cluster", B, S, k);
        expect(one.assign[2] == one.assign[3] && bits(one.dist[2]) == bits(one.dist[3]), "identical samples: one cluster, the same distance", B, S, k);
    }
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    const uint32_t Bs[] = {1, 2, 300, 2049, 4097}, Ss[] = {2, 3, 6, 33, 300}, ks[] = {1, 3, 7};
    for (uint32_t B : Bs)
        for (uint32_t S : Ss)
            for (uint32_t k : ks)
                for (int kind = 0; kind < 3; kind++) {
                    if ((S == 33 && B > 2049) || (S == 300 && (B > 300 || kind != 0))) continue;  // (the many samples on the large trees add no path)
                    one_shape(B, S, k, kind, false, rng);
                    if (S >= 5 && k == 3) one_shape(B, S, k, kind, true, rng);
                }
    // every sample empty: fillers
    {
        Input in;
        in.B = 7;
        in.S = 4;
        in.h.assign(7, 1.0);
        in.u.assign(28, 0.0);
        in.v.assign(28, 0.0);
        in.active.assign(4, 0);
        const Run r = run(in, 3, 10, 1, 1);
        bool ok = r.info[0] == 0 && r.info[1] == 0 && r.info[2] == 0 && r.info[3] == 1;
        for (uint32_t s = 0; s < 4; s++) ok = ok && r.assign[s] == rk::KMEANS_NONE && bits(r.dist[s]) == 0;
        for (uint32_t j = 0; j < 3; j++) ok = ok && r.sizes[j] == 0 && bits(r.within[j]) == 0;
        for (double c : r.centroids) ok = ok && bits(c) == 0;
        expect(ok, "every sample empty");
    }
    printf("%llu checks, %llu wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}
