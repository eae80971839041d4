// The host twin of the edge PCA (rappas_amd/csrc/rk_samples_host.h: lane_sum, epca_centre, epca_gram_rows, epca_iterate, epca_finish)
// run on its own, so that tests/test_epca_host_cpp.py can build it with the address and undefined-behaviour sanitizers: seeded trees
// of B = 1, 2, 300, 2049, 4097 nodes (random with shuffled ids, caterpillar, star) with S = 2, 3, 6, 65, 130 samples, an empty sample,
// two identical ones and 2^62 on one branch.  The raw output is held against what the definition promises of any run, against a
// second run whose nodes and rows are dealt to three, and against sums recomputed in another order.
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

uint64_t bits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

struct Run {
    std::vector<double> xc, G, raw;
    std::vector<uint8_t> active;
    uint32_t n = 0, k_eff = 0;
};

// what rk_epca_host does behind its checks, the nodes and the rows dealt to `deal`
void run(uint32_t B, uint32_t S, uint32_t k, uint32_t iters, const rk::TreeWalk &w, const std::vector<int32_t> &parent, const std::vector<uint64_t> &m, uint32_t deal, Run &r) {
    const uint64_t W = 2 * (uint64_t)B + 4;
    std::vector<uint64_t> clade(S * (uint64_t)B);
    std::vector<double> v(S * (uint64_t)B), cols(2 * (uint64_t)k * S);
    r.xc.assign(S * (uint64_t)B, 0.0);
    r.G.assign((uint64_t)S * S, -1.0);
    r.raw.assign(rk::epca_out_doubles(B, S, k), 0.0);
    r.active.assign(S, 0);
    r.n = 0;
    for (uint64_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, parent.data(), m.data() + s * W, clade.data() + s * B);
        rk::kr_profiles_sample(B, w.root, m.data() + s * W, clade.data() + s * B, r.xc.data() + s * B, v.data() + s * B);
        r.n += r.active[s] = clade[s * B + w.root] != 0;
    }
    r.k_eff = r.n < 2 ? 0u : std::min(k, r.n - 1);
    if (!r.k_eff) return;
    for (uint32_t th = 0; th < deal; th++) rk::epca_centre(B, S, w.root, r.active.data(), r.n, r.xc.data(), v.data(), th, deal, r.xc.data());
    for (uint32_t th = deal; th-- > 0;) rk::epca_gram_rows(B, S, r.xc.data(), th, deal, r.G.data());
    rk::epca_iterate(B, S, k, r.k_eff, iters, r.G.data(), r.xc.data(), cols.data(), r.raw.data());
}

void one_shape(uint32_t B, uint32_t S, uint32_t k, uint32_t iters, int kind, int special, std::mt19937_64 &rng) {
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
    if (special == 1) {  // S >= 5: sample 1 empty, 3 a copy of 2, 4 with 2^62 on one branch
        for (uint32_t x = 0; x < B; x++) { m[1 * W + x] = 0; m[3 * W + x] = m[2 * W + x]; m[4 * W + x] = 0; }
        m[4 * W + B / 2] = 1ull << 62;
        m[4 * W + B - 1] += 12345;
    }
    if (special >= 2) {  // nobody holds mass (2), one sample does (3)
        std::fill(m.begin(), m.end(), 0);
        if (special == 3) m[(S - 1) * W + B / 2] = 99;
    }
    Run a, b;
    run(B, S, k, iters, w, parent, m, 1, a);
    run(B, S, k, iters, w, parent, m, 3, b);
    const uint32_t n_want = special == 1 ? S - 1 : special == 2 ? 0 : special == 3 ? 1 : S;
    expect(a.n == n_want && b.n == n_want, "the number of active samples", a.n, n_want);
    expect(a.k_eff == (n_want < 2 ? 0u : std::min(k, n_want - 1)) && b.k_eff == a.k_eff, "k_eff = min(k, n - 1)", a.k_eff, k);
    bool same = a.raw.size() == b.raw.size();
    for (size_t i = 0; same && i < a.raw.size(); i++) same = bits(a.raw[i]) == bits(b.raw[i]);
    expect(same, "the same bits however nodes and rows are dealt", B, S);
    const double *raw = a.raw.data(), *lambda = raw + 1, *nn = lambda + k, *rr = nn + k, *q = rr + k, *wl = q + (uint64_t)k * S;
    if (!a.k_eff) {
        bool zero = true;
        for (double d : a.raw) zero = zero && bits(d) == 0;
        expect(zero, "k_eff == 0: every output double is +0.0", B, S);
        return;
    }
    // G: bitwise symmetric, +0.0 rows of the samples without mass, the trace by the lane rule and (loosely) by a plain sum
    bool sym = true, dead = true;
    double plain = 0.0;
    for (uint64_t s = 0; s < S; s++) {
        plain += a.G[s * S + s];
        for (uint64_t t = 0; t < S; t++) {
            sym = sym && bits(a.G[s * S + t]) == bits(a.G[t * S + s]);
            if (!a.active[s]) dead = dead && bits(a.G[s * S + t]) == 0;
        }
    }
    expect(sym, "G is bitwise symmetric", B, S);
    expect(dead, "the rows of G of samples without mass are +0.0", B, S);
    expect(std::fabs(raw[0] - plain) <= 1e-12 * std::fabs(plain), "trace", B, S);
    // centring: the entries of every node add up to nothing, up to the roundings of the lane-rule sum behind the mean ((S / 64 + 64)
    // adds on sums of at most S, each 2^-53 relative), of the mean and of the S differences
    double worst = 0.0;
    for (uint64_t x = 0; x < B; x++) {
        double sum = 0.0;
        for (uint64_t s = 0; s < S; s++) sum += a.xc[s * B + x];
        worst = std::max(worst, std::fabs(sum));
    }
    expect(worst <= (S / 64.0 + 68.0) * S * 1.2e-16, "the centred rows add up to zero", B, S);
    if (special == 1) {
        bool twin = true;
        for (uint32_t j = 0; j < a.k_eff; j++) twin = twin && bits(q[j * (uint64_t)S + 2]) == bits(q[j * (uint64_t)S + 3]) && q[j * (uint64_t)S + 1] == 0.0;
        expect(twin, "identical samples have identical q entries, the empty one zeros", B, S);
    }
    for (uint32_t j = 0; j < k; j++) {
        const double *qj = q + j * (uint64_t)S;
        if (j >= a.k_eff) {
            bool zero = bits(lambda[j]) == 0 && bits(nn[j]) == 0 && bits(rr[j]) == 0;
            for (uint32_t s = 0; s < S; s++) zero = zero && bits(qj[s]) == 0;
            for (uint32_t x = 0; x < B; x++) zero = zero && bits(wl[j * (uint64_t)B + x]) == 0;
            expect(zero, "a component >= k_eff is +0.0", j, a.k_eff);
            continue;
        }
        if (nn[j] == 0.0) {
            expect(bits(lambda[j]) == 0 && bits(rr[j]) == 0, "a zero column has lambda = rr = +0.0", j, S);
            continue;
        }
        // the scaling of step 6 (later columns' projections only touch later columns)
        uint32_t i = 0;
        for (uint32_t s = 1; s < S; s++)
            if (std::fabs(qj[s]) > std::fabs(qj[i])) i = s;
        expect(bits(qj[i]) == bits(1.0), "the largest element of a column is exactly +1.0", j, i);
        expect(nn[j] >= 1.0 && nn[j] <= (double)S, "1 <= nn <= S", j, S);
        expect(rr[j] >= 0.0 && lambda[j] >= -1e-12 * raw[0] && lambda[j] <= raw[0] * (1 + 1e-12), "0 <= lambda <= trace, rr >= 0", j, S);
        // (how orthogonal two columns come out depends on how parallel they went into the one pass of Gram-Schmidt -- after few
        // iterations on a matrix with one large eigenvalue, nearly -- so no bound is held here: tests/test_epca_host.py holds one on a
        // converged run)
        // lambda and the loadings by plain sums
        double num = 0.0, wmax = 0.0;
        for (uint64_t s = 0; s < S; s++) {
            double z = 0.0;
            for (uint64_t t = 0; t < S; t++) z += a.G[s * S + t] * qj[t];
            num += qj[s] * z;
        }
        expect(std::fabs(num / nn[j] - lambda[j]) <= 1e-11 * raw[0], "lambda is the Rayleigh quotient", j, S);
        for (uint64_t x = 0; x < B; x++) {
            double d = 0.0;
            for (uint64_t s = 0; s < S; s++) d += a.xc[s * B + x] * qj[s];
            wmax = std::max(wmax, std::fabs(d - wl[j * (uint64_t)B + x]));
        }
        expect(wmax <= 1e-12 * S, "w = Xc q", j, S);
    }
    // the finish: zero rule, eigenvalue = lambda, projections scaled q
    std::vector<double> ev(k), share(k), res(k), proj((uint64_t)S * k), load((uint64_t)B * k);
    rk::epca_finish(B, S, k, raw, ev.data(), share.data(), res.data(), proj.data(), load.data());
    bool fin = true;
    for (uint32_t j = 0; j < k; j++) {
        const bool on = lambda[j] > 0.0 && nn[j] != 0.0;
        fin = fin && bits(ev[j]) == bits(on ? lambda[j] : 0.0) && res[j] >= 0.0 && share[j] >= 0.0 && share[j] <= 1 + 1e-12;
        for (uint32_t s = 0; s < S; s++) fin = fin && (on ? proj[(uint64_t)s * k + j] == q[j * (uint64_t)S + s] * std::sqrt(lambda[j] / nn[j]) : bits(proj[(uint64_t)s * k + j]) == 0);
        for (uint32_t x = 0; x < B; x++) fin = fin && (on || bits(load[(uint64_t)x * k + j]) == 0) && load[(uint64_t)x * k + j] == load[(uint64_t)x * k + j];
    }
    expect(fin, "the finish", B, S);
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    for (uint32_t B : {1u, 2u, 300u, 2049u, 4097u})
        for (int kind = 0; kind < 3; kind++)
            for (uint32_t S : {2u, 3u, 6u, 65u, 130u}) {
                if (B > 2049 && S > 6) continue;  // (the sanitizer build stays quick)
                const uint32_t k = 1 + (uint32_t)(rng() % 8), iters = 1 + (uint32_t)(rng() % 4);
                one_shape(B, S, k, iters, kind, 0, rng);
                if (S >= 5) one_shape(B, S, 8, 12, kind, 1, rng);
            }
    for (int special = 2; special <= 3; special++) one_shape(40, 5, 4, 3, 0, special, rng);
    one_shape(300, 9, 2, 128, 0, 0, rng);
    printf("%llu checks, %llu wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}
