// The host twin of the per-sample diversity measures (rappas_amd/csrc/rk_samples_host.h: diversity_sample over rk_divmath.h) run on
// its own, without the library: two small seeded shapes -- B = 300 (one chunk, lanes with one and with two nodes) and B = 2100 (two
// chunks), ids out of pre-order, one sample empty, one with all its mass on one branch --, printed as integers and bit patterns so
// that tests/test_diversity_host_cpp.py can hold the rows against tests/diversity_ref.py word for word.  Also the program to build
// with the address and undefined-behaviour sanitizers.
#include "rk_samples_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

uint64_t bits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

int one_shape(uint32_t B, uint32_t S, const std::vector<double> &theta, std::mt19937_64 &rng) {
    std::vector<int32_t> parent(B, -1);
    std::vector<float> bl(B);
    for (uint32_t x = 1; x < B; x++) parent[x] = (int32_t)(rng() % x);
    for (uint32_t x = 0; x < B; x++) bl[x] = (float)(rng() % 4096) / 1024.0f;
    if (B > 1) {  // ids out of pre-order: swap the root's id with another node's
        const uint32_t y = 1 + (uint32_t)(rng() % (B - 1));
        for (uint32_t x = 0; x < B; x++) parent[x] = parent[x] == 0 ? (int32_t)y : parent[x] == (int32_t)y ? 0 : parent[x];
        std::swap(parent[0], parent[y]);
        std::swap(bl[0], bl[y]);
    }
    char msg[256];
    rk::TreeWalk w;
    if (rk::tree_walk("diversity_host", B, parent.data(), bl.data(), true, w, msg, sizeof(msg))) {
        printf("WRONG: %s\n", msg);
        return 1;
    }
    if (rk::diversity_theta_args("diversity_host", (uint32_t)theta.size(), theta.data(), msg, sizeof(msg))) {
        printf("WRONG: %s\n", msg);
        return 1;
    }
    const uint64_t W = 2 * (uint64_t)B + 4;
    std::vector<uint64_t> m(S * W + 1, 0);
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t x = 0; x < B; x++) m[s * W + x] = rng() % 3 == 0 ? rng() % (1ull << 34) : 0;
    for (uint32_t x = 0; x < B; x++) m[1 * W + x] = 0;                      // sample 1: empty
    for (uint32_t x = 0; x < B; x++) m[2 * W + x] = x == B / 2 ? 1ull << 62 : 0;  // sample 2: everything on one branch
    std::vector<double> h(B);
    for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(bl.data(), x, w.root);
    const uint32_t C = rk::DIVERSITY_FIXED + 2 * (uint32_t)theta.size();
    std::vector<uint64_t> clade(B);
    std::vector<double> row(C);
    printf("shape %u %u %zu\nparent", B, S, theta.size());
    for (uint32_t x = 0; x < B; x++) printf(" %d", parent[x]);
    printf("\nbranch_len");
    for (uint32_t x = 0; x < B; x++) printf(" %a", (double)bl[x]);
    printf("\ntheta");
    for (double t : theta) printf(" %a", t);
    printf("\n");
    for (uint32_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, parent.data(), m.data() + s * W, clade.data());
        rk::diversity_sample(B, w.root, m.data() + s * W, clade.data(), h.data(), (uint32_t)theta.size(), theta.data(), row.data());
        printf("mass");
        for (uint32_t x = 0; x < B; x++) printf(" %" PRIu64, m[s * W + x]);
        printf("\nrow");
        for (uint32_t i = 0; i < C; i++) printf(" %016" PRIx64, bits(row[i]));
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    int wrong = one_shape(300, 4, {0.0, 0.25, 1.0}, rng);
    wrong += one_shape(2100, 3, {}, rng);
    wrong += one_shape(2100, 3, {2.0, 0.5, 8.0, 3.25, 1.0, 0.0, 7.5, 0.125}, rng);
    printf("done %d wrong\n", wrong);
    return wrong ? 1 : 0;
}
