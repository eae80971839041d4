// The host twin of the edge statistics (rappas_amd/csrc/rk_edgestat_host.h over rk_samples_host.h and rk_samplemath.h) run on its
// own, without the library: a few small seeded shapes -- S on both sides of the 64 lanes, ids out of pre-order, one sample empty, two
// samples identical, a metadata column of few values, one that is not finite in the empty sample and one that is not finite in an
// active one --, the raw words and the finished table printed as integers and bit patterns so that tests/test_edgestat_host_cpp.py
// can hold them against tests/edgestat_ref.py word for word.  Also the program to build with the address and undefined-behaviour
// sanitizers.
#include "rk_edgestat_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

namespace {

int one_shape(uint32_t B, uint32_t S, uint32_t F, std::mt19937_64 &rng) {
    std::vector<int32_t> parent(B, -1);
    for (uint32_t x = 1; x < B; x++) parent[x] = (int32_t)(rng() % x);
    if (B > 1) {  // ids out of pre-order: swap the root's id with another node's
        const uint32_t y = 1 + (uint32_t)(rng() % (B - 1));
        for (uint32_t x = 0; x < B; x++) parent[x] = parent[x] == 0 ? (int32_t)y : parent[x] == (int32_t)y ? 0 : parent[x];
        std::swap(parent[0], parent[y]);
    }
    char msg[256];
    rk::TreeWalk w;
    if (rk::tree_walk("edgestat_host", B, parent.data(), nullptr, false, w, msg, sizeof(msg))) {
        printf("WRONG: %s\n", msg);
        return 1;
    }
    const uint64_t W = 2 * (uint64_t)B + 4;
    std::vector<uint64_t> m(S * W + 1, 0);
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t x = 0; x < B; x++) m[s * W + x] = rng() % 3 == 0 ? rng() % (1ull << 34) : 0;
    if (S > 3) {
        for (uint32_t x = 0; x < B; x++) m[1 * W + x] = 0;             // sample 1: empty
        for (uint32_t x = 0; x < B; x++) m[3 * W + x] = m[2 * W + x];  // sample 3: a copy of sample 2
    }
    std::vector<double> meta((size_t)F * S);
    for (uint32_t f = 0; f < F; f++)
        for (uint32_t s = 0; s < S; s++) meta[(size_t)f * S + s] = f % 2 ? (double)(rng() % 4) : (double)(int64_t)(rng() % 2000001) / 1000.0 - 1000.0;
    if (F > 1 && S > 3) meta[1 * S + 1] = std::numeric_limits<double>::quiet_NaN();  // in the empty sample: the column stays usable
    if (F > 2 && S > 3) meta[2 * S + 2] = std::numeric_limits<double>::infinity();   // in an active sample: unusable

    std::vector<uint64_t> clade((size_t)S * B);
    std::vector<uint8_t> active(S);
    uint32_t n = 0;
    for (uint32_t s = 0; s < S; s++) {
        rk::clade_masses_sample(w, parent.data(), m.data() + s * W, clade.data() + (size_t)s * B);
        n += active[s] = clade[(size_t)s * B + w.root] != 0;
    }
    std::vector<uint64_t> raw((size_t)rk::edgestat_out_words(B, F), 0);
    uint32_t info[2] = {n, 0};
    if (n) {
        rk::EdgestatColumns col;
        rk::edgestat_columns(S, n, F, active.data(), meta.data(), col, raw.data() + (size_t)B * rk::edgestat_row_words(F));
        info[1] = col.unusable;
        for (uint32_t th = 0; th < 3; th++) rk::edgestat_edges(B, S, W, w.root, n, F, active.data(), m.data(), clade.data(), col, th, 3, raw.data());
    }
    std::vector<double> table((size_t)B * (8 + 4 * F)), ftab(2 * (size_t)F + 1);
    rk::edgestat_finish(B, F, raw.data(), info, table.data(), ftab.data());

    printf("shape %u %u %u\nparent", B, S, F);
    for (uint32_t x = 0; x < B; x++) printf(" %d", parent[x]);
    printf("\n");
    for (uint32_t s = 0; s < S; s++) {
        printf("mass");
        for (uint32_t x = 0; x < B; x++) printf(" %" PRIu64, m[s * W + x]);
        printf("\n");
    }
    for (uint32_t f = 0; f < F; f++) {
        printf("meta");
        for (uint32_t s = 0; s < S; s++) printf(" %016" PRIx64, rk::edgestat_word(meta[(size_t)f * S + s]));
        printf("\n");
    }
    printf("info %u %u\nraw", info[0], info[1]);
    for (uint64_t v : raw) printf(" %016" PRIx64, v);
    printf("\ntable");
    for (double v : table) printf(" %016" PRIx64, rk::edgestat_word(v));
    printf("\nfeatures");
    for (size_t i = 0; i < 2 * (size_t)F; i++) printf(" %016" PRIx64, rk::edgestat_word(ftab[i]));
    printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    int wrong = one_shape(1, 1, 0, rng);
    wrong += one_shape(40, 5, 3, rng);
    wrong += one_shape(9, 64, 1, rng);
    wrong += one_shape(25, 65, 8, rng);
    wrong += one_shape(6, 200, 2, rng);
    printf("done %d wrong\n", wrong);
    return wrong ? 1 : 0;
}
