// The launch plan of windowed trees with short rows (rappas_amd/csrc/rk_plan.h) swept over a dense grid of its inputs: every class of
// batch the re-tiling pre-pass can find on the device must be placed by some kernel, and no kernel may be launched for records it cannot
// hold.  Built and run by tests/test_plan_grid.py; no GPU, no HIP.
//   plan_grid                      sweep the grid; prints one line per violated rule (with the region of inputs where it fails), exit 1
//   plan_grid case BITS K WPR LENS FIXED_LEN UNITS_PER_CODE ENTRIES_PER_KEY N_BRANCHES HASH_CAPABLE STREAM VERDICT FIRST_OK MARKED_LIST
//                                  the plan of one input, as key=value lines
#include "rk_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace rk_plan;

namespace {

struct Input {
    uint32_t bits, k, wpr;
    bool lens;
    uint32_t fixed_len;
    double upc, epk;
    In in;
};

In make_in(const Input &x, const ReadShape &rs) {
    In in = x.in;
    in.est_units = rs.est_units;
    in.full_hit_entries = full_hit_entries(rs.max_syms, x.k, 1000000, (uint64_t)(x.epk * 1000000.0));
    in.words_per_read = x.wpr;
    in.one_batch = rs.one_batch;
    return in;
}

// the device's side of the contract (rk_kernels.hip: batch_is_mine, takes_only_marked)
bool admits(const Launch &l, bool verdict, int c) { return l.run && (!l.only_if || !verdict || ((l.only_if >> c) & 1u)); }
bool wide_takes_all(const Plan &p, bool verdict, int c) { return !p.only_marked || (verdict && p.marked_if && !((p.marked_if >> c) & 1u)); }

struct Region {
    uint64_t count = 0;
    uint32_t nb_lo = ~0u, nb_hi = 0, wpr_lo = ~0u, wpr_hi = 0;
    double est_lo = 1e300, est_hi = -1.0;
    uint32_t classes = 0;
    std::string example;
};
std::map<std::string, Region> violations;

void flag(const char *rule, const Input &x, const In &in, int c) {
    Region &r = violations[rule];
    if (!r.count) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s k=%u %s words=%u n_branches=%u est_units=%.1f full_hit_entries=%.0f hash_capable=%d stream=%d verdict=%d first_ok=%d marked_list=%d "
                 "knobs{always=%d big=%d small=%d clade_small=%d wstream_always=%d no_wstream=%d slack=%u} class=%d",
                 x.bits == 5 ? "amino acids" : "DNA", x.k, x.lens ? "ragged" : ("fixed_len=" + std::to_string(x.fixed_len)).c_str(), x.wpr, in.n_branches,
                 in.est_units, in.full_hit_entries, in.hash_capable, in.stream, in.verdict, in.first_ok, in.marked_list, in.knobs.hash_always,
                 in.knobs.hash_big_table, in.knobs.hash_small_table, in.knobs.hash_clade_small, in.knobs.wstream_always, in.knobs.no_wstream,
                 in.knobs.key_slack, c);
        r.example = buf;
    }
    r.count++;
    r.nb_lo = std::min(r.nb_lo, in.n_branches); r.nb_hi = std::max(r.nb_hi, in.n_branches);
    r.wpr_lo = std::min(r.wpr_lo, x.wpr); r.wpr_hi = std::max(r.wpr_hi, x.wpr);
    r.est_lo = std::min(r.est_lo, in.est_units); r.est_hi = std::max(r.est_hi, in.est_units);
    if (c >= 0) r.classes |= 1u << c;
}

void check(const Input &x, const In &in) {
    const Plan p = launch_plan(in);
    const First by_class[3] = {p.first.for_uniform, p.first.for_sparse, p.first.for_clade};
    for (int c = 0; c < 3; c++) {
        const bool first = admits(p.hash_small, in.verdict, c) || admits(p.hash_big, in.verdict, c) || admits(p.sorted, in.verdict, c);
        const bool wide = wide_takes_all(p, in.verdict, c);
        if (!first && !wide) flag("class placed by no kernel (its reads keep whatever their result buffers held)", x, in, c);
        if (first && wide) flag("class placed twice (a first kernel and place_packed16w_kernel on every tile)", x, in, c);
        if (!p.fit.sorted_fits && by_class[c] == F_SORTED) flag("F_SORTED without sorted_fits", x, in, c);
        if (!p.fit.hash_fits && (by_class[c] == F_HASH_BIG || by_class[c] == F_HASH_SMALL)) flag("hash kernel without hash_fits", x, in, c);
    }
    if (p.sorted.run && (x.wpr > 16 || !p.fit.sorted_fits)) flag("place_packed16s_kernel launched on records it cannot hold", x, in, -1);
    if ((p.hash_small.run || p.hash_big.run || p.hash_behind.run) && !p.fit.hash_fits) flag("place_hash64_kernel launched without hash_fits", x, in, -1);
    if (!in.verdict && (by_class[0] != by_class[1] || by_class[0] != by_class[2])) flag("classes differ without a verdict", x, in, -1);
    if (!in.first_ok && (p.hash_small.run || p.hash_big.run || p.hash_behind.run || p.sorted.run || p.only_marked))
        flag("first kernel or only_marked without the tile marks", x, in, -1);
    if (p.hash_behind.run && !(p.hash_small.run && in.marked_list && p.hash_behind.only_if == p.hash_small.only_if))
        flag("2 048-slot second launch not behind the small table's tiles", x, in, -1);
    if (p.only_marked != (p.hash_small.run || p.hash_big.run || p.sorted.run)) flag("only_marked without a first kernel", x, in, -1);
}

int run_case(char **v) {
    Input x{};
    x.bits = (uint32_t)atoi(v[0]); x.k = (uint32_t)atoi(v[1]); x.wpr = (uint32_t)atoi(v[2]); x.lens = atoi(v[3]) != 0;
    x.fixed_len = (uint32_t)atoi(v[4]); x.upc = atof(v[5]); x.epk = atof(v[6]);
    x.in.n_branches = (uint32_t)atoi(v[7]); x.in.hash_capable = atoi(v[8]) != 0; x.in.stream = atoi(v[9]) != 0;
    x.in.verdict = atoi(v[10]) != 0; x.in.first_ok = atoi(v[11]) != 0; x.in.marked_list = atoi(v[12]) != 0;
    const In in = make_in(x, read_shape(x.bits, x.k, x.wpr, x.lens, x.fixed_len, x.upc));
    const Plan p = launch_plan(in);
    printf("est_units=%.3f\nfull_hit_entries=%.1f\none_batch=%d\nhash_fits=%d\nhash_small=%d\nsorted_fits=%d\n", in.est_units, in.full_hit_entries,
           in.one_batch, p.fit.hash_fits, p.fit.hash_small, p.fit.sorted_fits);
    printf("for_uniform=%d\nfor_sparse=%d\nfor_clade=%d\n", p.first.for_uniform, p.first.for_sparse, p.first.for_clade);
    printf("hash_small=%d,%u\nhash_big=%d,%u\nhash_behind=%d,%u\nsorted=%d,%u\n", p.hash_small.run, p.hash_small.only_if, p.hash_big.run,
           p.hash_big.only_if, p.hash_behind.run, p.hash_behind.only_if, p.sorted.run, p.sorted.only_if);
    printf("only_marked=%d\nmarked_if=%u\n", p.only_marked, p.marked_if);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 15 && !strcmp(argv[1], "case")) return run_case(argv + 2);
    std::vector<uint32_t> nbs;
    for (uint32_t nb = 1117; nb < 65535; nb += 1499) nbs.push_back(nb);
    for (uint32_t nb : {2000u, 2001u, 2600u, 9250u, 13500u, 17250u, 18700u, 24000u, 24001u, 28000u, 28001u, 36000u, 42000u, 56000u, 56001u, 65535u})
        nbs.push_back(nb);
    const double upcs[] = {0.0, 0.02, 0.05, 0.1, 0.2, 0.34, 0.5, 0.75, 1.0, 1.5, 2.2, 3.0};
    const double epks[] = {1.0, 4.0, 12.7, 30.0};
    struct Alpha { uint32_t bits, k; std::vector<uint32_t> fixed; };
    const Alpha alphas[] = {{2, 10, {50, 100, 150, 153, 154, 200, 256, 260, 400}}, {2, 8, {151, 152, 200}}, {5, 5, {60, 100, 102, 103, 116, 117, 120, 180}}};
    const uint32_t wprs[] = {4, 8, 10, 12, 16, 17, 20, 24, 32};
    uint64_t evaluated = 0;
    for (const Alpha &al : alphas) {
        std::vector<Input> shapes;
        for (uint32_t w : wprs) shapes.push_back(Input{al.bits, al.k, w, true, 0, 0, 0, In{}});
        for (uint32_t L : al.fixed) shapes.push_back(Input{al.bits, al.k, (L * al.bits + 31) / 32, false, L, 0, 0, In{}});
        for (Input x : shapes)
            for (double upc : upcs)
                for (double epk : epks) {
                    x.upc = upc; x.epk = epk;
                    const ReadShape rs = read_shape(x.bits, x.k, x.wpr, x.lens, x.fixed_len, upc);
                    if (rs.est_units > 400.0) continue;
                    for (uint32_t bools = 0; bools < 32; bools++) {
                        x.in.hash_capable = bools & 1; x.in.stream = bools & 2; x.in.verdict = bools & 4;
                        x.in.first_ok = bools & 8; x.in.marked_list = bools & 16;
                        if (x.in.marked_list && !x.in.first_ok) continue;  // (the list lives behind the marks)
                        for (uint32_t kb = 0; kb < 64; kb++) {
                            Knobs &kn = x.in.knobs;
                            kn.hash_always = kb & 1; kn.hash_big_table = kb & 2; kn.hash_small_table = kb & 4; kn.hash_clade_small = kb & 8;
                            kn.wstream_always = kb & 16; kn.no_wstream = kb & 32;
                            if (x.in.hash_capable && (kn.no_wstream || !(x.in.stream || kn.hash_always))) continue;  // (rk_engine.hip: hash_capable)
                            for (uint32_t nb : nbs) {
                                x.in.n_branches = nb;
                                check(x, make_in(x, rs));
                                evaluated++;
                            }
                        }
                    }
                }
    }
    for (const auto &v : violations) {
        const Region &r = v.second;
        printf("VIOLATION %s: %llu inputs; n_branches %u .. %u, est_units %.1f .. %.1f, words_per_read %u .. %u, classes mask %u; e.g. %s\n",
               v.first.c_str(), (unsigned long long)r.count, r.nb_lo, r.nb_hi, r.est_lo, r.est_hi, r.wpr_lo, r.wpr_hi, r.classes, r.example.c_str());
    }
    printf("%llu inputs, %zu rules violated\n", (unsigned long long)evaluated, violations.size());
    return violations.empty() ? 0 : 1;
}
