// The launch geometry of the placement kernels (rappas_amd/csrc/rk_geometry.h) swept over its inputs: every LDS layout a kernel is launched
// with must stay inside the block's allocation, and the blocks a CU is asked to hold must fit its LDS.  Built and run by
// tests/test_geometry_grid.py; no GPU, no HIP.
//   geometry_grid                  sweep the grid; prints one line per violated rule (with the region of inputs where it fails), exit 1
//   geometry_grid case FAMILY K=V ...
//                                  every field of one geometry, as one line of key=value pairs
//   geometry_grid table FILE       FILE holds lines "FAMILY <tab> K=V ... <tab> fields": prints each line with its fields recomputed
//   geometry_grid list             the inputs of tests/golden/launch_geometry.tsv, with their fields
// FAMILY: dense plan windowed sorted hash wg amb.  Inputs (all optional): nb lds bits keep lanes wpr upc upr passes log_slots indexed
#include "rk_geometry.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace rk_geom;

namespace {

const size_t AMB_LIST_BYTES = 160 * 8 + 640;  // place_ascii_kernel: a candidate list of 160 items + the alphabet's tables (rk_kernels.hip)

struct Input {
    std::string family;
    uint32_t nb = 999, bits = 2, keep = 7, lanes = 0, wpr = 10, log_slots = RK_HASH_LOG_SLOTS;
    size_t lds = 160 * 1024;
    double upc = 1.0, upr = 1.5;  // row units per k-mer code and per row: what decides WindowPlan::stream
    int passes = 1;
    bool indexed = false;
};

std::string inputs_of(const Input &x) {
    char b[256];
    const std::string &f = x.family;
    if (f == "dense") snprintf(b, sizeof(b), "nb=%u lds=%zu bits=%u keep=%u lanes=%u", x.nb, x.lds, x.bits, x.keep, x.lanes);
    else if (f == "plan") snprintf(b, sizeof(b), "nb=%u bits=%u upc=%g upr=%g", x.nb, x.bits, x.upc, x.upr);
    else if (f == "windowed") snprintf(b, sizeof(b), "nb=%u lds=%zu bits=%u upc=%g upr=%g keep=%u wpr=%u", x.nb, x.lds, x.bits, x.upc, x.upr, x.keep, x.wpr);
    else if (f == "sorted") snprintf(b, sizeof(b), "nb=%u lds=%zu bits=%u upc=%g upr=%g", x.nb, x.lds, x.bits, x.upc, x.upr);
    else if (f == "hash") snprintf(b, sizeof(b), "lds=%zu log_slots=%u", x.lds, x.log_slots);
    else if (f == "wg") snprintf(b, sizeof(b), "nb=%u lds=%zu keep=%u passes=%d", x.nb, x.lds, x.keep, x.passes);
    else snprintf(b, sizeof(b), "nb=%u lds=%zu indexed=%d passes=%d", x.nb, x.lds, x.indexed, x.passes);
    return b;
}

bool parse(const std::string &family, const std::vector<std::string> &kv, Input &x) {
    x.family = family;
    for (const std::string &s : kv) {
        const size_t eq = s.find('=');
        if (eq == std::string::npos) return false;
        const std::string k = s.substr(0, eq), v = s.substr(eq + 1);
        if (k == "nb") x.nb = (uint32_t)atoll(v.c_str());
        else if (k == "lds") x.lds = (size_t)atoll(v.c_str());
        else if (k == "bits") x.bits = (uint32_t)atoi(v.c_str());
        else if (k == "keep") x.keep = (uint32_t)atoi(v.c_str());
        else if (k == "lanes") x.lanes = (uint32_t)atoi(v.c_str());
        else if (k == "wpr") x.wpr = (uint32_t)atoi(v.c_str());
        else if (k == "upc") x.upc = atof(v.c_str());
        else if (k == "upr") x.upr = atof(v.c_str());
        else if (k == "passes") x.passes = atoi(v.c_str());
        else if (k == "log_slots") x.log_slots = (uint32_t)atoi(v.c_str());
        else if (k == "indexed") x.indexed = atoi(v.c_str()) != 0;
        else return false;
    }
    static const char *families[] = {"dense", "plan", "windowed", "sorted", "hash", "wg", "amb"};
    return std::any_of(std::begin(families), std::end(families), [&](const char *f) { return family == f; });
}

std::string wave_fields(Status st, const WaveGeometry &w) {
    char b[256];
    snprintf(b, sizeof(b), "status=%d s_stride=%u main_cap=%u work_cap=%u list_cap=%u lds_wave=%zu waves_cu=%u wide=%d", st, w.s_stride, w.main_cap,
             w.work_cap, w.list_cap, w.lds_wave, w.waves_cu, w.wide);
    return b;
}

std::string fields_of(const Input &x) {
    char b[320];
    Knobs kn;
    kn.wg_passes = x.passes;
    const std::string &f = x.family;
    WindowPlan wp;
    const bool planned = window_plan(x.nb, x.bits, x.upc, x.upr, kn, wp);
    if (f == "dense") {
        Geometry g{};
        const Status st = choose_geometry(x.nb, x.bits, x.lds, x.lanes, x.keep, kn, g);
        snprintf(b, sizeof(b), "status=%d G=%u NG=%u s_stride=%u list_cap=%u pu=%u lds_per_wave=%zu waves_per_cu=%u", st, g.G, g.NG, g.s_stride, g.list_cap,
                 g.pu, g.lds_per_wave, g.waves_per_cu);
    } else if (f == "plan") {
        snprintf(b, sizeof(b), "planned=%d stream=%d n_win=%u W=%u s_stride=%u main_cap=%u work_cap=%u lds_wave=%zu", planned, wp.stream, wp.n_win, wp.W, wp.s_stride,
                 wp.main_cap, wp.work_cap, lds_of_four_reads(wp.s_stride, wp.main_cap, wp.work_cap));
    } else if (f == "windowed" || f == "sorted") {
        if (!planned) return "planned=0";
        WaveGeometry w;
        const Status st = f == "windowed" ? windowed_geometry(wp, x.keep, x.wpr, x.lds, w) : sorted_geometry(wp, x.lds, w);
        return "planned=1 " + wave_fields(st, w);
    } else if (f == "hash") {
        return wave_fields(GEOM_OK, hash_geometry(x.log_slots, rk_plan::hash_key_limit(rk_plan::Knobs{}, x.log_slots), x.lds, kn));
    } else if (f == "wg") {
        WgGeometry g{};
        const Status st = choose_wg_geometry(x.nb, x.lds, x.keep, kn, g);
        snprintf(b, sizeof(b), "status=%d nw=%u s_stride=%u list_cap=%u wgs_per_cu=%u n_pass=%u lds=%zu", st, g.nw, g.s_stride, g.list_cap, g.wgs_per_cu, g.n_pass, g.lds);
    } else {
        AmbGeometry a;
        const Status st = amb_geometry(x.nb, x.lds, x.indexed, AMB_LIST_BYTES, kn, a);
        snprintf(b, sizeof(b), "status=%d s_stride=%u amb_chunk=%u s_win=%u lds=%zu waves_cu=%u", st, a.s_stride, a.amb_chunk, a.s_win, a.lds, a.waves_cu);
    }
    return b;
}

void print_line(const Input &x) { printf("%s\t%s\t%s\n", x.family.c_str(), inputs_of(x).c_str(), fields_of(x).c_str()); }

std::vector<std::string> words(const std::string &s) {
    std::istringstream in(s);
    std::vector<std::string> out;
    for (std::string w; in >> w;) out.push_back(w);
    return out;
}

int run_table(const char *path) {
    std::ifstream in(path);
    if (!in) return 2;
    for (std::string line; std::getline(in, line);) {
        if (line.empty() || line[0] == '#') { printf("%s\n", line.c_str()); continue; }
        const size_t t1 = line.find('\t'), t2 = line.find('\t', t1 + 1);
        Input x;
        if (t1 == std::string::npos || t2 == std::string::npos || !parse(line.substr(0, t1), words(line.substr(t1 + 1, t2 - t1 - 1)), x)) return 2;
        print_line(x);
    }
    return 0;
}

const size_t LDS_SIZES[] = {160 * 1024, 64 * 1024};
// the two shapes of rows a windowed image is planned for: short rows (place_packed16s_kernel first beyond 4 500 branches, narrower
// windows) and rows of several units (place_packed16w_kernel alone)
const struct { double upc, upr; } ROWS[] = {{1.0, 1.5}, {0.3, 5.0}};

// tests/golden/launch_geometry.tsv: the tree sizes at which a geometry changes its path, crossed with the small axes
int run_list() {
    const uint32_t sizes[] = {1, 3, 4, 999, 1116, 1117, 1276, 1277, 1290, 1999, 3999, 4500, 4501, 8192, 8193, 9001, 16000, 16001, 19999, 28001, 39999, 65534, 65535};
    printf("# family <tab> inputs <tab> every field of the geometry (tests/geometry_grid.cpp: `geometry_grid list`)\n");
    for (uint32_t ls : {RK_HASH_LOG_SLOTS, RK_HASH_LOG_SLOTS - 1})
        for (size_t lds : LDS_SIZES) { Input x; x.family = "hash"; x.log_slots = ls; x.lds = lds; print_line(x); }
    for (uint32_t nb : sizes) {
        Input x;
        x.nb = nb;
        x.family = "dense";
        for (size_t lds : LDS_SIZES)
            for (uint32_t lanes : {0u, 8u, 16u, 32u, 64u})
                for (uint32_t keep : {1u, 7u, 16u})
                    for (uint32_t bits : {2u, 5u}) {
                        if (bits == 5 && keep != 7) continue;  // (the alphabet only sets the probe rounds)
                        x.lds = lds; x.lanes = lanes; x.keep = keep; x.bits = bits;
                        print_line(x);
                    }
        x = Input(); x.nb = nb;
        for (uint32_t bits : {2u, 5u})
            for (const auto &r : ROWS) {
                x.bits = bits; x.upc = r.upc; x.upr = r.upr;
                x.family = "plan";
                print_line(x);
                if (nb <= RK_WINDOW_MIN_BRANCHES || bits == 5) continue;  // (the alphabet only decides WindowPlan::stream, as the rows do)
                for (size_t lds : LDS_SIZES) {
                    x.lds = lds;
                    x.family = "sorted";
                    print_line(x);
                    x.family = "windowed";
                    for (uint32_t keep : {7u, 9u})
                        for (uint32_t wpr : {10u, 11u, 40u}) { x.keep = keep; x.wpr = wpr; print_line(x); }
                }
            }
        for (size_t lds : LDS_SIZES)
            for (int passes : {1, 2, 4}) {
                x = Input(); x.nb = nb; x.lds = lds; x.passes = passes;
                x.family = "wg";
                for (uint32_t keep : {7u, 16u}) { x.keep = keep; print_line(x); }
                if (passes == 4) continue;
                x.family = "amb";
                for (bool indexed : {false, true}) { x.indexed = indexed; print_line(x); }
            }
    }
    return 0;
}

struct Region {
    uint64_t count = 0;
    uint32_t nb_lo = ~0u, nb_hi = 0;
    std::string example;
};
std::map<std::string, Region> violations;

void flag(const char *rule, const Input &x) {
    Region &r = violations[rule];
    if (!r.count) r.example = x.family + " " + inputs_of(x) + " -> " + fields_of(x);
    r.count++;
    r.nb_lo = std::min(r.nb_lo, x.nb); r.nb_hi = std::max(r.nb_hi, x.nb);
}

// `wanted` blocks of `lds` bytes a CU: what is resident (the granule rule; the occupancy query can only lower it) fits the CU's LDS.
// FINDING: resident_per_cu counts the granules of a 160 KB CU whatever lds_per_cu is, so on a CU of 64 KB (no gfx950) blocks of a few KB
// fit by division only (dense up to 5 203 branches, the ambiguity kernel up to 4 968: e.g. 31 blocks of 2 064 B are 31 x 2 560 B); there
// the occupancy query is what holds the grid to one round.  With granules at 160 KB, by division at 64 KB.
bool resident_fit(uint64_t wanted, size_t lds, size_t lds_per_cu) {
    const uint64_t n = resident_per_cu(wanted, ~0ull, lds);
    return n * (lds_per_cu == 160 * 1024 ? (lds + 511) & ~(size_t)511 : lds) <= lds_per_cu;
}

uint64_t evaluated = 0;

void check_dense(Input &x) {
    x.family = "dense";
    Knobs kn;
    Geometry g{};
    evaluated++;
    const Status st = choose_geometry(x.nb, x.bits, x.lds, x.lanes, x.keep, kn, g);
    if (st == KEEP_NEEDS_LANES) {
        if (x.lanes == 0 || x.lanes >= x.keep) flag("dense: refused for keep_at_most although the lanes hold it", x);
        return;
    }
    if (st == READ_EXCEEDS_LDS) {
        if (g.lds_per_wave <= x.lds) flag("dense: refused although one wave fits", x);
        return;
    }
    const uint32_t min_cap = g.G + 3 * (g.G == 64 ? RK_RING64 : RK_RING) + 40;
    if (g.s_stride % 4 || g.s_stride < x.nb + 1) flag("dense: s_stride not a multiple of 4 or < n_branches + 1", x);
    if (g.list_cap % 2 || g.list_cap < min_cap) flag("dense: list_cap odd or below min_cap", x);
    if (g.G < x.keep || g.NG * g.G != 64) flag("dense: lane group does not hold keep_at_most", x);
    if (g.lds_per_wave != (size_t)g.NG * ((size_t)g.s_stride * 4 + (size_t)g.list_cap * 8)) flag("dense: lds_per_wave is not NG score vectors and lists", x);
    if (g.waves_per_cu < 1 || !resident_fit(g.waves_per_cu, g.lds_per_wave, x.lds)) flag("dense: resident waves do not fit the CU's LDS", x);
}

void check_windowed(Input &x, const WindowPlan &wp) {
    WaveGeometry w;
    x.family = "windowed";
    evaluated++;
    const Status st = windowed_geometry(wp, x.keep, x.wpr, x.lds, w);
    if (st != GEOM_OK) { flag("windowed: no wave fits", x); return; }
    if (w.work_cap % 2 || w.work_cap < (x.keep > 8 ? 96u : 88u)) flag("windowed: work_cap odd or below the select's scratch", x);
    // FINDING (the arithmetic as it was before it moved here): from 65 281 branches on (64 windows of 1 024) the plan leaves a main list of
    // 164 items and a work list of 88, and keep_at_most > 8 moves 8 of them to the work list: 156.  Left as it is; the rule holds for the
    // plan, for keep_at_most <= 8 everywhere and for keep_at_most > 8 below 65 281 branches.
    if (w.main_cap < (x.keep > 8 && x.nb > 65280 ? 156u : 160u)) flag("windowed: main_cap below 160 (156 for keep_at_most > 8 on the largest trees)", x);
    if (w.main_cap + w.work_cap != wp.main_cap + wp.work_cap) flag("windowed: main_cap + work_cap not conserved by the re-balance", x);
    if (w.s_stride != wp.W + 4 || w.list_cap != w.work_cap / 2) flag("windowed: s_stride is not W + 4 or list_cap not half the work list", x);
    if (w.lds_wave != (size_t)16 * (w.s_stride + w.main_cap + w.work_cap)) flag("windowed: lds_wave is not four reads' slots and lists", x);
    if (w.waves_cu < 1 || w.waves_cu > 8 || !resident_fit(w.waves_cu, w.lds_wave, x.lds)) flag("windowed: resident waves do not fit the CU's LDS", x);
}

void check_sorted(Input &x, const WindowPlan &wp) {
    WaveGeometry w;
    x.family = "sorted";
    evaluated++;
    const Status st = sorted_geometry(wp, x.lds, w);
    if (st != GEOM_OK) { flag("sorted: no wave fits", x); return; }
    if (w.main_cap % 4 || w.main_cap > 640) flag("sorted: main_cap not a multiple of 4 or beyond 640", x);
    if (w.main_cap < 200 + 5 * wp.n_win + 24 - 3) flag("sorted: a list below its need", x);
    // no unsigned wrap in budget - s_str - work: a wrapped list is clamped to 640 items and looks legal by itself, so the three parts are
    // held against the budget they were cut from -- whole 512-byte granules of a 160 KB CU shared by 5 .. 8 waves; and on such a CU the
    // launch asks for exactly the waves whose budget they fit
    const uint32_t words = w.s_stride + w.main_cap + w.work_cap;
    uint32_t budget_waves = 0;
    for (uint32_t n = 5; n <= 8; n++)
        if (words <= (160 * 1024 / n / 512 * 512) / 16) budget_waves = n;
    if (!budget_waves) flag("sorted: slots + list + work list beyond the budget of five waves (unsigned wrap in budget - s_str - work)", x);
    else if (x.lds == 160 * 1024 && w.waves_cu != budget_waves) flag("sorted: the waves asked for are not the waves whose budget the layout fits", x);
    if (w.s_stride != wp.W + 16) flag("sorted: s_stride is not W + 16", x);
    if (w.work_cap % 2 || w.work_cap < 96 || w.list_cap != w.work_cap / 2) flag("sorted: work list odd, below 96 or list_cap not its half", x);
    if (w.wide != (wp.W > 512)) flag("sorted: WIDE does not follow the window", x);
    if (w.lds_wave != (size_t)16 * (w.s_stride + w.main_cap + w.work_cap)) flag("sorted: lds_wave is not four reads' slots and lists", x);
    if (w.waves_cu < 1 || w.waves_cu > 8 || !resident_fit(w.waves_cu, w.lds_wave, x.lds)) flag("sorted: resident waves do not fit the CU's LDS", x);
}

void check_wg(Input &x) {
    x.family = "wg";
    Knobs kn;
    kn.wg_passes = x.passes;
    WgGeometry g{};
    evaluated++;
    if (choose_wg_geometry(x.nb, x.lds, x.keep, kn, g) != GEOM_OK) {
        // refused only when not even four passes of sixteen waves fit
        const size_t s_bytes = (size_t)(((x.nb + 3) / 4 + 4) & ~3u) * 4;
        if (s_bytes + 256 + (size_t)(4 * 16 * x.keep + 18) * 8 + 66 * 8 <= x.lds) flag("wg: refused although four passes fit", x);
        return;
    }
    uint32_t win = 0;
    for (uint32_t p = 0; p < g.n_pass; p++) {
        const uint32_t span = 32 / g.n_pass;
        win = std::max(win, (uint32_t)(((uint64_t)(p + 1) * span * x.nb) / 32) - (uint32_t)(((uint64_t)p * span * x.nb) / 32));
    }
    const size_t min_list = g.n_pass > 1 ? 66 : std::max<size_t>(66, (size_t)g.nw * x.keep + 18);
    const size_t cand = g.n_pass > 1 ? (size_t)(g.n_pass * g.nw * x.keep + 18) * 8 : 0;
    if (g.n_pass < (uint32_t)x.passes || (g.n_pass != 1 && g.n_pass != 2 && g.n_pass != 4)) flag("wg: fewer passes than forced", x);
    if (g.s_stride % 4 || g.s_stride < win + 1) flag("wg: s_stride not a multiple of 4 or < window + 1", x);
    if (g.list_cap % 2 || g.list_cap < min_list || g.list_cap > 512) flag("wg: list_cap odd or below min_list", x);
    if (g.nw * g.wgs_per_cu != 16) flag("wg: not sixteen waves a CU", x);
    if (g.lds != (size_t)g.s_stride * 4 + (size_t)g.list_cap * 8 + 256 + cand) flag("wg: lds is not S | list | counters | candidates", x);
    if (!resident_fit(g.wgs_per_cu, g.lds, x.lds)) flag("wg: resident workgroups do not fit the CU's LDS", x);
}

void check_amb(Input &x) {
    x.family = "amb";
    Knobs kn;
    kn.wg_passes = x.passes;
    AmbGeometry a;
    evaluated++;
    if (amb_geometry(x.nb, x.lds, x.indexed, AMB_LIST_BYTES, kn, a) != GEOM_OK) { flag("amb: refused", x); return; }
    if (a.amb_chunk < 1) flag("amb: chunk < 1", x);
    if ((size_t)a.s_stride * 4 + AMB_LIST_BYTES + 8 * (size_t)a.amb_chunk != a.lds || a.lds > x.lds) flag("amb: S | list | Samb | Camb | tables beyond the CU's LDS", x);
    if (a.s_win == x.nb ? a.s_stride % 4 || a.s_stride < x.nb + 1 : a.s_win % 4 || a.s_stride != a.s_win + 4 || a.amb_chunk != a.s_win) flag("amb: s_stride does not hold the window", x);
    if (a.amb_chunk > a.s_stride) flag("amb: chunk beyond the score vector", x);
    if (a.waves_cu < 1 || !resident_fit(a.waves_cu, a.lds, x.lds)) flag("amb: resident waves do not fit the CU's LDS", x);
}

int run_sweep() {
    for (uint32_t nb = 1; nb <= 65535; nb++) {
        Input x;
        x.nb = nb;
        for (size_t lds : LDS_SIZES) {
            x.lds = lds;
            for (uint32_t bits : {2u, 5u})
                for (uint32_t keep = 1; keep <= 16; keep++)
                    for (uint32_t lanes : {0u, 8u, 16u, 32u, 64u}) { x.bits = bits; x.keep = keep; x.lanes = lanes; check_dense(x); }
            for (int passes : {1, 2, 4})
                for (uint32_t keep = 1; keep <= 16; keep++) { x.passes = passes; x.keep = keep; check_wg(x); }
            for (int passes : {1, 2})
                for (bool indexed : {false, true}) { x.passes = passes; x.indexed = indexed; check_amb(x); }
        }
        for (uint32_t bits : {2u, 5u})
            for (const auto &r : ROWS) {
                x.bits = bits; x.upc = r.upc; x.upr = r.upr;
                WindowPlan wp;
                x.family = "plan";
                evaluated++;
                if (!window_plan(nb, bits, r.upc, r.upr, Knobs{}, wp)) {
                    if (nb > RK_WINDOW_MIN_BRANCHES) flag("plan: no plan for a tree beyond RK_WINDOW_MIN_BRANCHES", x);
                    continue;
                }
                if (wp.n_win < 1 || wp.n_win > 64 || (uint64_t)wp.n_win * wp.W < nb || wp.W % 4 || wp.W > 1024) flag("plan: windows do not cover the tree, or more than 64", x);
                if (wp.main_cap < 160 || wp.main_cap % 2 || wp.work_cap % 2 || wp.work_cap < 88) flag("plan: main_cap < 160 or work_cap < 88", x);
                if (lds_of_four_reads(wp.s_stride, wp.main_cap, wp.work_cap) > 160 * 1024 / 8) flag("plan: more than 1 280 words a read", x);
                for (size_t lds : LDS_SIZES) {
                    x.lds = lds;
                    check_sorted(x, wp);
                    for (uint32_t keep = 1; keep <= 16; keep++)
                        for (uint32_t wpr = 1; wpr <= 40; wpr++) { x.keep = keep; x.wpr = wpr; check_windowed(x, wp); }
                }
            }
    }
    for (uint32_t ls : {RK_HASH_LOG_SLOTS, RK_HASH_LOG_SLOTS - 1})
        for (size_t lds : LDS_SIZES) {
            Input x;
            x.family = "hash"; x.log_slots = ls; x.lds = lds; x.nb = 0;
            evaluated++;
            const WaveGeometry w = hash_geometry(ls, rk_plan::hash_key_limit(rk_plan::Knobs{}, ls), lds, Knobs{});
            if (w.lds_wave != (size_t)(2 * (1u << ls) + 64 + 320) * 4 || w.work_cap + 16 > w.s_stride) flag("hash: lds_wave is not two tables, a word a lane and the list", x);
            if (w.waves_cu < 1 || !resident_fit(w.waves_cu, w.lds_wave, lds)) flag("hash: resident waves do not fit the CU's LDS", x);
        }
    for (const auto &v : violations)
        printf("VIOLATION %s: %llu inputs; n_branches %u .. %u; e.g. %s\n", v.first.c_str(), (unsigned long long)v.second.count, v.second.nb_lo, v.second.nb_hi, v.second.example.c_str());
    printf("%llu inputs, %zu rules violated\n", (unsigned long long)evaluated, violations.size());
    return violations.empty() ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "case")) {
        Input x;
        if (!parse(argv[2], std::vector<std::string>(argv + 3, argv + argc), x)) return 2;
        print_line(x);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "table")) return run_table(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "list")) return run_list();
    return argc == 1 ? run_sweep() : 2;
}
