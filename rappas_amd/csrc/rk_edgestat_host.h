// rk_edgestat_host.h -- the host side of the edge statistics (edge dispersion and edge correlation; include/rappas_place.h holds the
// definition): the host twin of the kernels of rk_edgestat.h behind rk_edgestat_host, and the one finish (the only
// square roots) behind rk_edgestat_finish_host.  Header-only, plain C++, beside rk_samples_host.h, whose tree walk, clade sums and
// lane rule it uses.  The profiles, the centring and the rank word are those of rk_samplemath.h, the text the kernels compile; the
// ranks are found by a sort of the active values and two binary searches an entry, the integers of the definition's counting.
// Not part of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rk_samples_host.h"

namespace rk {

constexpr uint32_t EDGESTAT_MAX_SAMPLES = 4096, EDGESTAT_MAX_FEATURES = 8;
constexpr uint64_t EDGESTAT_NAN = 0x7FF8000000000000ull;  // the filler of a double of an unusable column

inline uint64_t edgestat_row_words(uint32_t F) { return 6 + 4 * (uint64_t)F; }
inline uint64_t edgestat_out_words(uint32_t B, uint32_t F) { return (uint64_t)B * edgestat_row_words(F) + 3 * (uint64_t)F; }

inline uint64_t edgestat_word(double d) {
    uint64_t w;
    memcpy(&w, &d, 8);
    return w;
}
inline double edgestat_double(uint64_t w) {
    double d;
    memcpy(&d, &w, 8);
    return d;
}

// d[s] = rank2(a)[s] - (n + 1) over the active entries, 0 for the others; `sorted` is scratch.  Returns rss.
inline int64_t edgestat_ranks(uint32_t S, uint32_t n, const uint8_t *active, const double *a, std::vector<double> &sorted, int32_t *d) {
    sorted.clear();
    for (uint32_t s = 0; s < S; s++)
        if (active[s]) sorted.push_back(a[s]);
    std::sort(sorted.begin(), sorted.end());
    int64_t rss = 0;
    for (uint32_t s = 0; s < S; s++) {
        d[s] = 0;
        if (!active[s]) continue;
        const uint32_t less = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), a[s]) - sorted.begin());
        const uint32_t upto = (uint32_t)(std::upper_bound(sorted.begin(), sorted.end(), a[s]) - sorted.begin());
        d[s] = edgestat_rank_dev(less, upto, n);
        rss += (int64_t)d[s] * d[s];
    }
    return rss;
}

// mean, the centred entries c[S] and ss of a row whose inactive entries count as +0.0
inline void edgestat_moments(uint32_t S, uint32_t n, const uint8_t *active, const double *a, double &mean, double *c, double &ss) {
    mean = lane_sum(S, [&](uint32_t s) { return active[s] ? a[s] : 0.0; }) / (double)n;
    for (uint32_t s = 0; s < S; s++) c[s] = edgestat_centre(active[s] != 0, a[s], mean);
    ss = lane_sum(S, [&](uint32_t s) { const double t = c[s] * c[s]; return t; });
}

// What the column prelude leaves of the metadata: per column whether it is usable, gc[S] and gd[S]; its three raw words are written
struct EdgestatColumns {
    uint32_t unusable = 0;
    std::vector<double> gc;   // [F][S]
    std::vector<int32_t> gd;  // [F][S]
};
inline void edgestat_columns(uint32_t S, uint32_t n, uint32_t F, const uint8_t *active, const double *meta, EdgestatColumns &col, uint64_t *feature_rows) {
    col.gc.assign((uint64_t)F * S, 0.0);
    col.gd.assign((uint64_t)F * S, 0);
    std::vector<double> sorted;
    for (uint32_t f = 0; f < F; f++) {
        const double *g = meta + (uint64_t)f * S;
        uint64_t *out = feature_rows + 3 * (uint64_t)f;
        bool usable = true;
        for (uint32_t s = 0; s < S; s++) usable = usable && (!active[s] || std::isfinite(g[s]));
        if (!usable) {
            col.unusable |= 1u << f;
            out[0] = out[1] = EDGESTAT_NAN;
            out[2] = 0;
            continue;
        }
        double mean, ss;
        edgestat_moments(S, n, active, g, mean, col.gc.data() + (uint64_t)f * S, ss);
        const int64_t rss = edgestat_ranks(S, n, active, g, sorted, col.gd.data() + (uint64_t)f * S);
        out[0] = edgestat_word(mean);
        out[1] = edgestat_word(ss);
        out[2] = (uint64_t)rss;
    }
}

// One quantity of one edge: a[S] (the entries of inactive samples +0.0) -> the words of the row that belong to q
inline void edgestat_quantity(uint32_t S, uint32_t n, uint32_t F, uint32_t q, const uint8_t *active, const double *a, const EdgestatColumns &col, double *c, int32_t *d,
                              std::vector<double> &sorted, uint64_t *row) {
    double mean, ss;
    edgestat_moments(S, n, active, a, mean, c, ss);
    const int64_t rss = edgestat_ranks(S, n, active, a, sorted, d);
    row[3 * q] = edgestat_word(mean);
    row[3 * q + 1] = edgestat_word(ss);
    row[3 * q + 2] = (uint64_t)rss;
    for (uint32_t f = 0; f < F; f++) {
        uint64_t *out = row + 6 + 4 * (uint64_t)f + 2 * q;
        if (col.unusable >> f & 1) {
            out[0] = EDGESTAT_NAN;
            out[1] = 0;
            continue;
        }
        const double *gc = col.gc.data() + (uint64_t)f * S;
        const int32_t *gd = col.gd.data() + (uint64_t)f * S;
        out[0] = edgestat_word(lane_sum(S, [&](uint32_t s) { const double t = c[s] * gc[s]; return t; }));
        int64_t rcross = 0;
        for (uint32_t s = 0; s < S; s++) rcross += (int64_t)d[s] * gd[s];
        out[1] = (uint64_t)rcross;
    }
}

// The rows of the edges x = x_lo, x_lo + x_step, ...: clade [S][B] and the masses of the buffer (W words a sample) in, raw rows out
inline void edgestat_edges(uint32_t B, uint32_t S, uint64_t W, uint32_t root, uint32_t n, uint32_t F, const uint8_t *active, const uint64_t *masses, const uint64_t *clade,
                           const EdgestatColumns &col, uint32_t x_lo, uint32_t x_step, uint64_t *raw) {
    std::vector<double> a0(S), a1(S), c(S), sorted;
    std::vector<int32_t> d(S);
    for (uint64_t x = x_lo; x < B; x += x_step) {
        for (uint64_t s = 0; s < S; s++) {
            const bool on = active[s] && x != root;
            const uint64_t T = clade[s * B + root];
            a0[s] = on ? edgestat_share(masses[s * W + x], T) : 0.0;
            a1[s] = on ? edgestat_imbalance(clade[s * B + x], masses[s * W + x], T) : 0.0;
        }
        uint64_t *row = raw + x * edgestat_row_words(F);
        edgestat_quantity(S, n, F, 0, active, a0.data(), col, c.data(), d.data(), sorted, row);
        edgestat_quantity(S, n, F, 1, active, a1.data(), col, c.data(), d.data(), sorted, row);
    }
}

// Finish: what a caller reads, from the raw output and its info words (rk_edgestat_finish_host)
inline void edgestat_finish(uint32_t B, uint32_t F, const uint64_t *raw, const uint32_t *info, double *table, double *feature_table) {
    const uint64_t RW = edgestat_row_words(F), C = 8 + 4 * (uint64_t)F;
    const uint64_t *feat = raw + (uint64_t)B * RW;
    if (info[0] == 0) {  // the raw words are fillers, not sums
        for (uint64_t i = 0; i < (uint64_t)B * C; i++) table[i] = edgestat_double(EDGESTAT_NAN);
        for (uint64_t i = 0; i < 2 * (uint64_t)F; i++) feature_table[i] = edgestat_double(EDGESTAT_NAN);
        return;
    }
    const double n = (double)info[0];
    for (uint32_t f = 0; f < F; f++) {
        feature_table[2 * f] = edgestat_double(feat[3 * f]);
        feature_table[2 * f + 1] = edgestat_double(feat[3 * f + 1]) / n;
    }
    for (uint64_t x = 0; x < B; x++) {
        const uint64_t *row = raw + x * RW;
        double *out = table + x * C;
        for (uint32_t q = 0; q < 2; q++) {
            const double mean = edgestat_double(row[3 * q]), ss = edgestat_double(row[3 * q + 1]);
            const double var = ss / n, sd = std::sqrt(var);
            double *o = out + 5 * q;
            o[0] = mean;
            o[1] = var;
            o[2] = sd;
            if (q == 0) {
                o[3] = sd / mean;
                o[4] = var / mean;
            }
            const double rss = (double)(int64_t)row[3 * q + 2];
            for (uint32_t f = 0; f < F; f++) {
                const double gss = edgestat_double(feat[3 * f + 1]), grss = (double)(int64_t)feat[3 * f + 2];
                const double cross = edgestat_double(row[6 + 4 * f + 2 * q]), rcross = (double)(int64_t)row[6 + 4 * f + 2 * q + 1];
                const double pp = ss * gss, rr = rss * grss;
                out[8 + 4 * f + 2 * q] = cross / std::sqrt(pp);
                out[8 + 4 * f + 2 * q + 1] = rcross / std::sqrt(rr);
            }
        }
    }
}

}  // namespace rk
