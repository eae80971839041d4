// rk_samples_host.h -- the host side of the sample-level calls: the checks and the one walk of a tree behind
// rk_tree_validate / rk_tree_create, and the host twins of clade_masses_kernel, kr_pairs_kernel, the squash kernels (rk_samples.h) and
// the edge-PCA kernels (rk_epca.h) behind rk_clade_masses_host, rk_kr_distances_host, rk_squash_host and rk_epca_host, and the
// distance tables of a tree with the twin of edpl_kernel (rk_edpl.h) behind rk_edpl_host and rk_tree_distance_host, and the twin of
// the k-means kernels (rk_kmeans.h) behind rk_kmeans_host, and the twin of the diversity kernels (rk_diversity.h;
// DESIGN.md 4.14) behind rk_diversity_host.  Header-only,
// plain C++, like rk_masses_host.h.  Not part of the C ABI.
//
// The KR distance is written as include/rappas_place.h defines it, term by term and in the order fixed there, so that the device and
// this file give the same bits: the KR term, the Gram term and the chunk rule are those of rk_samplemath.h, the text the kernels
// compile.  The reference has no counterpart: it stops at the jplace it writes.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "rk_divmath.h"
#include "rk_samplemath.h"

namespace rk {

constexpr uint32_t KR_CHUNK = 2048;  // RK_KR_CHUNK: node ids per partial sum

// What one walk of a tree leaves: pre-order position and subtree size of every node, the node at every position.  Children are taken
// in ascending id, so the walk is a function of the parent array alone.
struct TreeWalk {
    uint32_t root = 0;
    std::vector<uint32_t> pre, size, node_at;
};

// The checks of rk_tree_validate, then the walk (iterative: a caterpillar is B - 1 deep).  branch_len == nullptr: the lengths are not
// part of the call (rk_clade_masses_host).  0, or -1 with a message in `msg`; nothing else is written on failure.
inline int tree_walk(const char *who, uint32_t B, const int32_t *parent, const float *branch_len, bool need_len, TreeWalk &w, char *msg, size_t msg_len) {
    auto bad = [&](const char *fmt, auto... a) { snprintf(msg, msg_len, fmt, who, a...); return -1; };
    if (B < 1 || B > 65535) return bad("%s: n_branches=%u must be in 1..65535", B);
    if (!parent) return bad("%s: null parent array");
    if (need_len && !branch_len) return bad("%s: null branch_len array");
    int64_t root = -1;
    std::vector<uint32_t> first(B + 1, 0);  // children of x, as a CSR filled in id order: ascending
    for (uint32_t x = 0; x < B; x++) {
        const int32_t p = parent[x];
        if (p == -1) {
            if (root >= 0) return bad("%s: nodes %u and %u both have parent -1: one root, not more", (uint32_t)root, x);
            root = x;
        } else if (p < 0 || (uint32_t)p >= B) {
            return bad("%s: parent[%u]=%d is outside 0..%u", x, p, B - 1);
        } else if ((uint32_t)p == x) {
            return bad("%s: parent[%u] is the node itself", x);
        } else {
            first[(uint32_t)p + 1]++;
        }
    }
    if (root < 0) return bad("%s: no node has parent -1: the tree has no root");
    if (branch_len)
        for (uint32_t x = 0; x < B; x++)
            if (x != (uint32_t)root && !(branch_len[x] >= 0.0f && std::isfinite(branch_len[x])))
                return bad("%s: branch_len[%u]=%g must be finite and not negative", x, (double)branch_len[x]);
    for (uint32_t x = 0; x < B; x++) first[x + 1] += first[x];
    std::vector<uint32_t> kids(B ? B - 1 : 0), fill(first.begin(), first.end() - 1);
    for (uint32_t x = 0; x < B; x++)
        if ((int64_t)x != root) kids[fill[(uint32_t)parent[x]]++] = x;
    std::vector<uint32_t> pre(B, 0), size(B, 1), node_at(B, 0), next(first.begin(), first.end() - 1), stack;
    uint32_t n = 0;
    stack.push_back((uint32_t)root);
    node_at[0] = (uint32_t)root;
    n = 1;
    while (!stack.empty()) {
        const uint32_t x = stack.back();
        if (next[x] < first[x + 1]) {
            const uint32_t c = kids[next[x]++];
            pre[c] = n;
            node_at[n++] = c;
            stack.push_back(c);
        } else {
            stack.pop_back();
            if (!stack.empty()) size[stack.back()] += size[x];
        }
    }
    if (n != B) {  // whoever was not met hangs on a cycle
        std::vector<char> met(B, 0);
        for (uint32_t p = 0; p < n; p++) met[node_at[p]] = 1;
        uint32_t x = 0;
        while (met[x]) x++;
        return bad("%s: node %u does not reach the root (a cycle among the parents)", x);
    }
    w.root = (uint32_t)root;
    w.pre.swap(pre);
    w.size.swap(size);
    w.node_at.swap(node_at);
    return 0;
}

// h[x]: half the length of the edge above x, 0 for the root
inline double kr_half_length(const float *branch_len, uint32_t x, uint32_t root) { return x == root ? 0.0 : (double)branch_len[x] * 0.5; }

// The clade sums of one sample: c[x] = mass_q30 over x's subtree, x included.  Backwards along the pre-order every node is met after
// its whole subtree, so it hands a finished sum to its parent.  Integers: exact, any order gives the same words.
inline void clade_masses_sample(const TreeWalk &w, const int32_t *parent, const uint64_t *mass, uint64_t *c) {
    const uint32_t B = (uint32_t)w.node_at.size();
    for (uint32_t x = 0; x < B; x++) c[x] = mass[x];
    for (uint32_t p = B; p-- > 1;) {
        const uint32_t x = w.node_at[p];
        c[(uint32_t)parent[x]] += c[x];
    }
}

// The normalised profiles of one sample: u[x] = c(x) / T, v[x] = (c(x) - m(x)) / T, T = c(root).  T == 0: every entry is 0 / 0.
inline void kr_profiles_sample(uint32_t B, uint32_t root, const uint64_t *mass, const uint64_t *c, double *u, double *v) {
    const double T = (double)c[root];
    for (uint32_t x = 0; x < B; x++) {
        u[x] = (double)c[x] / T;
        v[x] = (double)(c[x] - mass[x]) / T;
    }
}

// A sum over the node ids in the order of the definitions: nodes in ascending id, a partial per KR_CHUNK ids that starts at +0.0 and
// takes term(acc, x) node after node; the partials by the chunk rule of rk_samplemath.h.
template <class Term>
inline double chunk_walk(uint32_t B, Term &&term) {
    return chunk_sum((B + KR_CHUNK - 1) / KR_CHUNK, [&](uint32_t c) {
        const uint32_t x0 = c * KR_CHUNK, x1 = x0 + KR_CHUNK < B ? x0 + KR_CHUNK : B;
        double acc = 0.0;
        for (uint32_t x = x0; x < x1; x++) acc = term(acc, x);
        return acc;
    });
}

// D(s, t) from the profiles of the two samples
inline double kr_pair(uint32_t B, const double *h, const double *us, const double *vs, const double *ut, const double *vt) {
    return chunk_walk(B, [&](double acc, uint32_t x) { return kr_term(acc, h[x], us[x], ut[x], vs[x], vt[x]); });
}

// Rows s = s_lo, s_lo + s_step, ... of the matrix: the pairs (s, t >= s), each written at [s][t] and [t][s].  u and v hold the
// profiles sample after sample, B doubles each.
inline void kr_rows(uint32_t B, uint32_t S, const double *h, const double *u, const double *v, uint32_t s_lo, uint32_t s_step, double *out) {
    for (uint64_t s = s_lo; s < S; s += s_step)
        for (uint64_t t = s; t < S; t++) {
            const double d = kr_pair(B, h, u + s * B, v + s * B, u + t * B, v + t * B);
            out[s * S + t] = d;
            out[t * S + s] = d;
        }
}

// ------------------------------------------------------------------------------------------------
// Squash clustering (include/rappas_place.h holds the definition): the host twin of the squash kernels of rk_samples.h.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t SQUASH_NONE = 0xFFFFFFFFu;  // RK_SQUASH_NONE
struct SquashMerge {                           // rk_squash_merge
    uint32_t a, b, size, reserved;
    double distance;
};

// The active pair a < b with the smallest D[a][b]; ties to the smaller a, then the smaller b (rows and columns ascending, strict <).
// false: fewer than two clusters are active.
inline bool squash_pick(uint32_t S, const double *D, const uint8_t *active, uint32_t &a_out, uint32_t &b_out) {
    bool found = false;
    double best = 0.0;
    for (uint32_t a = 0; a < S; a++) {
        if (!active[a]) continue;
        for (uint32_t b = a + 1; b < S; b++)
            if (active[b] && (!found || D[(uint64_t)a * S + b] < best)) {
                found = true;
                best = D[(uint64_t)a * S + b];
                a_out = a;
                b_out = b;
            }
    }
    return found;
}

// Cluster a takes in cluster b: the weighted average of the two profiles, entry by entry
inline void squash_merge_profiles(uint32_t B, uint32_t na, uint32_t nb, double *ua, double *va, const double *ub, const double *vb) {
    const double wa = (double)na, wb = (double)nb, n = (double)(na + nb);
    for (uint32_t x = 0; x < B; x++) {
        ua[x] = (wa * ua[x] + wb * ub[x]) / n;
        va[x] = (wa * va[x] + wb * vb[x]) / n;
    }
}

// The new distances of cluster a to the active clusters t = t_lo, t_lo + t_step, ...: written at [a][t] and [t][a]
inline void squash_row(uint32_t B, uint32_t S, const double *h, const double *u, const double *v, const uint8_t *active, uint32_t a, uint32_t t_lo, uint32_t t_step,
                       double *D) {
    for (uint64_t t = t_lo; t < S; t += t_step) {
        if (!active[t] || t == a) continue;
        const double d = kr_pair(B, h, u + (uint64_t)a * B, v + (uint64_t)a * B, u + t * B, v + t * B);
        D[(uint64_t)a * S + t] = d;
        D[t * S + a] = d;
    }
}

// The S - 1 steps over profiles u, v (sample after sample, B doubles each; merged in place), the matrix D (updated in place) and the
// active flags (cleared as clusters are taken in).  row_step(a) fills the row of the merged cluster: squash_row over every t, dealt
// as the caller likes.  Returns n_merges; the rows behind it are fillers.
template <class RowStep>
inline uint32_t squash_steps(uint32_t B, uint32_t S, double *u, double *v, double *D, uint8_t *active, SquashMerge *merges, RowStep &&row_step) {
    std::vector<uint32_t> size(S, 1);
    uint32_t n_merges = 0;
    for (uint32_t k = 0; k + 1 < S; k++) {
        uint32_t a = 0, b = 0;
        if (!squash_pick(S, D, active, a, b)) {
            merges[k] = SquashMerge{SQUASH_NONE, SQUASH_NONE, 0, 0, 0.0};
            continue;
        }
        const double d = D[(uint64_t)a * S + b];
        squash_merge_profiles(B, size[a], size[b], u + (uint64_t)a * B, v + (uint64_t)a * B, u + (uint64_t)b * B, v + (uint64_t)b * B);
        size[a] += size[b];
        active[b] = 0;
        merges[k] = SquashMerge{a, b, size[a], 0, d};
        n_merges++;
        row_step(a);
    }
    return n_merges;
}

// ------------------------------------------------------------------------------------------------
// Edge principal components (include/rappas_place.h holds the definition, steps 1 - 8): the host twin of the epca kernels of
// rk_epca.h, and the one finish (the only square roots) behind rk_epca_finish_host.  Profiles and the centred matrix lie sample
// after sample, B doubles each; the column blocks Q, Y, Z are [k][S]; G is [S][S].
// ------------------------------------------------------------------------------------------------
constexpr uint32_t EPCA_LANES = 64, EPCA_MAX_SAMPLES = 4096, EPCA_MAX_COMPONENTS = 8, EPCA_MAX_ITERS = 10000;

inline uint64_t epca_out_doubles(uint32_t B, uint32_t S, uint32_t k) { return 1 + (uint64_t)k * (3 + (uint64_t)S + B); }

// LS(f): 64 sequential lane sums from +0.0 over s = l, l + 64, ..., added in ascending lane order onto +0.0
template <class F>
inline double lane_sum(uint32_t S, F &&f) {
    double p[EPCA_LANES];
    for (uint32_t l = 0; l < EPCA_LANES; l++) {
        double a = 0.0;
        for (uint32_t s = l; s < S; s += EPCA_LANES) a = a + f(s);
        p[l] = a;
    }
    double r = 0.0;
    for (uint32_t l = 0; l < EPCA_LANES; l++) r = r + p[l];
    return r;
}
inline double epca_dot(uint32_t S, const double *a, const double *b) {
    return lane_sum(S, [&](uint32_t s) { const double t = a[s] * b[s]; return t; });
}

// Steps 2 and 3 for the nodes x = x_lo, x_lo + x_step, ...: xc[s * B + x] from the profiles and the active flags (n of them set)
inline void epca_centre(uint32_t B, uint32_t S, uint32_t root, const uint8_t *active, uint32_t n, const double *u, const double *v, uint32_t x_lo, uint32_t x_step,
                        double *xc) {
    for (uint64_t x = x_lo; x < B; x += x_step) {
        auto X = [&](uint32_t s) { return active[s] && x != root ? (u[s * (uint64_t)B + x] + v[s * (uint64_t)B + x]) - 1.0 : 0.0; };
        const double mean = lane_sum(S, X) / (double)n;
        for (uint32_t s = 0; s < S; s++) xc[s * (uint64_t)B + x] = active[s] && x != root ? X(s) - mean : 0.0;
    }
}

// G[s][t] from the centred rows of the two samples: the same walk, acc = acc + (a * b)
inline double epca_gram_pair(uint32_t B, const double *xs, const double *xt) {
    return chunk_walk(B, [&](double acc, uint32_t x) { return gram_term(acc, xs[x], xt[x]); });
}

// Rows s = s_lo, s_lo + s_step, ... of G: the pairs (s, t >= s), each written at [s][t] and [t][s]
inline void epca_gram_rows(uint32_t B, uint32_t S, const double *xc, uint32_t s_lo, uint32_t s_step, double *G) {
    for (uint64_t s = s_lo; s < S; s += s_step)
        for (uint64_t t = s; t < S; t++) {
            const double g = epca_gram_pair(B, xc + s * B, xc + t * B);
            G[s * S + t] = g;
            G[t * S + s] = g;
        }
}

inline double epca_start(uint32_t s, uint32_t j) { return (double)((s * 8u + j + 1u) * 2654435761u) / 4294967296.0 - 0.5; }

// out[j][s] = LS(t -> G[s][t] * in[j][t]) for j < k_eff
inline void epca_multiply(uint32_t S, uint32_t k_eff, const double *G, const double *in, double *out) {
    for (uint32_t j = 0; j < k_eff; j++)
        for (uint64_t s = 0; s < S; s++) out[j * (uint64_t)S + s] = epca_dot(S, G + s * S, in + j * (uint64_t)S);
}

// the smallest index with the largest fabs of a column (plain >), and that fabs
inline uint32_t epca_largest(uint32_t S, const double *y, double *best) {
    uint32_t i = 0;
    *best = std::fabs(y[0]);
    for (uint32_t s = 1; s < S; s++)
        if (std::fabs(y[s]) > *best) {
            *best = std::fabs(y[s]);
            i = s;
        }
    return i;
}

// Step 6 behind the product: the columns of Y scaled by their largest element and made orthogonal, in column order; a column that
// its projections have left with nothing but their rounding (the zero rule of step 6; not in the first iteration, whose columns come
// from the start vectors) becomes +0.0 and is projected on by nobody
inline void epca_orth(uint32_t S, uint32_t k_eff, bool first, double *Y) {
    double top0[EPCA_MAX_COMPONENTS];  // the largest fabs of every column as the product delivered it
    for (uint32_t j = 0; j < k_eff; j++) epca_largest(S, Y + j * (uint64_t)S, &top0[j]);
    uint32_t applied = 0;  // the projections column j has been through: the live columns before it
    double scale = 0.0;    // the largest top0 of those live columns
    for (uint32_t j = 0; j < k_eff; j++) {
        double *yj = Y + j * (uint64_t)S;
        double best;
        const uint32_t i = epca_largest(S, yj, &best);
        if (best <= epca_noise_bound(S, first ? 0u : applied, top0[j] > scale ? top0[j] : scale)) {
            for (uint32_t s = 0; s < S; s++) yj[s] = 0.0;
            continue;
        }
        applied++;
        if (top0[j] > scale) scale = top0[j];
        const double pivot = yj[i];
        for (uint32_t s = 0; s < S; s++) yj[s] = yj[s] / pivot;
        const double nn = epca_dot(S, yj, yj);
        for (uint32_t l = j + 1; l < k_eff; l++) {
            double *yl = Y + l * (uint64_t)S;
            const double d = epca_dot(S, yj, yl) / nn;
            for (uint32_t s = 0; s < S; s++) {
                const double t = d * yj[s];
                yl[s] = yl[s] - t;
            }
        }
    }
}

// Steps 5 - 8 over G and the centred matrix: the raw output.  work: 2 * k * S doubles.  k_eff > 0.
inline void epca_iterate(uint32_t B, uint32_t S, uint32_t k, uint32_t k_eff, uint32_t iters, const double *G, const double *xc, double *work, double *raw) {
    double *q = work, *y = work + (uint64_t)k * S;
    for (uint32_t j = 0; j < k_eff; j++)
        for (uint32_t s = 0; s < S; s++) q[j * (uint64_t)S + s] = epca_start(s, j);
    for (uint32_t it = 0; it < iters; it++) {
        epca_multiply(S, k_eff, G, q, y);
        epca_orth(S, k_eff, it == 0, y);
        std::swap(q, y);
    }
    double *z = y;
    epca_multiply(S, k_eff, G, q, z);
    double *lambda = raw + 1, *nn = lambda + k, *rr = nn + k, *q_out = rr + k, *w_out = q_out + (uint64_t)k * S;
    raw[0] = lane_sum(S, [&](uint32_t s) { return G[(uint64_t)s * S + s]; });
    for (uint32_t j = 0; j < k_eff; j++) {
        const double *qj = q + j * (uint64_t)S, *zj = z + j * (uint64_t)S;
        nn[j] = epca_dot(S, qj, qj);
        if (nn[j] == 0.0) {
            nn[j] = lambda[j] = rr[j] = 0.0;
        } else {
            const double lam = epca_dot(S, qj, zj) / nn[j];
            lambda[j] = lam;
            rr[j] = lane_sum(S, [&](uint32_t s) {
                const double t = lam * qj[s], r = zj[s] - t, r2 = r * r;
                return r2;
            });
        }
        for (uint32_t s = 0; s < S; s++) q_out[j * (uint64_t)S + s] = qj[s];
        for (uint64_t x = 0; x < B; x++)
            w_out[j * (uint64_t)B + x] = lane_sum(S, [&](uint32_t s) { const double t = xc[s * (uint64_t)B + x] * qj[s]; return t; });
    }
}

// Finish: what a caller reads, from the raw output (rk_epca_finish_host)
inline void epca_finish(uint32_t B, uint32_t S, uint32_t k, const double *raw, double *eigenvalue, double *share, double *residual, double *projection,
                        double *loading) {
    const double trace = raw[0], *lambda = raw + 1, *nn = lambda + k, *rr = nn + k, *q = rr + k, *w = q + (uint64_t)k * S;
    for (uint32_t j = 0; j < k; j++) {
        const bool on = lambda[j] > 0.0 && nn[j] != 0.0;
        eigenvalue[j] = on ? lambda[j] : 0.0;
        share[j] = on ? lambda[j] / trace : 0.0;
        residual[j] = on ? std::sqrt(rr[j] / nn[j]) : 0.0;
        const double ps = on ? std::sqrt(lambda[j] / nn[j]) : 0.0, ls = on ? std::sqrt(lambda[j] * nn[j]) : 1.0;
        for (uint64_t s = 0; s < S; s++) projection[s * k + j] = on ? q[j * (uint64_t)S + s] * ps : 0.0;
        for (uint64_t x = 0; x < B; x++) loading[x * k + j] = on ? w[j * (uint64_t)B + x] / ls : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// EDPL: the distance between two branches and the pair sum of a read, as include/rappas_place.h defines them.  The
// tables are built once here, for rk_tree_create (which uploads them as they are) and for the host twins alike.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t EDPL_MAX_K = 16;

// what a row of a read needs of its branch: pos, the root distance of the midpoint of the edge above it, and its pre-order interval
struct EdplNode {
    double pos;
    uint32_t pre, end;
};

// node[B] by node id; lca: one block of 8-byte words that holds, by pre-order position p,
//   dpar[B]  binary64: D of the parent of the node at p (the root: +0.0) -- the D[l] of a pair whose shallowest node between them sits at p
//   depth[B] 16-bit
//   table[levels][B] 16-bit: table[j][p] = a position of least depth among p .. p + 2^j - 1 (clamped to B - 1); table[0][p] = p
// levels = floor(log2(B - 1)) + 1 for B >= 2, 0 for B == 1: a range of B - 1 positions is the longest a query has.
struct TreeDist {
    uint32_t B = 0, levels = 0;
    std::vector<EdplNode> node;
    std::vector<uint64_t> lca;
    const double *dpar() const { return (const double *)lca.data(); }
    const uint16_t *depth() const { return (const uint16_t *)(lca.data() + B); }
    const uint16_t *table() const { return depth() + B; }
};

inline uint32_t edpl_levels(uint32_t B) {
    uint32_t levels = 0;
    while (B >= 2 && (1u << levels) <= B - 1) levels++;
    return levels;
}
// 8-byte words of the block of B positions
inline uint64_t edpl_lca_words(uint32_t B) { return (uint64_t)B + ((uint64_t)B * 2 * (1 + edpl_levels(B)) + 7) / 8; }

// D[x] = D[parent[x]] + (double)branch_len[x] along the pre-order (a parent is met before its children), pos[x] = D[x] - h[x]
inline void tree_dist_build(const TreeWalk &w, const int32_t *parent, const float *branch_len, TreeDist &t) {
    const uint32_t B = (uint32_t)w.node_at.size(), levels = edpl_levels(B);
    t.B = B;
    t.levels = levels;
    t.node.assign(B, EdplNode{0.0, 0, 0});
    t.lca.assign(edpl_lca_words(B), 0);
    double *dpar = (double *)t.lca.data();
    uint16_t *depth = (uint16_t *)(t.lca.data() + B), *table = depth + B;
    std::vector<double> D(B, 0.0);
    for (uint32_t p = 0; p < B; p++) {
        const uint32_t x = w.node_at[p];
        if (p) {
            const uint32_t up = (uint32_t)parent[x];
            D[x] = D[up] + (double)branch_len[x];
            dpar[p] = D[up];
            depth[p] = (uint16_t)(depth[w.pre[up]] + 1);
        }
        t.node[x] = EdplNode{D[x] - kr_half_length(branch_len, x, w.root), p, p + w.size[x]};
        table[p] = (uint16_t)p;
    }
    for (uint32_t j = 1; j < levels; j++) {
        const uint16_t *below = table + (uint64_t)(j - 1) * B;
        uint16_t *row = table + (uint64_t)j * B;
        for (uint32_t p = 0; p < B; p++) {
            const uint32_t q = p + (1u << (j - 1)) < B ? p + (1u << (j - 1)) : B - 1;
            row[p] = depth[below[q]] < depth[below[p]] ? below[q] : below[p];
        }
    }
}

// d(a, b) of two nodes given by their EdplNode: the one met first in the pre-order either holds the other in its interval (it is the
// ancestor) or the two meet at the parent of a shallowest node among the positions behind the first, up to the second.
inline double tree_distance(const EdplNode &a, const EdplNode &b, uint32_t B, const double *dpar, const uint16_t *depth, const uint16_t *table) {
    if (a.pre == b.pre) return 0.0;
    const EdplNode &f = a.pre < b.pre ? a : b, &s = a.pre < b.pre ? b : a;
    if (s.pre < f.end) return s.pos - f.pos;
    const uint32_t len = s.pre - f.pre, j = 31u - (uint32_t)__builtin_clz(len);
    const uint16_t *row = table + (uint64_t)j * B;
    const uint32_t c1 = row[f.pre + 1], c2 = row[s.pre + 1 - (1u << j)];
    const double dl = dpar[depth[c2] < depth[c1] ? c2 : c1];
    return (a.pos - dl) + (b.pos - dl);
}

// edpl[r] of one read: its first n rows (n = min(n_rows, K)), the usable ones in row order
inline double edpl_read(const TreeDist &t, uint32_t n, const uint16_t *branch, const double *lwr) {
    const double *dpar = t.dpar();
    const uint16_t *depth = t.depth(), *table = t.table();
    double acc = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        if (!(branch[i] < t.B && lwr[i] > 0.0)) continue;
        for (uint32_t j = i + 1; j < n; j++) {
            if (!(branch[j] < t.B && lwr[j] > 0.0)) continue;
            const double ww = lwr[i] * lwr[j], d = tree_distance(t.node[branch[i]], t.node[branch[j]], t.B, dpar, depth, table);
            const double term = ww * d;
            acc = acc + term;
        }
    }
    return 2.0 * acc;
}

inline void edpl_range(const TreeDist &t, uint32_t K, uint64_t r_lo, uint64_t r_hi, const uint8_t *n_rows, const uint16_t *branch, const double *lwr, double *edpl) {
    for (uint64_t r = r_lo; r < r_hi; r++) edpl[r] = edpl_read(t, n_rows[r] < K ? n_rows[r] : K, branch + r * K, lwr + r * K);
}

// ------------------------------------------------------------------------------------------------
// Phylogenetic k-means (include/rappas_place.h holds the definition): the host twin of the kernels of rk_kmeans.h.
// Profiles lie sample after sample, B doubles each; the centroid profiles cu, cv cluster after cluster, B doubles each; Dc is [k][S].
// ------------------------------------------------------------------------------------------------
constexpr uint32_t KMEANS_NONE = 0xFFFFFFFFu, KMEANS_GROUP = 256, KMEANS_MAX_K = 64, KMEANS_MAX_ROUNDS = 1024;

struct KmeansOut {  // the outputs of a run; centroids may be nullptr
    uint32_t *assign;
    double *dist;
    uint32_t *sizes;
    double *within;
    uint32_t *info;
    double *centroids;
};

// every output as its filler, info = {k_eff, n_active, 0 rounds, converged | status << 1}
inline void kmeans_fill(uint32_t B, uint32_t S, uint32_t k, uint32_t k_eff, uint32_t n_active, uint32_t status, const KmeansOut &o) {
    for (uint32_t s = 0; s < S; s++) {
        o.assign[s] = KMEANS_NONE;
        o.dist[s] = 0.0;
    }
    for (uint32_t j = 0; j < k; j++) {
        o.sizes[j] = 0;
        o.within[j] = 0.0;
    }
    if (o.centroids)
        for (uint64_t i = 0; i < (uint64_t)k * 2 * B; i++) o.centroids[i] = 0.0;
    o.info[0] = k_eff;
    o.info[1] = n_active;
    o.info[2] = 0;
    o.info[3] = 1u | status << 1;
}

// Dc[j][s] for the centroids j_lo <= j < j_hi and the active samples s = s_lo, s_lo + s_step, ...: the centroid is the first operand
inline void kmeans_distances(uint32_t B, uint32_t S, const double *h, const double *u, const double *v, const uint8_t *active, const double *cu, const double *cv,
                             uint32_t j_lo, uint32_t j_hi, uint32_t s_lo, uint32_t s_step, double *Dc) {
    for (uint64_t j = j_lo; j < j_hi; j++)
        for (uint64_t s = s_lo; s < S; s += s_step)
            if (active[s]) Dc[j * S + s] = kr_pair(B, h, cu + j * B, cv + j * B, u + s * B, v + s * B);
}

// Farthest-first seeds 1 .. k_eff - 1 behind seed_0 = the smallest active sample; every seed's profile becomes its cluster's centroid.
// dist_step(j_lo, j_hi) fills rows j_lo .. j_hi - 1 of Dc: kmeans_distances over every s, dealt as the caller likes.
template <class DistStep>
inline void kmeans_seed(uint32_t B, uint32_t S, uint32_t k_eff, const double *u, const double *v, const uint8_t *active, double *cu, double *cv, const double *Dc,
                        uint32_t *seeds, DistStep &&dist_step) {
    std::vector<double> mind(S, 0.0);
    std::vector<uint8_t> is_seed(S, 0);
    auto take = [&](uint32_t j, uint32_t s) {
        seeds[j] = s;
        is_seed[s] = 1;
        for (uint64_t x = 0; x < B; x++) {
            cu[j * (uint64_t)B + x] = u[s * (uint64_t)B + x];
            cv[j * (uint64_t)B + x] = v[s * (uint64_t)B + x];
        }
    };
    uint32_t s0 = 0;
    while (!active[s0]) s0++;
    take(0, s0);
    for (uint32_t j = 1; j < k_eff; j++) {
        dist_step(j - 1, j);
        const double *row = Dc + (uint64_t)(j - 1) * S;
        uint32_t best = KMEANS_NONE;
        for (uint32_t s = 0; s < S; s++) {
            if (!active[s]) continue;
            mind[s] = (j == 1 || row[s] < mind[s]) ? row[s] : mind[s];
            if (!is_seed[s] && (best == KMEANS_NONE || mind[s] > mind[best])) best = s;
        }
        take(j, best);
    }
}

// assign[s] = the nearest centroid of every active s (plain <, ties to the smaller j), dist[s] its distance; returns `changed`
inline uint32_t kmeans_assign(uint32_t S, uint32_t k_eff, const double *Dc, const uint8_t *active, uint32_t *assign, double *dist) {
    uint32_t changed = 0;
    for (uint32_t s = 0; s < S; s++) {
        if (!active[s]) continue;
        uint32_t best = 0;
        for (uint32_t j = 1; j < k_eff; j++)
            if (Dc[(uint64_t)j * S + s] < Dc[(uint64_t)best * S + s]) best = j;
        changed += assign[s] != best;
        assign[s] = best;
        dist[s] = Dc[(uint64_t)best * S + s];
    }
    return changed;
}

// The new centroids of the clusters j = j_lo, j_lo + j_step, ... < k_eff: the members in ascending s, one partial a group of
// KMEANS_GROUP sample indices from +0.0, the partials of the groups that hold a member in group order, then the division.  A cluster
// without members keeps its profile.
inline void kmeans_update(uint32_t B, uint32_t S, uint32_t k_eff, const double *u, const double *v, const uint32_t *assign, uint32_t j_lo, uint32_t j_step, double *cu,
                          double *cv) {
    std::vector<double> pu(B), pv(B), su(B), sv(B);
    for (uint64_t j = j_lo; j < k_eff; j += j_step) {
        uint32_t n = 0;
        for (uint32_t g0 = 0; g0 < S; g0 += KMEANS_GROUP) {
            uint32_t in_group = 0;
            for (uint64_t s = g0; s < S && s < g0 + KMEANS_GROUP; s++) {
                if (assign[s] != j) continue;
                if (!in_group++)
                    for (uint32_t x = 0; x < B; x++) pu[x] = pv[x] = 0.0;
                for (uint32_t x = 0; x < B; x++) {
                    pu[x] = pu[x] + u[s * B + x];
                    pv[x] = pv[x] + v[s * B + x];
                }
            }
            if (!in_group) continue;
            for (uint32_t x = 0; x < B; x++) {
                su[x] = n ? su[x] + pu[x] : pu[x];
                sv[x] = n ? sv[x] + pv[x] : pv[x];
            }
            n += in_group;
        }
        if (!n) continue;
        const double nn = (double)n;
        for (uint32_t x = 0; x < B; x++) {
            cu[j * B + x] = su[x] / nn;
            cv[j * B + x] = sv[x] / nn;
        }
    }
}

// The rounds behind the start (cu, cv hold the seeds' profiles), then sizes, within, info and the centroids.  dist_step(j_lo, j_hi)
// as in kmeans_seed; update_step() gives every cluster its new centroid: kmeans_update over every j, dealt as the caller likes.
template <class DistStep, class UpdateStep>
inline void kmeans_rounds(uint32_t B, uint32_t S, uint32_t k, uint32_t k_eff, uint32_t n_active, uint32_t max_rounds, const uint8_t *active, const double *cu,
                          const double *cv, const double *Dc, const KmeansOut &o, DistStep &&dist_step, UpdateStep &&update_step) {
    kmeans_fill(B, S, k, k_eff, n_active, 0, o);
    uint32_t rounds = 0, converged = 0;
    while (rounds < max_rounds && !converged) {
        dist_step(0, k_eff);
        const uint32_t changed = kmeans_assign(S, k_eff, Dc, active, o.assign, o.dist);
        rounds++;
        if (changed == 0) converged = 1;
        else update_step();
    }
    for (uint32_t s = 0; s < S; s++)
        if (active[s]) {
            o.sizes[o.assign[s]]++;
            o.within[o.assign[s]] = o.within[o.assign[s]] + o.dist[s];
        }
    o.info[2] = rounds;
    o.info[3] = converged;
    if (o.centroids)
        for (uint64_t j = 0; j < k_eff; j++)
            for (uint64_t x = 0; x < B; x++) {
                o.centroids[(j * 2) * B + x] = cu[j * B + x];
                o.centroids[(j * 2 + 1) * B + x] = cv[j * B + x];
            }
}

// ------------------------------------------------------------------------------------------------
// Per-sample diversity measures (include/rappas_place.h holds the definition): the host twin of the kernels of
// rk_diversity.h.  The terms are those of rk_divmath.h, the text the kernel compiles; the order of the sum is written out here.
// ------------------------------------------------------------------------------------------------
// The row of one sample from its masses and clade sums: per chunk of KR_CHUNK ids DIVERSITY_LANES lane partials, lane j over the
// nodes base + j, base + j + 256, ..., folded by halving; the chunks in order, the first one as it is.  T == 0: the NaN row.
template <uint32_t NT>
inline void diversity_row(uint32_t B, uint32_t root, const uint64_t *mass, const uint64_t *c, const double *h, const double *theta, double *out) {
    constexpr uint32_t C = DIVERSITY_FIXED + 2 * NT;
    const uint64_t T = c[root];
    if (T == 0) {
        for (uint32_t i = 0; i < C; i++) out[i] = divmath_double(DIVERSITY_NAN);
        return;
    }
    std::vector<double> lanes((size_t)DIVERSITY_LANES * C);
    for (uint32_t x0 = 0; x0 < B; x0 += KR_CHUNK) {
        const uint32_t x1 = x0 + KR_CHUNK < B ? x0 + KR_CHUNK : B;
        for (uint32_t j = 0; j < DIVERSITY_LANES; j++) {
            double *acc = lanes.data() + (size_t)j * C;
            for (uint32_t i = 0; i < C; i++) acc[i] = 0.0;
            for (uint32_t x = x0 + j; x < x1; x += DIVERSITY_LANES) diversity_node<NT>(c[x], mass[x], T, h[x], theta, acc);
        }
        for (uint32_t stride = DIVERSITY_LANES / 2; stride > 0; stride >>= 1)
            for (uint32_t j = 0; j < stride; j++)
                for (uint32_t i = 0; i < C; i++) lanes[(size_t)j * C + i] = lanes[(size_t)j * C + i] + lanes[(size_t)(j + stride) * C + i];
        for (uint32_t i = 0; i < C; i++) out[i] = chunk_fold(x0 == 0, out[i], lanes[i]);
    }
}

inline void diversity_sample(uint32_t B, uint32_t root, const uint64_t *mass, const uint64_t *c, const double *h, uint32_t n_theta, const double *theta, double *out) {
    switch (n_theta) {
    case 0: return diversity_row<0>(B, root, mass, c, h, theta, out);
    case 1: return diversity_row<1>(B, root, mass, c, h, theta, out);
    case 2: return diversity_row<2>(B, root, mass, c, h, theta, out);
    case 3: return diversity_row<3>(B, root, mass, c, h, theta, out);
    case 4: return diversity_row<4>(B, root, mass, c, h, theta, out);
    case 5: return diversity_row<5>(B, root, mass, c, h, theta, out);
    case 6: return diversity_row<6>(B, root, mass, c, h, theta, out);
    case 7: return diversity_row<7>(B, root, mass, c, h, theta, out);
    default: return diversity_row<8>(B, root, mass, c, h, theta, out);
    }
}

// what every diversity call tests of its thetas; 0, or -1 with a message
inline int diversity_theta_args(const char *who, uint32_t n_theta, const double *theta, char *msg, size_t msg_len) {
    if (n_theta && !theta) {
        snprintf(msg, msg_len, "%s: null theta array with n_theta=%u", who, n_theta);
        return -1;
    }
    for (uint32_t i = 0; i < n_theta; i++)
        if (!(theta[i] >= 0.0 && theta[i] <= 8.0)) {
            snprintf(msg, msg_len, "%s: theta[%u]=%g must be in 0..8", who, i, theta[i]);
            return -1;
        }
    return 0;
}

}  // namespace rk
