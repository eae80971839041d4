// rk_samples.h -- #included by rk_kernels.hip: the sample-level kernels -- the clade sums of sample mass buffers
// over a tree on the device, the pairwise Kantorovich-Rubinstein distances between the samples, and the squash clustering of the
// samples over those distances.  The launches and the entry points
// are in rk_samples_impl.h, the host twins in rk_samples_host.h.  Not part of the C ABI.
#pragma once
#include "rk_device.h"
#include "rk_samplemath.h"

namespace rk {

// ------------------------------------------------------------------------------------------------
// clade_masses_kernel: clade[s][x] = the sum of mass_q30 of sample s over x's subtree.  In pre-order a subtree is an interval, so
// with E[p] = the sum of the masses at the positions below p the answer is E[pre + size] - E[pre]: exact in 64-bit integers.
// One block per sample walks the B positions in chunks of CLADE_CHUNK: a thread gathers CLADE_ITEMS consecutive positions, the
// thread sums are scanned across the wave by shuffles, the four wave sums meet in the LDS, a carry runs from chunk to chunk; the
// chunk's E lies in the LDS (CLADE_CHUNK + 1 words: both ends of the chunk).  A node whose interval ends inside the chunk it starts
// in is written at once.  A node that spans chunks -- few on a bushy tree, nearly all on a caterpillar -- is written as 0 - E[pre]
// in the chunk of its start and receives + E[pre + size] in the chunk of its end (modulo 2^64 the sum is the difference): the host
// lists those nodes ordered by the chunk of their end (span_node, span_end, span_off[chunk]), the same block does both steps with a
// barrier between any two chunks, so no other scratch is needed and the output is written, never added into from outside.
// No 64-bit shift anywhere.
// ------------------------------------------------------------------------------------------------
constexpr u32 CLADE_ITEMS = 8, CLADE_CHUNK = 256 * CLADE_ITEMS;

__global__ void __launch_bounds__(256) clade_masses_kernel(u32 B, u64 W, const u32 *node_at, const u32 *end_at, const u32 *span_node, const u32 *span_end,
                                                           const u32 *span_off, const u64 *masses, u64 *clade) {
    __shared__ u64 E[CLADE_CHUNK + 1];
    __shared__ u64 wave_sum[4];
    const u64 *m = masses + (u64)blockIdx.x * W;
    u64 *out = clade + (u64)blockIdx.x * B;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 carry = 0;
    for (u32 c0 = 0, c = 0; c0 < B; c0 += CLADE_CHUNK, c++) {
        const u32 base = c0 + tid * CLADE_ITEMS;
        u64 v[CLADE_ITEMS], t = 0;
        u32 node[CLADE_ITEMS];
#pragma unroll
        for (u32 i = 0; i < CLADE_ITEMS; i++) {
            const u32 p = base + i;
            node[i] = p < B ? node_at[p] : 0u;
            v[i] = p < B ? m[node[i]] : 0ull;
            t += v[i];
        }
        u64 inc = t;  // inclusive scan of the thread sums across the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 y = __shfl_up(inc, o, 64);
            if (lane >= (u32)o) inc += y;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        u64 before = carry, total = 0;
#pragma unroll
        for (u32 w = 0; w < 4; w++) {
            const u64 ws = wave_sum[w];
            if (w < wave) before += ws;
            total += ws;
        }
        u64 e = before + inc - t;
#pragma unroll
        for (u32 i = 0; i < CLADE_ITEMS; i++) {
            E[tid * CLADE_ITEMS + i] = e;
            e += v[i];
        }
        if (tid == 255) E[CLADE_CHUNK] = e;  // (positions beyond B add nothing: every E behind the last one holds the sample's total)
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < CLADE_ITEMS; i++) {
            const u32 p = base + i;
            if (p < B) {
                const u32 q = end_at[p];  // pre + size: in p + 1 .. B
                const u64 lo = E[p - c0];
                out[node[i]] = q <= c0 + CLADE_CHUNK ? E[q - c0] - lo : 0ull - lo;
            }
        }
        for (u32 k = span_off[c] + tid; k < span_off[c + 1]; k += 256) out[span_node[k]] += E[span_end[k] - c0];  // (started in an earlier chunk)
        carry += total;
        __syncthreads();  // E and wave_sum are free again; the writes of this chunk lie before the next one's
    }
}

// ------------------------------------------------------------------------------------------------
// The KR distance matrix (include/rappas_place.h holds the definition and the order of the sum).
//
// kr_profiles_kernel: u[x][s] = c_s(x) / T_s and v[x][s] = (c_s(x) - m_s(x)) / T_s, node-major (the pair kernel loads 64 samples of
// one node as one 512-byte line).  A block transposes a tile of 32 nodes x 32 samples through the LDS: the clade sums and the masses
// are read along the nodes, the profiles written along the samples.  binary64, IEEE conversion and division.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) kr_profiles_kernel(u32 B, u32 S, u64 W, u32 root, const u64 *masses, const u64 *clade, double *U, double *V) {
    __shared__ double tu[32][33], tv[32][33];
    const u32 i = threadIdx.x & 31, j = threadIdx.x >> 5;
    const u32 x0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
#pragma unroll
    for (u32 jj = 0; jj < 4; jj++) {
        const u32 sl = j + 8 * jj, s = s0 + sl, x = x0 + i;
        if (s < S && x < B) {
            const u64 c = clade[(u64)s * B + x], mm = masses[(u64)s * W + x];
            const double T = (double)clade[(u64)s * B + root];
            tu[sl][i] = (double)c / T;
            tv[sl][i] = (double)(c - mm) / T;
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 jj = 0; jj < 4; jj++) {
        const u32 xl = j + 8 * jj, x = x0 + xl, s = s0 + i;
        if (s < S && x < B) {
            U[(u64)x * S + s] = tu[i][xl];
            V[(u64)x * S + s] = tv[i][xl];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// kr_pairs_kernel: a distance-matrix GEMM without MFMA (fabs sits inside the sum).  A block of 256 threads owns a tile of 64 x 64
// sample pairs on or above the diagonal (blockIdx.x counts those tiles row by row) and the chunks [blockIdx.y * chunks_per_block,
// + chunks_per_block) of RK_KR_CHUNK node ids.  Per stage of KR_STAGE nodes the profiles of the tile's 64 row samples and 64 column
// samples go through the LDS (the next stage's loads are in flight in registers while this one is summed); a thread keeps a 4 x 4
// micro-tile of pairs -- rows 2ty, 2ty + 1, 32 + 2ty, 33 + 2ty, columns likewise from tx, so that the 16 lanes of a ds_read_b128
// group read 256 contiguous bytes of the columns and one or two addresses of the rows -- and walks the nodes in ascending id:
// acc = (acc + h * |u_s - u_t|) + h * |v_s - v_t| (kr_term of rk_samplemath.h), three FP64 operations a term (no contraction).
// A chunk's partial starts at +0.0.  With to_part == 0 the block holds every chunk and folds the partials by the chunk rule
// (chunk_fold) into D; otherwise it writes each partial to part[chunk] (S x S doubles each) and kr_reduce_kernel adds them by the
// same rule.  Either way an entry and its mirror are written by the one thread that summed the pair: no atomics, and the bits depend on
// neither grid nor tile.  A diagonal tile sums both triangles (|a - b| == |b - a|: the same bits) and writes no mirror.
// epca_gram_kernel (rk_epca.h) is this kernel with one staged matrix.  One frame under both was built and measured
// (profiles/sample_frames_rates.txt): this kernel ran 5 - 7 % slower through it, with the stage loop's instructions unchanged but
// for the register numbers, so the two stay two texts until that is understood; the terms and the chunk rule are shared.
// ------------------------------------------------------------------------------------------------
constexpr u32 KR_TILE = 64, KR_STAGE = 8, KR_CHUNK_IDS = 2048;

__global__ void __launch_bounds__(256) kr_pairs_kernel(u32 B, u32 S, u32 n_tiles_side, u32 chunks_per_block, u32 to_part, const double *U, const double *V,
                                                       const double *h, double *D, double *part) {
    __shared__ __attribute__((aligned(16))) double st[KR_STAGE * 256];  // [node][u | v][rows | columns][64]
    // the tile: rows of tiles on or above the diagonal, n, n - 1, ... tiles long
    u32 ti = 0, rem = blockIdx.x;
    while (rem >= n_tiles_side - ti) {
        rem -= n_tiles_side - ti;
        ti++;
    }
    const u32 tj = ti + rem;
    const u32 r0 = ti * KR_TILE, c0 = tj * KR_TILE;
    const u32 tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // what this thread loads of every node of a stage: sample `ls` of the rows or the columns, from u or from v
    const u32 lj = tid & 63, l_col = (tid >> 6) & 1, l_v = tid >> 7;
    const u32 ls = (l_col ? c0 : r0) + lj;
    const double *src = (l_v ? V : U) + ls;
    const bool l_ok = ls < S;
    const u32 n_chunks = (B + KR_CHUNK_IDS - 1) / KR_CHUNK_IDS;
    const u32 ch_lo = blockIdx.y * chunks_per_block, ch_hi = min(ch_lo + chunks_per_block, n_chunks);
    double d[4][4] = {};
    for (u32 ch = ch_lo; ch < ch_hi; ch++) {
        const u32 x_lo = ch * KR_CHUNK_IDS, x_hi = min(x_lo + KR_CHUNK_IDS, B);
        double acc[4][4];
#pragma unroll
        for (u32 a = 0; a < 4; a++)
#pragma unroll
            for (u32 b = 0; b < 4; b++) acc[a][b] = 0.0;
        double nxt[KR_STAGE];
#pragma unroll
        for (u32 k = 0; k < KR_STAGE; k++) nxt[k] = l_ok && x_lo + k < x_hi ? src[(u64)(x_lo + k) * S] : 0.0;
        for (u32 x0 = x_lo; x0 < x_hi; x0 += KR_STAGE) {
            __syncthreads();  // the stage before this one has been read
#pragma unroll
            for (u32 k = 0; k < KR_STAGE; k++) st[k * 256 + tid] = nxt[k];
            __syncthreads();
            const u32 x1 = x0 + KR_STAGE;
#pragma unroll
            for (u32 k = 0; k < KR_STAGE; k++) nxt[k] = l_ok && x1 + k < x_hi ? src[(u64)(x1 + k) * S] : 0.0;
            const u32 nk = min(KR_STAGE, x_hi - x0);
#pragma unroll 1
            for (u32 k = 0; k < nk; k++) {
                const double hx = h[x0 + k];  // (uniform: a scalar load)
                const double *b = st + k * 256;
                double ru[4], cu[4], rv[4], cv[4];
#pragma unroll
                for (u32 g = 0; g < 2; g++) {
                    const double2 a0 = *(const double2 *)(b + g * 32 + 2 * ty), a1 = *(const double2 *)(b + 64 + g * 32 + 2 * tx);
                    const double2 a2 = *(const double2 *)(b + 128 + g * 32 + 2 * ty), a3 = *(const double2 *)(b + 192 + g * 32 + 2 * tx);
                    ru[2 * g] = a0.x; ru[2 * g + 1] = a0.y;
                    cu[2 * g] = a1.x; cu[2 * g + 1] = a1.y;
                    rv[2 * g] = a2.x; rv[2 * g + 1] = a2.y;
                    cv[2 * g] = a3.x; cv[2 * g + 1] = a3.y;
                }
#pragma unroll
                for (u32 a = 0; a < 4; a++)
#pragma unroll
                    for (u32 bb = 0; bb < 4; bb++) acc[a][bb] = kr_term(acc[a][bb], hx, ru[a], cu[bb], rv[a], cv[bb]);
            }
        }
        if (to_part) {
            double *dst = part + (u64)ch * S * S;
#pragma unroll
            for (u32 a = 0; a < 4; a++)
#pragma unroll
                for (u32 bb = 0; bb < 4; bb++) {
                    const u32 s = r0 + (a >> 1) * 32 + 2 * ty + (a & 1), t = c0 + (bb >> 1) * 32 + 2 * tx + (bb & 1);
                    if (s < S && t < S) {
                        dst[(u64)s * S + t] = acc[a][bb];
                        if (ti != tj) dst[(u64)t * S + s] = acc[a][bb];
                    }
                }
        } else {
#pragma unroll
            for (u32 a = 0; a < 4; a++)
#pragma unroll
                for (u32 bb = 0; bb < 4; bb++) d[a][bb] = chunk_fold(ch == ch_lo, d[a][bb], acc[a][bb]);
        }
    }
    if (!to_part && ch_lo < ch_hi) {
#pragma unroll
        for (u32 a = 0; a < 4; a++)
#pragma unroll
            for (u32 bb = 0; bb < 4; bb++) {
                const u32 s = r0 + (a >> 1) * 32 + 2 * ty + (a & 1), t = c0 + (bb >> 1) * 32 + 2 * tx + (bb & 1);
                if (s < S && t < S) {
                    D[(u64)s * S + t] = d[a][bb];
                    if (ti != tj) D[(u64)t * S + s] = d[a][bb];
                }
            }
    }
}

// D[i] = the partials of entry i by the chunk rule: the entries of both triangles hold the same partials
__global__ void __launch_bounds__(256) kr_reduce_kernel(u64 n, u32 n_chunks, const double *part, double *D) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    D[i] = chunk_sum(n_chunks, [&](u32 c) { return part[(u64)c * n + i]; });
}

// ------------------------------------------------------------------------------------------------
// Squash clustering (include/rappas_place.h holds the definition).  After the KR matrix the profiles U, V, the half
// lengths h and D are on the device; S - 1 steps follow, each five plain launches in stream order.  Which pair a step picked stays
// on the device: squash_pick_finish_kernel writes row k of the output, the kernels behind it read that row, and where it is a
// filler (fewer than two active clusters) they return at once.  No atomics, no grid-wide wait; every sum has one owner and a fixed
// order, so the bits depend on neither grid nor block shape.
//   squash_init_kernel         active[s] = T_s != 0, size[s] = 1, n_merges = max(active - 1, 0)        (one block)
//   squash_pick_kernel         the minimum of (D[a][b], a, b) over the active pairs a < b of the rows a block owns -> scratch[block]
//   squash_pick_finish_kernel  the minimum over the blocks; row k, active[b] = 0, size[a] += size[b]   (one block)
//   squash_merge_kernel        one thread a node: the new column a of U and V, and a contiguous copy ua, va
//   squash_row_kernel          the hot path: (chunk of KR_CHUNK_IDS ids) x (group of SQUASH_GROUP samples: one wave); a thread owns one t
//                              and walks its chunk by node_ring (below), h / ua / va of the chunk staged in the LDS and read a batch
//                              at a time, the KR term with the merged cluster as the first operand -- into part[chunk][t]
//   squash_row_reduce_kernel   D[min(a, t)][max(a, t)] = the partials of t by the chunk rule (the pick reads the upper triangle only)
// The (distance, a, b) order is total, so any shape of the reduction finds the same pair.
// ------------------------------------------------------------------------------------------------
constexpr u32 SQUASH_FILLER = 0xFFFFFFFFu, SQUASH_GROUP = 64, SQUASH_UNROLL = 8, SQUASH_DEPTH = 4, SQUASH_PICK_BLOCKS = 512;

struct SquashRow {  // rk_squash_merge
    u32 a, b, size, reserved;
    double distance;
};
struct SquashBest {
    double d;
    u32 a, b;
};

__device__ __forceinline__ void squash_take(SquashBest &best, double d, u32 a, u32 b) {
    if (d < best.d || (d == best.d && (a < best.a || (a == best.a && b < best.b)))) best = SquashBest{d, a, b};
}

// the best of the block's 256 candidates, in every thread of it
__device__ __forceinline__ SquashBest squash_block_best(SquashBest mine) {
    __shared__ SquashBest cand[256];
    const u32 tid = threadIdx.x;
    cand[tid] = mine;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            SquashBest x = cand[tid];
            const SquashBest y = cand[tid + o];
            squash_take(x, y.d, y.a, y.b);
            cand[tid] = x;
        }
    }
    __syncthreads();
    return cand[0];
}

__global__ void __launch_bounds__(256) squash_init_kernel(u32 B, u32 S, u32 root, const u64 *clade, u32 *active, u32 *size, u32 *n_merges) {
    __shared__ u32 count[256];
    const u32 tid = threadIdx.x;
    u32 n = 0;
    for (u32 s = tid; s < S; s += 256) {
        const u32 on = clade[(u64)s * B + root] != 0 ? 1u : 0u;
        active[s] = on;
        size[s] = 1;
        n += on;
    }
    count[tid] = n;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) count[tid] += count[tid + o];
    }
    if (tid == 0) *n_merges = count[0] ? count[0] - 1 : 0;
}

__global__ void __launch_bounds__(256) squash_pick_kernel(u32 S, const double *D, const u32 *active, SquashBest *scratch) {
    SquashBest best{__builtin_inf(), SQUASH_FILLER, SQUASH_FILLER};
    for (u32 a = blockIdx.x; a + 1 < S; a += gridDim.x) {
        if (!active[a]) continue;  // (uniform)
        const double *row = D + (u64)a * S;
        for (u32 b = a + 1 + threadIdx.x; b < S; b += 256)
            if (active[b]) squash_take(best, row[b], a, b);
    }
    best = squash_block_best(best);
    if (threadIdx.x == 0) scratch[blockIdx.x] = best;
}

__global__ void __launch_bounds__(256) squash_pick_finish_kernel(u32 n_scratch, u32 k, const SquashBest *scratch, u32 *active, u32 *size, SquashRow *merges) {
    SquashBest best{__builtin_inf(), SQUASH_FILLER, SQUASH_FILLER};
    for (u32 i = threadIdx.x; i < n_scratch; i += 256) {
        const SquashBest c = scratch[i];
        squash_take(best, c.d, c.a, c.b);
    }
    best = squash_block_best(best);
    if (threadIdx.x != 0) return;
    if (best.a == SQUASH_FILLER) {
        merges[k] = SquashRow{SQUASH_FILLER, SQUASH_FILLER, 0, 0, 0.0};
        return;
    }
    const u32 n = size[best.a] + size[best.b];  // (size[b] stays: the merge kernel reads it)
    size[best.a] = n;
    active[best.b] = 0;
    merges[k] = SquashRow{best.a, best.b, n, 0, best.d};
}

__global__ void __launch_bounds__(256) squash_merge_kernel(u32 B, u32 S, u32 k, const SquashRow *merges, const u32 *size, double *U, double *V, double *ua, double *va) {
    const SquashRow row = merges[k];
    const u32 x = blockIdx.x * 256 + threadIdx.x;
    if (row.a == SQUASH_FILLER || x >= B) return;
    const u32 nb = size[row.b], na = row.size - nb;
    const double wa = (double)na, wb = (double)nb, n = (double)row.size;
    double *pu = U + (u64)x * S, *pv = V + (u64)x * S;
    const double u = (wa * pu[row.a] + wb * pu[row.b]) / n;
    const double v = (wa * pv[row.a] + wb * pv[row.b]) / n;
    pu[row.a] = u;
    pv[row.a] = v;
    ua[x] = u;
    va[x] = v;
}

// ------------------------------------------------------------------------------------------------
// node_ring<UNROLL, DEPTH>: the frame of squash_row_kernel and of kmeans_dist_kernel (rk_kmeans.h) -- a thread's walk in ascending id
// over the nodes [x_lo, x_lo + n) of its own sample's columns pu, pv of U and V (the 64 lanes of a wave take one 512-byte line of
// each a node).  Whole groups of DEPTH batches of UNROLL nodes go through a ring of register batches, DEPTH - 1 of them in flight
// while one is summed (a thread's sum is one dependent chain, so what a wave can hide of the loads' latency is what it has in
// flight).  A batch at x0 is, in this order: q = uniform(x0), what it reads beside the loads; the loads of the batch ahead; a
// scheduling barrier; sum(q, x0, u, v); a scheduling barrier -- the barriers keep the loads of the batch ahead, and the uniform
// reads of this one, in front of this one's sum.  Then the batches that fill no group, and term(x, u, v) for the nodes that fill
// no batch.
// ------------------------------------------------------------------------------------------------
template <u32 UNROLL, u32 DEPTH, class Uniform, class Sum, class Term>
__device__ __forceinline__ void node_ring(const double *pu, const double *pv, u32 S, u32 x_lo, u32 n, Uniform &&uniform, Sum &&sum, Term &&term) {
    auto load = [&](double(&lu)[UNROLL], double(&lv)[UNROLL], u32 x0) {
#pragma unroll
        for (u32 i = 0; i < UNROLL; i++) {
            lu[i] = pu[(u64)(x0 + i) * S];
            lv[i] = pv[(u64)(x0 + i) * S];
        }
    };
    const u32 x_hi = x_lo + n, n_batches = n / (UNROLL * DEPTH) * DEPTH;
    u32 x = x_lo;
    if (n_batches) {
        double ru[DEPTH][UNROLL], rv[DEPTH][UNROLL];
#pragma unroll
        for (u32 d = 0; d + 1 < DEPTH; d++) load(ru[d], rv[d], x_lo + d * UNROLL);
        for (u32 b0 = 0; b0 < n_batches; b0 += DEPTH) {
#pragma unroll
            for (u32 d = 0; d < DEPTH; d++) {
                const u32 x0 = x_lo + (b0 + d) * UNROLL, ahead = min(b0 + d + DEPTH - 1, n_batches - 1);  // (the last batches load the last one again: no branch)
                const auto q = uniform(x0);
                load(ru[(d + DEPTH - 1) % DEPTH], rv[(d + DEPTH - 1) % DEPTH], x_lo + ahead * UNROLL);
                __builtin_amdgcn_sched_barrier(0);
                sum(q, x0, ru[d], rv[d]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        x = x_lo + n_batches * UNROLL;
    }
    for (; x + UNROLL <= x_hi; x += UNROLL) {  // the batches that fill no group
        double lu[UNROLL], lv[UNROLL];
        const auto q = uniform(x);
        load(lu, lv, x);
        sum(q, x, lu, lv);
    }
    for (; x < x_hi; x++) term(x, pu[(u64)x * S], pv[(u64)x * S]);
}

__global__ void __launch_bounds__(SQUASH_GROUP) squash_row_kernel(u32 B, u32 S, u32 k, const SquashRow *merges, const u32 *active, const double *U, const double *V,
                                                         const double *h, const double *ua, const double *va, double *part) {
    __shared__ double uni[3][KR_CHUNK_IDS];  // h, ua, va of the chunk: the same for every thread of the block
    const u32 a = merges[k].a;
    if (a == SQUASH_FILLER) return;
    const u32 t = blockIdx.y * SQUASH_GROUP + threadIdx.x;
    const bool need = t < S && t != a && active[t] != 0;
    if (!__syncthreads_or(need)) return;  // the block's samples are all inactive or a
    const u32 x_lo = blockIdx.x * KR_CHUNK_IDS, x_hi = min(x_lo + KR_CHUNK_IDS, B);
    for (u32 i = threadIdx.x; i < x_hi - x_lo; i += SQUASH_GROUP) {
        uni[0][i] = h[x_lo + i];
        uni[1][i] = ua[x_lo + i];
        uni[2][i] = va[x_lo + i];
    }
    __syncthreads();
    if (__ballot(need) == 0) return;  // (a group of several waves: the wave's 64 samples are all inactive or a; no barrier below)
    const u32 tc = t < S ? t : S - 1;  // (lanes without a sample of their own read the last one's and write nothing)
    double acc = 0.0;
    struct Uniform {  // h, ua, va of a batch: broadcast reads of the LDS
        double h[SQUASH_UNROLL], a[SQUASH_UNROLL], b[SQUASH_UNROLL];
    };
    node_ring<SQUASH_UNROLL, SQUASH_DEPTH>(
        U + tc, V + tc, S, x_lo, x_hi - x_lo,
        [&](u32 x0) {
            Uniform q;
#pragma unroll
            for (u32 i = 0; i < SQUASH_UNROLL; i++) {
                q.h[i] = uni[0][x0 - x_lo + i];
                q.a[i] = uni[1][x0 - x_lo + i];
                q.b[i] = uni[2][x0 - x_lo + i];
            }
            return q;
        },
        [&](const Uniform &q, u32, const double(&lu)[SQUASH_UNROLL], const double(&lv)[SQUASH_UNROLL]) {
#pragma unroll
            for (u32 i = 0; i < SQUASH_UNROLL; i++) acc = kr_term(acc, q.h[i], q.a[i], lu[i], q.b[i], lv[i]);
        },
        [&](u32 x, double u, double v) { acc = kr_term(acc, uni[0][x - x_lo], uni[1][x - x_lo], u, uni[2][x - x_lo], v); });
    if (need) part[(u64)blockIdx.x * S + t] = acc;
}

__global__ void __launch_bounds__(256) squash_row_reduce_kernel(u32 S, u32 k, u32 n_chunks, const SquashRow *merges, const u32 *active, const double *part, double *D) {
    const u32 a = merges[k].a;
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (a == SQUASH_FILLER || t >= S || t == a || !active[t]) return;
    D[(u64)min(a, t) * S + max(a, t)] = chunk_sum(n_chunks, [&](u32 c) { return part[(u64)c * S + t]; });
}

}  // namespace rk
