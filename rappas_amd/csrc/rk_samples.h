// rk_samples.h -- #included by rk_kernels.hip: the sample-level kernels -- the clade sums of sample mass buffers over
// a tree on the device, and the pairwise Kantorovich-Rubinstein distances between the samples.  The launches and the entry points
// are in rk_samples_impl.h, the host twins in rk_samples_host.h.  Not part of the C ABI.
#pragma once
#include "rk_device.h"

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
// acc = (acc + h * |u_s - u_t|) + h * |v_s - v_t|, three FP64 operations a term (no contraction).
// A chunk's partial starts at +0.0.  With n_part == 0 the block holds every chunk and adds the partials in chunk order into D, the
// first one as it is; otherwise it writes each partial to part[chunk] (S x S doubles each) and kr_reduce_kernel adds them in chunk
// order.  Either way an entry and its mirror are written by the one thread that summed the pair: no atomics, and the bits depend on
// neither grid nor tile.  A diagonal tile sums both triangles (|a - b| == |b - a|: the same bits) and writes no mirror.
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
                    for (u32 bb = 0; bb < 4; bb++) {
                        const double term1 = hx * fabs(ru[a] - cu[bb]);
                        const double term2 = hx * fabs(rv[a] - cv[bb]);
                        acc[a][bb] = (acc[a][bb] + term1) + term2;
                    }
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
                for (u32 bb = 0; bb < 4; bb++) d[a][bb] = ch == ch_lo ? acc[a][bb] : d[a][bb] + acc[a][bb];
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

// D[i] = part[0][i], then + part[1][i], ... in chunk order: the entries of both triangles hold the same partials
__global__ void __launch_bounds__(256) kr_reduce_kernel(u64 n, u32 n_chunks, const double *part, double *D) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double d = part[i];
    for (u32 c = 1; c < n_chunks; c++) d = d + part[(u64)c * n + i];
    D[i] = d;
}

}  // namespace rk
