// rk_epca.h -- #included by rk_kernels.hip behind rk_samples.h: the edge-PCA kernels (include/rappas_place.h holds the
// definition, steps 1 - 8).  After the clade sums and the profiles U, V of the KR call, plain launches in stream order: no atomics, no
// grid-wide wait, every sum has one owner and a fixed order, so the bits depend on neither grid nor block shape.  n_active and k_eff
// are found on the device (info[0], info[1]) and stay there: the host launches for k columns, a kernel leaves a column >= k_eff alone
// and the results kernel writes it as +0.0.
//   epca_init_kernel      active[s] = T_s != 0, info = {n_active, k_eff}, the start vectors                     (one block)
//   epca_centre_kernel    one wave a node: X from the 512-byte lines of U[x] and V[x], the lane rule for the mean, Xc[x][.] over U[x][.]
//   epca_gram_kernel      the hot path: kr_pairs_kernel's shape with one staged matrix and acc = acc + a * b
//   (kr_reduce_kernel     the chunk partials of G in chunk order, when they went through the workspace)
//   epca_multiply_kernel  one wave a sample row s: out[j][s] = LS(t -> G[s][t] * in[j][t]), k accumulators a lane
//   epca_orth_kernel      one block: step 6 behind the product, column after column; the dots of the columns l > j go to different waves
//   epca_results_kernel   one block: trace, nn, lambda, rr, the q rows, zeros for the columns >= k_eff
//   epca_loadings_kernel  one wave a node: w[j][x] = LS(s -> Xc[x][s] * q[j][s]), k accumulators a lane
// The launches and the entry points are in rk_samples_impl.h, the host twin in rk_samples_host.h.  No 64-bit shift anywhere.
#pragma once
#include "rk_samples.h"

namespace rk {

constexpr u32 EPCA_MAX_K = 8, EPCA_WAVES = 4, EPCA_STAGE = 8;

// the value of lane i (a constant) in every lane
__device__ __forceinline__ double epca_lane_value(double p, int i) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), i), __builtin_amdgcn_readlane(__double2loint(p), i));
}

// The second half of the lane rule: (((+0.0 + p_0) + p_1) + ...) + p_63 over the 64 lanes' partials, in every lane.  Whole waves only.
__device__ __forceinline__ double epca_lane_finish(double p) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 64; i++) acc = acc + epca_lane_value(p, i);
    return acc;
}

// A lane's sum is one dependent chain in ascending s, which the definition does not let it split; what it can do is have the loads
// of EPCA_AHEAD steps in flight before the adds of those steps (the order of the adds stays).
constexpr u32 EPCA_AHEAD = 8;

// dot(a, b) by one whole wave
__device__ __forceinline__ double epca_wave_dot(u32 S, u32 lane, const double *a, const double *b) {
    double p = 0.0;
    u32 s = lane;
    for (; s + 64 * (EPCA_AHEAD - 1) < S; s += 64 * EPCA_AHEAD) {
        double x[EPCA_AHEAD], y[EPCA_AHEAD];
#pragma unroll
        for (u32 i = 0; i < EPCA_AHEAD; i++) {
            x[i] = a[s + 64 * i];
            y[i] = b[s + 64 * i];
        }
#pragma unroll
        for (u32 i = 0; i < EPCA_AHEAD; i++) {
            const double t = x[i] * y[i];
            p = p + t;
        }
    }
    for (; s < S; s += 64) {
        const double t = a[s] * b[s];
        p = p + t;
    }
    return epca_lane_finish(p);
}

__device__ __forceinline__ double epca_start_value(u32 s, u32 j) { return (double)((s * 8u + j + 1u) * 2654435761u) / 4294967296.0 - 0.5; }

__global__ void __launch_bounds__(256) epca_init_kernel(u32 B, u32 S, u32 k, u32 root, const u64 *clade, u32 *active, u32 *info, double *Q) {
    __shared__ u32 count[256];
    const u32 tid = threadIdx.x;
    u32 n = 0;
    for (u32 s = tid; s < S; s += 256) {
        const u32 on = clade[(u64)s * B + root] != 0 ? 1u : 0u;
        active[s] = on;
        n += on;
        for (u32 j = 0; j < k; j++) Q[(u64)j * S + s] = epca_start_value(s, j);
    }
    count[tid] = n;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) count[tid] += count[tid + o];
    }
    if (tid == 0) {
        info[0] = count[0];
        info[1] = count[0] < 2 ? 0u : min(k, count[0] - 1);
    }
}

// Steps 2 and 3.  U[x][.] becomes Xc[x][.]; V is only read.  k_eff == 0: Xc is all +0.0 (and so is G).
__global__ void __launch_bounds__(64 * EPCA_WAVES) epca_centre_kernel(u32 B, u32 S, u32 root, const u32 *active, const u32 *info, double *U, const double *V) {
    const u32 lane = threadIdx.x & 63, x = blockIdx.x * EPCA_WAVES + (threadIdx.x >> 6);
    if (x >= B) return;  // (a whole wave)
    const u32 n = info[0];
    const bool on = info[1] != 0 && x != root;
    double *pu = U + (u64)x * S;
    const double *pv = V + (u64)x * S;
    double p = 0.0;
    for (u32 s = lane; s < S; s += 64) {
        const double X = on && active[s] ? (pu[s] + pv[s]) - 1.0 : 0.0;
        p = p + X;
    }
    const double mean = epca_lane_finish(p) / (double)n;
    for (u32 s = lane; s < S; s += 64) pu[s] = on && active[s] ? ((pu[s] + pv[s]) - 1.0) - mean : 0.0;
}

// ------------------------------------------------------------------------------------------------
// epca_gram_kernel: a symmetric rank-B update, G = Xc^T Xc, in the order the definition fixes.  Built as kr_pairs_kernel is: a block
// of 256 threads owns a tile of 64 x 64 sample pairs on or above the diagonal and the chunks [blockIdx.y * chunks_per_block,
// + chunks_per_block); per stage of EPCA_STAGE nodes the centred values of the tile's 64 row samples and 64 column samples go through
// the LDS -- one matrix, so a thread loads EPCA_STAGE / 2 values a stage, in flight in registers while the stage before is summed --;
// a thread keeps the same 4 x 4 micro-tile and walks the nodes in ascending id: acc = acc + r * c (gram_term of rk_samplemath.h), two
// FP64 operations a term.  The chunk rule (chunk_fold), the two forms of the chunk sum (to_part: part[chunk], added by
// kr_reduce_kernel) and the mirror written by the thread that summed the pair are kr_pairs_kernel's.  A diagonal tile sums both
// triangles (a * b == b * a: the same bits).  The two kernels stay two texts: rk_samples.h says why above kr_pairs_kernel.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) epca_gram_kernel(u32 B, u32 S, u32 n_tiles_side, u32 chunks_per_block, u32 to_part, const double *Xc, double *G, double *part) {
    __shared__ __attribute__((aligned(16))) double st[EPCA_STAGE * 128];  // [node][rows | columns][64]
    u32 ti = 0, rem = blockIdx.x;
    while (rem >= n_tiles_side - ti) {
        rem -= n_tiles_side - ti;
        ti++;
    }
    const u32 tj = ti + rem;
    const u32 r0 = ti * KR_TILE, c0 = tj * KR_TILE;
    const u32 tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // what this thread loads of a stage: sample `ls` of the rows or the columns, of the nodes l_k, l_k + 2, ...
    constexpr u32 LOADS = EPCA_STAGE / 2;
    const u32 lj = tid & 63, l_col = (tid >> 6) & 1, l_k = tid >> 7;
    const u32 ls = (l_col ? c0 : r0) + lj;
    const double *src = Xc + ls;
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
        double nxt[LOADS];
#pragma unroll
        for (u32 k = 0; k < LOADS; k++) nxt[k] = l_ok && x_lo + l_k + 2 * k < x_hi ? src[(u64)(x_lo + l_k + 2 * k) * S] : 0.0;
        for (u32 x0 = x_lo; x0 < x_hi; x0 += EPCA_STAGE) {
            __syncthreads();  // the stage before this one has been read
#pragma unroll
            for (u32 k = 0; k < LOADS; k++) st[(l_k + 2 * k) * 128 + (tid & 127)] = nxt[k];
            __syncthreads();
            const u32 x1 = x0 + EPCA_STAGE;
#pragma unroll
            for (u32 k = 0; k < LOADS; k++) nxt[k] = l_ok && x1 + l_k + 2 * k < x_hi ? src[(u64)(x1 + l_k + 2 * k) * S] : 0.0;
            const u32 nk = min(EPCA_STAGE, x_hi - x0);
#pragma unroll 1
            for (u32 k = 0; k < nk; k++) {
                const double *b = st + k * 128;
                double r[4], c[4];
#pragma unroll
                for (u32 g = 0; g < 2; g++) {
                    const double2 a0 = *(const double2 *)(b + g * 32 + 2 * ty), a1 = *(const double2 *)(b + 64 + g * 32 + 2 * tx);
                    r[2 * g] = a0.x; r[2 * g + 1] = a0.y;
                    c[2 * g] = a1.x; c[2 * g + 1] = a1.y;
                }
#pragma unroll
                for (u32 a = 0; a < 4; a++)
#pragma unroll
                    for (u32 bb = 0; bb < 4; bb++) acc[a][bb] = gram_term(acc[a][bb], r[a], c[bb]);
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
                    G[(u64)s * S + t] = d[a][bb];
                    if (ti != tj) G[(u64)t * S + s] = d[a][bb];
                }
            }
    }
}

// out[j][s] = LS(t -> G[s][t] * in[j][t]) for j < k_eff: a wave a row, the lanes along t
__global__ void __launch_bounds__(64 * EPCA_WAVES) epca_multiply_kernel(u32 S, u32 k, const u32 *info, const double *G, const double *in, double *out) {
    const u32 lane = threadIdx.x & 63, s = blockIdx.x * EPCA_WAVES + (threadIdx.x >> 6);
    const u32 k_eff = min(info[1], k);  // (never beyond the k columns there are)
    if (s >= S || k_eff == 0) return;  // (a whole wave)
    const double *row = G + (u64)s * S;
    double p[EPCA_MAX_K];
#pragma unroll
    for (u32 j = 0; j < EPCA_MAX_K; j++) p[j] = 0.0;
    constexpr u32 AHEAD = 4;
    u32 t = lane;
    for (; t + 64 * (AHEAD - 1) < S; t += 64 * AHEAD) {  // the loads of AHEAD steps, then their adds in order
        double g[AHEAD], q[AHEAD][EPCA_MAX_K];
#pragma unroll
        for (u32 i = 0; i < AHEAD; i++) {
            g[i] = row[t + 64 * i];
#pragma unroll
            for (u32 j = 0; j < EPCA_MAX_K; j++) q[i][j] = j < k_eff ? in[(u64)j * S + t + 64 * i] : 0.0;
        }
#pragma unroll
        for (u32 i = 0; i < AHEAD; i++)
#pragma unroll
            for (u32 j = 0; j < EPCA_MAX_K; j++)
                if (j < k_eff) {
                    const double term = g[i] * q[i][j];
                    p[j] = p[j] + term;
                }
    }
    for (; t < S; t += 64) {
        const double g = row[t];
#pragma unroll
        for (u32 j = 0; j < EPCA_MAX_K; j++)
            if (j < k_eff) {
                const double term = g * in[(u64)j * S + t];
                p[j] = p[j] + term;
            }
    }
#pragma unroll
    for (u32 j = 0; j < EPCA_MAX_K; j++)
        if (j < k_eff) {  // (uniform)
            const double y = epca_lane_finish(p[j]);
            if (lane == 0) out[(u64)j * S + s] = y;
        }
}

// Step 6 behind the product, in place in Y[k][S] (global memory: k * S * 8 bytes may pass the LDS).  One block.  Per column j: the
// block finds the pivot -- the largest fabs, the smallest index among equals: a total order, so the shape of the reduction plays no
// part --, divides the column, and after a barrier wave w takes the columns l = j + 1 + w, j + 1 + w + EPCA_WAVES, ...: nn (every
// wave sums it for itself: the same bits), d, and the update of column l.  A barrier closes the column.
// The zero rule: before the first column changes, the block takes the largest fabs of every column as the product delivered it (a
// maximum: no order in it; a thread holds one value per column, the loads of all columns in flight together, a wave folds them by
// six __shfl_xor steps into wave_top, and top0 is the largest of the four); at its turn a column whose largest fabs is at most
// epca_noise_bound(S, applied, the larger of its top0 and the top0 of the live columns before it) -- applied = those live columns,
// the projections it has been through -- is a zero column.  Nothing has been applied to column 0: the bound is +0.0 and the rule is the plain zero test; so it is for every column
// of the first iteration (`first`), whose columns come from the start vectors.
__global__ void __launch_bounds__(64 * EPCA_WAVES) epca_orth_kernel(u32 S, u32 k, u32 first, const u32 *info, double *Y) {
    __shared__ double best_v[64 * EPCA_WAVES];
    __shared__ u32 best_i[64 * EPCA_WAVES];
    __shared__ double wave_top[EPCA_WAVES][EPCA_MAX_K];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 k_eff = min(info[1], k);  // (never beyond the k columns there are)
    {
        double m[EPCA_MAX_K];
#pragma unroll
        for (u32 j = 0; j < EPCA_MAX_K; j++) m[j] = -1.0;  // (below every fabs)
        constexpr u32 AHEAD = 4, STEP = 64 * EPCA_WAVES;
        u32 s = tid;
        for (; s + STEP * (AHEAD - 1) < S; s += STEP * AHEAD) {  // the loads of AHEAD steps of every column, then the compares
            double a[AHEAD][EPCA_MAX_K];
#pragma unroll
            for (u32 i = 0; i < AHEAD; i++)
#pragma unroll
                for (u32 j = 0; j < EPCA_MAX_K; j++) a[i][j] = j < k_eff ? fabs(Y[(u64)j * S + s + STEP * i]) : -1.0;
#pragma unroll
            for (u32 i = 0; i < AHEAD; i++)
#pragma unroll
                for (u32 j = 0; j < EPCA_MAX_K; j++)
                    if (a[i][j] > m[j]) m[j] = a[i][j];
        }
        for (; s < S; s += STEP) {
#pragma unroll
            for (u32 j = 0; j < EPCA_MAX_K; j++) {
                const double a = j < k_eff ? fabs(Y[(u64)j * S + s]) : -1.0;
                if (a > m[j]) m[j] = a;
            }
        }
#pragma unroll
        for (u32 j = 0; j < EPCA_MAX_K; j++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double m2 = __shfl_xor(m[j], o, 64);
                if (m2 > m[j]) m[j] = m2;
            }
            if (lane == 0) wave_top[wave][j] = m[j];
        }
    }
    __syncthreads();
    u32 applied = 0;      // (uniform)
    double scale = 0.0;   // (uniform) the largest top0 of the live columns so far
    for (u32 j = 0; j < k_eff; j++) {
        double *yj = Y + (u64)j * S;
        double bv = -1.0;  // (below every fabs)
        u32 bi = 0;
        for (u32 s = tid; s < S; s += 64 * EPCA_WAVES) {
            const double a = fabs(yj[s]);
            if (a > bv) {
                bv = a;
                bi = s;
            }
        }
        best_v[tid] = bv;
        best_i[tid] = bi;
        for (u32 o = 32 * EPCA_WAVES; o > 0; o >>= 1) {
            __syncthreads();
            if (tid < o) {
                const double v2 = best_v[tid + o];
                const u32 i2 = best_i[tid + o];
                if (v2 > best_v[tid] || (v2 == best_v[tid] && i2 < best_i[tid])) {
                    best_v[tid] = v2;
                    best_i[tid] = i2;
                }
            }
        }
        __syncthreads();
        const double top = best_v[0];
        const double pivot = yj[best_i[0]];
        __syncthreads();  // everyone holds the pivot before the column changes; best_v and best_i are free again
        double top0 = wave_top[0][j];  // the largest fabs of the column as the product delivered it
#pragma unroll
        for (u32 w = 1; w < EPCA_WAVES; w++)
            if (wave_top[w][j] > top0) top0 = wave_top[w][j];
        if (top <= epca_noise_bound(S, first ? 0u : applied, top0 > scale ? top0 : scale)) {  // (uniform) a zero column: written as +0.0, projected on by nobody
            for (u32 s = tid; s < S; s += 64 * EPCA_WAVES) yj[s] = 0.0;
            continue;
        }
        applied++;
        if (top0 > scale) scale = top0;
        for (u32 s = tid; s < S; s += 64 * EPCA_WAVES) yj[s] = yj[s] / pivot;
        __syncthreads();
        if (j + 1 + wave < k_eff) {  // (a whole wave)
            const double nn = epca_wave_dot(S, lane, yj, yj);
            for (u32 l = j + 1 + wave; l < k_eff; l += EPCA_WAVES) {
                double *yl = Y + (u64)l * S;
                const double d = epca_wave_dot(S, lane, yj, yl) / nn;
                u32 s = lane;
                for (; s + 64 * (EPCA_AHEAD - 1) < S; s += 64 * EPCA_AHEAD) {  // (entries of their own: no order among them)
                    double x[EPCA_AHEAD], y[EPCA_AHEAD];
#pragma unroll
                    for (u32 i = 0; i < EPCA_AHEAD; i++) {
                        x[i] = yj[s + 64 * i];
                        y[i] = yl[s + 64 * i];
                    }
#pragma unroll
                    for (u32 i = 0; i < EPCA_AHEAD; i++) {
                        const double t = d * x[i];
                        yl[s + 64 * i] = y[i] - t;
                    }
                }
                for (; s < S; s += 64) {
                    const double t = d * yj[s];
                    yl[s] = yl[s] - t;
                }
            }
        }
        __syncthreads();
    }
}

// Step 7 and the head of the raw output: trace | lambda[k] | nn[k] | rr[k] | q[k][S].  One block; wave w takes the columns w,
// w + EPCA_WAVES, ...  The columns >= k_eff -- all of them when k_eff == 0, and then the trace too -- are +0.0.
__global__ void __launch_bounds__(64 * EPCA_WAVES) epca_results_kernel(u32 S, u32 k, const u32 *info, const double *G, const double *Q, const double *Z, double *raw) {
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 k_eff = min(info[1], k);  // (never beyond the k columns there are)
    double *lambda = raw + 1, *nn = lambda + k, *rr = nn + k, *q_out = rr + k;
    if (wave == 0) {
        double p = 0.0;
        if (k_eff)
            for (u32 s = lane; s < S; s += 64) p = p + G[(u64)s * S + s];
        const double trace = epca_lane_finish(p);
        if (lane == 0) raw[0] = trace;
    }
    for (u32 j = wave; j < k; j += EPCA_WAVES) {  // (a whole wave)
        const double *qj = Q + (u64)j * S, *zj = Z + (u64)j * S;
        double n_j = 0.0, lam = 0.0, r_j = 0.0;
        if (j < k_eff) {
            n_j = epca_wave_dot(S, lane, qj, qj);
            if (n_j == 0.0) {
                n_j = 0.0;
            } else {
                lam = epca_wave_dot(S, lane, qj, zj) / n_j;
                double p = 0.0;
                for (u32 s = lane; s < S; s += 64) {
                    const double t = lam * qj[s], r = zj[s] - t, r2 = r * r;
                    p = p + r2;
                }
                r_j = epca_lane_finish(p);
            }
        }
        if (lane == 0) {
            lambda[j] = lam;
            nn[j] = n_j;
            rr[j] = r_j;
        }
        for (u32 s = lane; s < S; s += 64) q_out[(u64)j * S + s] = j < k_eff ? qj[s] : 0.0;
    }
}

// w[j][x] = LS(s -> Xc[x][s] * q[j][s]): a wave a node, the Xc line coalesced, k accumulators a lane; +0.0 for the columns >= k_eff
__global__ void __launch_bounds__(64 * EPCA_WAVES) epca_loadings_kernel(u32 B, u32 S, u32 k, const u32 *info, const double *Xc, const double *Q, double *w) {
    const u32 lane = threadIdx.x & 63, x = blockIdx.x * EPCA_WAVES + (threadIdx.x >> 6);
    if (x >= B) return;  // (a whole wave)
    const u32 k_eff = min(info[1], k);  // (never beyond the k columns there are)
    const double *row = Xc + (u64)x * S;
    double p[EPCA_MAX_K];
#pragma unroll
    for (u32 j = 0; j < EPCA_MAX_K; j++) p[j] = 0.0;
    if (k_eff)
        for (u32 s = lane; s < S; s += 64) {
            const double c = row[s];
#pragma unroll
            for (u32 j = 0; j < EPCA_MAX_K; j++)
                if (j < k_eff) {
                    const double term = c * Q[(u64)j * S + s];
                    p[j] = p[j] + term;
                }
        }
#pragma unroll
    for (u32 j = 0; j < EPCA_MAX_K; j++)
        if (j < k) {  // (uniform)
            const double y = j < k_eff ? epca_lane_finish(p[j]) : 0.0;
            if (lane == 0) w[(u64)j * B + x] = y;
        }
}

}  // namespace rk
