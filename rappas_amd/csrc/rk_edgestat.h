// rk_edgestat.h -- #included by rk_kernels.hip behind rk_epca.h: the kernels of the edge statistics, edge dispersion and edge
// correlation (include/rappas_place.h holds the definition).  After the clade sums, plain launches in stream order:
// no atomics across blocks, no grid-wide wait, every sum has one owner; the floating-point sums have the order of the lane rule, the
// rank sums are integers.  n and the mask of the unusable columns are found on the device (info[0], info[1]) and stay there.
//   edgestat_profiles_kernel  kr_profiles_kernel's transpose: masses and clade sums read along the nodes, P0 (mass share) and P1
//                             (imbalance) written node-major [x][s], so that an edge's row is one contiguous line
//   edgestat_init_kernel      one block: active[s], n, the usable test of every column -> info
//   edgestat_column_kernel    one block a metadata column: gmean, gc[S], gss, gd[S], grss with the rank routines of the edge kernel
//   edgestat_edge_kernel      the hot path, one row = one (edge, quantity).  The row is read from memory once and again from the
//                             caches: into the LDS as rank keys (+inf for a sample without mass: it ranks behind every value and is
//                             never an answer), for the mean, for the centred sums -- a wave at a time by the lane rule, 1 + F
//                             accumulators a lane as epca_loadings_kernel has k -- and for the ranks.
//       COUNT form            S <= the crossover: a wave a row, four rows (two edges) a block.  A lane counts, for each of its
//                             samples, the keys below and not above its value: every lane reads the same LDS address, a broadcast
//                             without bank conflicts, S compares a sample and no sort.
//       SORT form             beyond: a block a row.  The keys, padded with +inf to a power of two, are sorted in the LDS (bitonic,
//                             compared as doubles: no key transform); a thread finds the two ends of the tie run of its value by
//                             two branch-free binary searches, which is rank2 without carrying an index through the sort.
// Where the forms cross is RK_EDGESTAT_COUNT_MAX_SAMPLES (profiles/edgestat_rate.txt).  The launches and the entry points are in
// rk_samples_impl.h, the host twin in rk_edgestat_host.h.  No 64-bit shift anywhere.
#pragma once
#include "rk_epca.h"

namespace rk {

constexpr u32 EDGESTAT_MAX_F = 8, EDGESTAT_THREADS = 256, EDGESTAT_WAVES = EDGESTAT_THREADS / 64;
constexpr u32 EDGESTAT_COUNT_LIMIT = 1024;  // the COUNT form's LDS holds four rows: the crossover, wherever a developer build puts it, stays below this
constexpr u64 EDGESTAT_FILLER = 0x7FF8000000000000ull;

__device__ __forceinline__ double edgestat_inf() { return __hiloint2double(0x7FF00000, 0); }
__device__ __forceinline__ bool edgestat_finite(double g) { return (__double2hiint(g) & 0x7FF00000) != 0x7FF00000; }
__device__ __forceinline__ u64 edgestat_bits(double d) { return (u64)__double_as_longlong(d); }

__global__ void __launch_bounds__(256) edgestat_profiles_kernel(u32 B, u32 S, u64 W, u32 root, const u64 *masses, const u64 *clade, double *P0, double *P1) {
    __shared__ double t0[32][33], t1[32][33];
    const u32 i = threadIdx.x & 31, j = threadIdx.x >> 5;
    const u32 x0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
#pragma unroll
    for (u32 jj = 0; jj < 4; jj++) {
        const u32 sl = j + 8 * jj, s = s0 + sl, x = x0 + i;
        if (s < S && x < B) {
            const u64 c = clade[(u64)s * B + x], mm = masses[(u64)s * W + x], T = clade[(u64)s * B + root];
            const bool on = T != 0 && x != root;
            t0[sl][i] = on ? edgestat_share(mm, T) : 0.0;
            t1[sl][i] = on ? edgestat_imbalance(c, mm, T) : 0.0;
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 jj = 0; jj < 4; jj++) {
        const u32 xl = j + 8 * jj, x = x0 + xl, s = s0 + i;
        if (s < S && x < B) {
            P0[(u64)x * S + s] = t0[i][xl];
            P1[(u64)x * S + s] = t1[i][xl];
        }
    }
}

__global__ void __launch_bounds__(256) edgestat_init_kernel(u32 B, u32 S, u32 F, u32 root, const u64 *clade, const double *meta, u32 *active, u32 *info) {
    __shared__ u32 count[256];
    __shared__ u32 bad;
    const u32 tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    u32 n = 0, mine = 0;
    for (u32 s = tid; s < S; s += 256) {
        const u32 on = clade[(u64)s * B + root] != 0 ? 1u : 0u;
        active[s] = on;
        n += on;
        for (u32 f = 0; f < F; f++)
            if (on && !edgestat_finite(meta[(u64)f * S + s])) mine |= 1u << f;
    }
    if (mine) atomicOr(&bad, mine);  // (in the LDS of the one block)
    count[tid] = n;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) count[tid] += count[tid + o];
    }
    __syncthreads();
    if (tid == 0) {
        info[0] = count[0];
        info[1] = bad;
    }
}

// ------------------------------------------------------------------------------------------------
// The two rank routines.  Both answer d = rank2 - (n + 1) for a finite value `a` that is among the keys.
// ------------------------------------------------------------------------------------------------
// COUNT: over the S keys of a row in the LDS (every lane the same address)
__device__ __forceinline__ int edgestat_rank_count(const double *key, u32 S, u32 n, double a) {
    u32 less = 0, upto = 0;
    for (u32 t = 0; t < S; t++) {
        const double b = key[t];
        less += b < a ? 1u : 0u;
        upto += b <= a ? 1u : 0u;
    }
    return edgestat_rank_dev(less, upto, n);
}

// SORT: the N keys (a power of two) ascending, by the whole block; the barrier behind the last step is the caller's to rely on
__device__ __forceinline__ void edgestat_sort(double *key, u32 N, u32 tid) {
    for (u32 k = 2; k <= N; k <<= 1)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 t = tid; t < N / 2; t += EDGESTAT_THREADS) {
                const u32 i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const bool up = (i & k) == 0;
                const double x = key[i], y = key[p];
                if ((y < x) == up) {
                    key[i] = y;
                    key[p] = x;
                }
            }
            __syncthreads();
        }
}
// the number of sorted keys for which `below(key)` holds (it holds for a prefix): log2 N steps without a branch
template <class Below>
__device__ __forceinline__ u32 edgestat_prefix(const double *key, u32 N, Below below) {
    u32 pos = 0;
    for (u32 step = N >> 1; step > 0; step >>= 1)
        if (below(key[pos + step - 1])) pos += step;
    return pos + (below(key[pos]) ? 1u : 0u);  // (the steps reach N - 1 at most)
}
__device__ __forceinline__ int edgestat_rank_sorted(const double *key, u32 N, u32 n, double a) {
    const u32 less = edgestat_prefix(key, N, [a](double b) { return b < a; });
    const u32 upto = edgestat_prefix(key, N, [a](double b) { return b <= a; });
    return edgestat_rank_dev(less, upto, n);
}

__device__ __forceinline__ long long edgestat_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One metadata column a block: feature row f of the raw output, gc and gd of the column in the workspace
__global__ void __launch_bounds__(EDGESTAT_THREADS) edgestat_column_kernel(u32 B, u32 S, u32 F, u32 N, u32 sort, const u32 *info, const u32 *active, const double *meta,
                                                                           double *gc, int *gd, u64 *raw) {
    extern __shared__ double edgestat_lds[];  // key[sort ? N : S]
    double *key = edgestat_lds;
    __shared__ long long wave_rss[EDGESTAT_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const u32 n = info[0];
    u64 *out = raw + (u64)B * (6 + 4 * (u64)F) + 3 * (u64)f;
    if (n == 0 || (info[1] >> f & 1)) {  // (the whole block) no sample with mass: zeros; an unusable column: the fillers
        if (tid < 3) out[tid] = n == 0 || tid == 2 ? 0ull : EDGESTAT_FILLER;
        return;
    }
    const double *g = meta + (u64)f * S;
    double *c = gc + (u64)f * S;
    int *d = gd + (u64)f * S;
    const u32 n_keys = sort ? N : S;
    for (u32 s = tid; s < n_keys; s += EDGESTAT_THREADS) key[s] = s < S && active[s] ? g[s] : edgestat_inf();
    // every wave takes the mean for itself: the same bits
    double p = 0.0;
    for (u32 s = lane; s < S; s += 64) p = p + (active[s] ? g[s] : 0.0);
    const double mean = epca_lane_finish(p) / (double)n;
    for (u32 s = tid; s < S; s += EDGESTAT_THREADS) c[s] = edgestat_centre(active[s] != 0, g[s], mean);
    if (wave == 0) {
        double q = 0.0;
        for (u32 s = lane; s < S; s += 64) {
            const double cs = edgestat_centre(active[s] != 0, g[s], mean);
            q = gram_term(q, cs, cs);
        }
        const double ss = epca_lane_finish(q);
        if (lane == 0) {
            out[0] = edgestat_bits(mean);
            out[1] = edgestat_bits(ss);
        }
    }
    __syncthreads();
    if (sort) edgestat_sort(key, N, tid);
    long long rss = 0;
    for (u32 s = tid; s < S; s += EDGESTAT_THREADS) {
        int ds = 0;
        if (active[s]) ds = sort ? edgestat_rank_sorted(key, N, n, g[s]) : edgestat_rank_count(key, S, n, g[s]);
        d[s] = ds;
        rss += (long long)ds * ds;
    }
    rss = edgestat_wave_sum(rss);
    if (lane == 0) wave_rss[wave] = rss;
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        for (u32 w = 0; w < EDGESTAT_WAVES; w++) total += wave_rss[w];
        out[2] = (u64)total;
    }
}

// ------------------------------------------------------------------------------------------------
// edgestat_edge_kernel<SORT>: NW waves a row -- 1 (COUNT: the block's four waves take the rows 4 * blockIdx.x ..) or 4 (SORT: the
// block takes row blockIdx.x); row r is quantity r & 1 of edge r >> 1.  Sum 0 is ss, sum 1 + f is cross_f; the waves of a row deal
// the sums round among them and take them in one pass over the row.  Every wave of every block reaches every barrier.
// ------------------------------------------------------------------------------------------------
template <bool SORT>
__global__ void __launch_bounds__(EDGESTAT_THREADS) edgestat_edge_kernel(u32 B, u32 S, u32 F, u32 N, const u32 *info, const u32 *active, const double *P0, const double *P1,
                                                                         const double *gc, const int *gd, u64 *raw) {
    constexpr u32 NW = SORT ? EDGESTAT_WAVES : 1, ROWS = EDGESTAT_WAVES / NW, SUMS = 1 + EDGESTAT_MAX_F;
    extern __shared__ double edgestat_lds[];  // SORT: key[N]; COUNT: key[ROWS][S]
    __shared__ long long wave_int[EDGESTAT_WAVES][SUMS];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 w = SORT ? wave : 0, gtid = SORT ? tid : lane;  // the wave within its row, the thread within its row
    const u32 r = blockIdx.x * ROWS + (SORT ? 0 : wave), x = r >> 1, q = r & 1;
    const bool valid = x < B;  // (a whole wave)
    const u32 n = info[0], unusable = info[1];
    const u64 RW = 6 + 4 * (u64)F;
    u64 *out = raw + (u64)x * RW;
    if (n == 0) {  // (the whole grid) no sample with mass: every word 0 / +0.0
        if (valid)
            for (u32 i = gtid; i < 3 + 2 * F; i += 64 * NW) out[i < 3 ? 3 * q + i : 6 + 4 * ((i - 3) >> 1) + 2 * q + ((i - 3) & 1)] = 0ull;
        return;
    }
    const double *row = (q ? P1 : P0) + (u64)(valid ? x : 0) * S;
    double *key = edgestat_lds + (SORT ? 0 : wave * S);
    const u32 n_keys = SORT ? N : S;
    if (valid)
        for (u32 s = gtid; s < n_keys; s += 64 * NW) key[s] = s < S && active[s] ? row[s] : edgestat_inf();
    if (valid) {
        // the mean, by every wave of the row for itself (the same bits); the entry of a sample without mass is +0.0
        double p = 0.0;
        for (u32 s = lane; s < S; s += 64) p = p + row[s];
        const double mean = epca_lane_finish(p) / (double)n;
        // the sums this wave owns: j = w, w + NW, ... < 1 + F, a column's only when it is usable
        u32 mine = 0;
        for (u32 j = w; j < 1 + F; j += NW)
            if (j == 0 || !(unusable >> (j - 1) & 1)) mine |= 1u << j;
        double acc[SUMS];
#pragma unroll
        for (u32 j = 0; j < SUMS; j++) acc[j] = 0.0;
        if (mine)
            for (u32 s = lane; s < S; s += 64) {
                const double c = edgestat_centre(active[s] != 0, row[s], mean);
#pragma unroll
                for (u32 j = 0; j < SUMS; j++)
                    if (mine >> j & 1) acc[j] = gram_term(acc[j], c, j == 0 ? c : gc[(u64)(j - 1) * S + s]);
            }
#pragma unroll
        for (u32 j = 0; j < SUMS; j++) {
            if (j >= 1 + F || j % NW != w) continue;  // (uniform) not this wave's word
            const bool filler = !(mine >> j & 1);
            const double sum = filler ? 0.0 : epca_lane_finish(acc[j]);
            if (lane == 0) out[j == 0 ? 3 * q + 1 : 6 + 4 * (u64)(j - 1) + 2 * q] = filler ? EDGESTAT_FILLER : edgestat_bits(sum);
        }
        if (w == 0 && lane == 0) out[3 * q] = edgestat_bits(mean);
    }
    __syncthreads();  // the keys are in the LDS
    if (SORT) edgestat_sort(key, N, tid);
    long long isum[SUMS];  // 0: rss; 1 + f: rcross_f
#pragma unroll
    for (u32 j = 0; j < SUMS; j++) isum[j] = 0;
    if (valid)
        for (u32 s = gtid; s < S; s += 64 * NW) {
            if (!active[s]) continue;
            const double a = row[s];
            const int d = SORT ? edgestat_rank_sorted(key, N, n, a) : edgestat_rank_count(key, S, n, a);
            isum[0] += (long long)d * d;
#pragma unroll
            for (u32 j = 1; j < SUMS; j++)
                if (j < 1 + F && !(unusable >> (j - 1) & 1)) isum[j] += (long long)d * gd[(u64)(j - 1) * S + s];
        }
#pragma unroll
    for (u32 j = 0; j < SUMS; j++)
        if (j < 1 + F) {  // (uniform)
            const long long v = edgestat_wave_sum(isum[j]);
            if (lane == 0) wave_int[wave][j] = v;
        }
    __syncthreads();
    if (valid && gtid < 1 + F) {
        long long total = 0;
        for (u32 k = 0; k < NW; k++) total += wave_int[(SORT ? 0 : wave) + k][gtid];
        out[gtid == 0 ? 3 * q + 2 : 6 + 4 * (u64)(gtid - 1) + 2 * q + 1] = (u64)total;  // (an unusable column summed nothing: its filler, 0)
    }
}

}  // namespace rk
