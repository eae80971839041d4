// rk_kmeans.h -- #included by rk_kernels.hip: the kernels of the phylogenetic k-means of the samples (include/rappas_place.h holds the
// definition).  After the profile stage of kr_launch the node-major profiles U[x][s], V[x][s] and h are on the device;
// the seeding and the rounds are plain launches in stream order.  What the run has found so far lives in the control words of the
// workspace (KM_*): a kernel reads them first and returns at once when the run is over or its centroids do not exist.  No atomics
// between blocks, no grid-wide wait; every sum has one owner and a fixed order, so the bits depend on neither grid nor block shape.
//   kmeans_init_kernel       active[s] = T_s != 0, n_active, k_eff, status, seed_0 or the caller's seeds, the fillers   (one block)
//   kmeans_gather_kernel     cu[j] = U[.][seed_j], cv[j] = V[.][seed_j]: the centroid-major profiles the distance kernel stages
//   kmeans_dist_kernel<KC>   the hot path: (chunk of KR_CHUNK_IDS ids) x (64 samples: one wave a block) x (group of KC centroids); a
//                            thread owns one sample and KC running sums, U and V come through node_ring of rk_samples.h, tile after
//                            tile of the chunk, h / cu_j / cv_j of a tile are staged in the LDS -> part[chunk][j][t]
//   kmeans_reduce_kernel     one thread a sample: the partials of every centroid by the chunk rule, and the nearest centroid among
//                            them -> best[s], bestd[s]
//   kmeans_seed_kernel       the running minimum mind[s] and the next farthest-first seed                               (one block)
//   kmeans_assign_kernel     assign, dist, changed, the sizes; in the last round within and info, and the done word     (one block)
//   kmeans_update_kernel     one wave a block, a lane a (node, cluster): the ordered group sums of U and V over the members, the division
//   kmeans_centroids_kernel  the optional output [k][2][B]
// Not part of the C ABI.
#pragma once
#include "rk_samples.h"

namespace rk {

constexpr u32 KMEANS_FILLER = 0xFFFFFFFFu, KMEANS_MAX_CENTROIDS = 64, KMEANS_WAVE = 64, KMEANS_UNROLL = 8, KMEANS_DEPTH = 4, KMEANS_UPDATE_GROUP = 256, KMEANS_UPDATE_ENTRIES = 512;
// the control words of a run, 32-bit each: KM_SEEDS is followed by the KMEANS_MAX_CENTROIDS seeds
constexpr u32 KM_DONE = 0, KM_KEFF = 1, KM_NACTIVE = 2, KM_STATUS = 3, KM_SEEDS = 8, KM_WORDS = KM_SEEDS + KMEANS_MAX_CENTROIDS;

// node ids a tile of the LDS staging holds: (1 + 2 KC) doubles an id, 24 / 20 / 18 / 17 KB a block
template <u32 KC>
struct KmeansTile {
    static constexpr u32 ids = KC == 1 ? 1024u : KC == 2 ? 512u : KC == 4 ? 256u : 128u;
};

struct KmeansSeeds {  // the caller's seeds as a kernel argument: no copy to order, nothing of the caller's read after the call
    u32 s[KMEANS_MAX_CENTROIDS];
};

// the centroids [j_base, j_limit) that exist: none when the run is over
__device__ __forceinline__ u32 kmeans_j_hi(const u32 *ctl, u32 k, u32 j_limit) {
    if (ctl[KM_DONE] != 0) return 0;
    return min(min(ctl[KM_KEFF], k), j_limit);  // (clamped to k: no word of the workspace leads a kernel out of its arrays)
}

__global__ void __launch_bounds__(256) kmeans_init_kernel(u32 B, u32 S, u32 k, u32 root, u32 have_seeds, KmeansSeeds seeds, const u64 *clade, u32 *ctl, u32 *active,
                                                          u32 *assign, double *dist, u32 *sizes, double *within, u32 *info) {
    __shared__ u32 count[256], first[256];
    __shared__ u32 bad_seed;
    const u32 tid = threadIdx.x;
    if (tid == 0) bad_seed = 0;
    u32 n = 0, lo = KMEANS_FILLER;
    for (u32 s = tid; s < S; s += 256) {
        const u32 on = clade[(u64)s * B + root] != 0 ? 1u : 0u;
        active[s] = on;
        assign[s] = KMEANS_FILLER;
        dist[s] = 0.0;
        n += on;
        if (on && lo == KMEANS_FILLER) lo = s;
    }
    count[tid] = n;
    first[tid] = lo;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            count[tid] += count[tid + o];
            first[tid] = min(first[tid], first[tid + o]);
        }
    }
    __syncthreads();
    if (tid < k) {
        sizes[tid] = 0;
        within[tid] = 0.0;
        if (have_seeds) {
            ctl[KM_SEEDS + tid] = seeds.s[tid];
            if (clade[(u64)seeds.s[tid] * B + root] == 0) bad_seed = 1;  // (the host has checked the index; any thread's store will do)
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const u32 n_active = count[0], status = have_seeds ? bad_seed : 0u, k_eff = have_seeds ? k : min(k, n_active);
    const u32 over = n_active == 0 || status != 0 ? 1u : 0u;
    ctl[KM_DONE] = over;
    ctl[KM_KEFF] = k_eff;
    ctl[KM_NACTIVE] = n_active;
    ctl[KM_STATUS] = status;
    info[0] = k_eff;
    info[1] = n_active;
    info[2] = 0;
    info[3] = 1u | status << 1;  // (the fillers' word: the last round writes its own)
    if (!have_seeds && n_active) {
        ctl[KM_SEEDS] = first[0];
        active[first[0]] = 3;  // bit 1: a seed
    }
}

__global__ void __launch_bounds__(256) kmeans_gather_kernel(u32 B, u32 S, u32 k, u32 j_first, const u32 *ctl, const double *U, const double *V, double *cu, double *cv) {
    const u32 j = j_first + blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (j >= kmeans_j_hi(ctl, k, k) || x >= B) return;
    const u32 s = min(ctl[KM_SEEDS + j], S - 1);
    cu[(u64)j * B + x] = U[(u64)x * S + s];
    cv[(u64)j * B + x] = V[(u64)x * S + s];
}

template <u32 KC>
__global__ void __launch_bounds__(KMEANS_WAVE) kmeans_dist_kernel(u32 B, u32 S, u32 k, u32 j_base, u32 j_limit, const u32 *ctl, const u32 *active, const double *U,
                                                                  const double *V, const double *h, const double *cu, const double *cv, double *part) {
    constexpr u32 TILE = KmeansTile<KC>::ids;
    __shared__ double uh[TILE];
    __shared__ __attribute__((aligned(16))) double uc[TILE][KC][2];  // cu_j, cv_j of a node side by side: one 16-byte broadcast read a centroid
    const u32 j_hi = kmeans_j_hi(ctl, k, j_limit), j0 = j_base + blockIdx.z * KC;
    if (j0 >= j_hi) return;
    const u32 t = blockIdx.y * KMEANS_WAVE + threadIdx.x;
    const bool need = t < S && (active[t] & 1u) != 0;
    if (!__syncthreads_or(need)) return;  // the block's samples are all inactive
    const u32 x_lo = blockIdx.x * KR_CHUNK_IDS, x_hi = min(x_lo + KR_CHUNK_IDS, B);
    const u32 tc = t < S ? t : S - 1;  // (lanes without a sample of their own read the last one's and write nothing)
    double acc[KC];
#pragma unroll
    for (u32 jj = 0; jj < KC; jj++) acc[jj] = 0.0;
    auto term = [&](u32 i, double u, double v) {  // node i of the tile: the centroid is the first operand
        const double hx = uh[i];
#pragma unroll
        for (u32 jj = 0; jj < KC; jj++) {
            const double2 c = *(const double2 *)uc[i][jj];
            acc[jj] = kr_term(acc[jj], hx, c.x, u, c.y, v);
        }
    };
    for (u32 y_lo = x_lo; y_lo < x_hi; y_lo += TILE) {  // the tiles of the chunk in ascending id: the sums run on across them
        const u32 n = min(TILE, x_hi - y_lo);
        __syncthreads();  // the tile before this one has been read
        for (u32 i = threadIdx.x; i < n; i += KMEANS_WAVE) uh[i] = h[y_lo + i];
#pragma unroll
        for (u32 jj = 0; jj < KC; jj++) {
            const u64 row = (u64)min(j0 + jj, j_hi - 1) * B + y_lo;  // (slots behind the last centroid sum it again and write nothing)
            for (u32 i = threadIdx.x; i < n; i += KMEANS_WAVE) {
                uc[i][jj][0] = cu[row + i];
                uc[i][jj][1] = cv[row + i];
            }
        }
        __syncthreads();
        node_ring<KMEANS_UNROLL, KMEANS_DEPTH>(  // (rk_samples.h; a batch reads nothing beside its loads: the tile's LDS words are read in the sum)
            U + tc, V + tc, S, y_lo, n, [](u32) { return 0; },
            [&](int, u32 x0, const double(&lu)[KMEANS_UNROLL], const double(&lv)[KMEANS_UNROLL]) {
#pragma unroll
                for (u32 i = 0; i < KMEANS_UNROLL; i++) term(x0 - y_lo + i, lu[i], lv[i]);
            },
            [&](u32 x, double u, double v) { term(x - y_lo, u, v); });
    }
    if (!need) return;
#pragma unroll
    for (u32 jj = 0; jj < KC; jj++)
        if (j0 + jj < j_hi) part[((u64)blockIdx.x * k + j0 + jj) * S + t] = acc[jj];
}

__global__ void __launch_bounds__(256) kmeans_reduce_kernel(u32 S, u32 k, u32 n_chunks, u32 j_base, u32 j_limit, const u32 *ctl, const u32 *active, const double *part,
                                                            u32 *best, double *bestd) {
    const u32 j_hi = kmeans_j_hi(ctl, k, j_limit), s = blockIdx.x * 256 + threadIdx.x;
    if (j_base >= j_hi || s >= S || !(active[s] & 1u)) return;
    u32 bj = j_base;
    double bd = 0.0;
    for (u32 j = j_base; j < j_hi; j++) {
        const double d = chunk_sum(n_chunks, [&](u32 c) { return part[((u64)c * k + j) * S + s]; });
        if (j == j_base || d < bd) {
            bd = d;
            bj = j;
        }
    }
    best[s] = bj;
    bestd[s] = bd;
}

struct KmeansFar {
    double m;
    u32 s;
};
__device__ __forceinline__ void kmeans_far_take(KmeansFar &x, const KmeansFar &y) {  // the larger minimum, ties to the smaller sample
    if (y.s != KMEANS_FILLER && (x.s == KMEANS_FILLER || y.m > x.m || (y.m == x.m && y.s < x.s))) x = y;
}

// seed j from the distances to seed j - 1 (bestd, of kmeans_reduce_kernel over that one centroid)
__global__ void __launch_bounds__(256) kmeans_seed_kernel(u32 S, u32 k, u32 j, u32 *ctl, u32 *active, const double *bestd, double *mind) {
    __shared__ KmeansFar cand[256];
    if (j >= kmeans_j_hi(ctl, k, k)) return;
    const u32 tid = threadIdx.x;
    KmeansFar mine{0.0, KMEANS_FILLER};
    for (u32 s = tid; s < S; s += 256) {
        const u32 a = active[s];
        if (!(a & 1u)) continue;
        const double d = bestd[s];
        const double m = j == 1 || d < mind[s] ? d : mind[s];
        mind[s] = m;
        if (!(a & 2u)) kmeans_far_take(mine, KmeansFar{m, s});
    }
    cand[tid] = mine;
    for (u32 o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            KmeansFar x = cand[tid];
            kmeans_far_take(x, cand[tid + o]);
            cand[tid] = x;
        }
    }
    if (tid != 0) return;
    const u32 s = cand[0].s;
    ctl[KM_SEEDS + j] = s;
    if (s < S) active[s] = 3;
}

__global__ void __launch_bounds__(256) kmeans_assign_kernel(u32 S, u32 k, u32 round, u32 max_rounds, u32 *ctl, const u32 *active, const u32 *best, const double *bestd,
                                                            u32 *assign, double *dist, u32 *members, u32 *sizes, double *within, u32 *info) {
    __shared__ u32 count[KMEANS_MAX_CENTROIDS], tile_a[256];
    __shared__ double tile_d[256];
    __shared__ u32 changed;
    if (kmeans_j_hi(ctl, k, k) == 0) return;
    const u32 tid = threadIdx.x;
    if (tid < KMEANS_MAX_CENTROIDS) count[tid] = 0;
    if (tid == 0) changed = 0;
    __syncthreads();
    u32 ch = 0;
    for (u32 s = tid; s < S; s += 256) {
        if (!(active[s] & 1u)) continue;
        const u32 b = min(best[s], k - 1);
        ch += assign[s] != b;
        assign[s] = b;
        dist[s] = bestd[s];
        atomicAdd(&count[b], 1u);
    }
    if (ch) atomicAdd(&changed, ch);
    __syncthreads();
    const bool last = changed == 0 || round + 1 == max_rounds;
    if (tid < k) {
        members[tid] = count[tid];  // (kmeans_update_kernel divides by them)
        sizes[tid] = count[tid];
    }
    if (!last) return;
    // within[j]: thread j adds the dist of its members in ascending s; a tile of 256 samples goes through the LDS (s = s0 + tid is one
    // of this thread's own samples: it reads back what it wrote above)
    double w = 0.0;
    for (u32 s0 = 0; s0 < S; s0 += 256) {
        __syncthreads();
        const u32 s = s0 + tid;
        tile_a[tid] = s < S ? assign[s] : KMEANS_FILLER;
        tile_d[tid] = s < S ? dist[s] : 0.0;
        __syncthreads();
        if (tid < k) {
            const u32 n = min(256u, S - s0);
            for (u32 i = 0; i < n; i++)
                if (tile_a[i] == tid) w = w + tile_d[i];
        }
    }
    if (tid < k) within[tid] = w;
    if (tid != 0) return;
    info[2] = round + 1;
    info[3] = changed == 0 ? 1u : 0u;
    if (changed == 0) ctl[KM_DONE] = 1;  // converged: this round's update and every kernel behind it return at once
}

// One wave a block.  With KP the power of two that holds the k clusters, the wave takes up to 64 / KP nodes (2^nodes_log2 of them: the
// launch takes fewer where the tree is too small to fill the device otherwise): lane = node of the wave * KP + cluster.  A tile of T
// samples (512 / the nodes of the wave, at most a group) of those nodes' two rows goes through the LDS with the samples' clusters;
// a lane walks it in ascending s and adds its members to the group's partial, and folds the partial into its sum where the group
// ends.  (One node a wave and one lane a cluster left 62 of 64 lanes idle at k = 2: the walk over the samples is the same for every
// node, so the nodes share it.)
__global__ void __launch_bounds__(KMEANS_WAVE) kmeans_update_kernel(u32 B, u32 S, u32 k, u32 kp_log2, u32 nodes_log2, const u32 *ctl, const u32 *assign, const u32 *members,
                                                                    const double *U, const double *V, double *cu, double *cv) {
    __shared__ u32 who[KMEANS_UPDATE_GROUP];
    __shared__ __attribute__((aligned(16))) double uv[KMEANS_UPDATE_ENTRIES][2];  // [node of the wave][sample of the tile]
    const u32 k_eff = kmeans_j_hi(ctl, k, k);
    if (k_eff == 0) return;
    const u32 lane = threadIdx.x, nodes = 1u << nodes_log2, t_log2 = min(9u - nodes_log2, 8u), T = 1u << t_log2;
    const u32 mine_node = min(lane >> kp_log2, nodes - 1), j = lane >> kp_log2 < nodes ? lane & ((1u << kp_log2) - 1u) : KMEANS_FILLER;  // (lanes behind the last node own no cluster)
    const u32 x0 = blockIdx.x * nodes, x = x0 + mine_node;
    const double2 *row = (const double2 *)uv[mine_node << t_log2];
    double su = 0.0, sv = 0.0;
    u32 seen = 0;
    for (u32 g0 = 0; g0 < S; g0 += KMEANS_UPDATE_GROUP) {
        double gu = 0.0, gv = 0.0;
        u32 in_group = 0;
        for (u32 t0 = g0; t0 < g0 + KMEANS_UPDATE_GROUP && t0 < S; t0 += T) {
            __syncthreads();  // the tile before this one has been read
            for (u32 i = lane; i < T; i += KMEANS_WAVE) who[i] = t0 + i < S ? assign[t0 + i] : KMEANS_FILLER;
            for (u32 e = lane; e < nodes << t_log2; e += KMEANS_WAVE) {
                const u32 xe = min(x0 + (e >> t_log2), B - 1), s = t0 + (e & (T - 1));  // (a node behind the last reads the last one's and writes nothing)
                uv[e][0] = s < S ? U[(u64)xe * S + s] : 0.0;
                uv[e][1] = s < S ? V[(u64)xe * S + s] : 0.0;
            }
            __syncthreads();
            const u32 n = min(T, S - t0);
            for (u32 sl = 0; sl < n; sl++) {
                const double2 q = row[sl];
                const bool mine = who[sl] == j;  // (a sample without mass belongs to no cluster: its NaNs are never added)
                gu = mine ? gu + q.x : gu;
                gv = mine ? gv + q.y : gv;
                in_group += mine;
            }
        }
        if (in_group) {
            su = seen ? su + gu : gu;
            sv = seen ? sv + gv : gv;
            seen = 1;
        }
    }
    if (x >= B || j >= k_eff) return;
    const u32 n = members[j];
    if (n == 0) return;  // a cluster that lost every member keeps its profile
    cu[(u64)j * B + x] = su / (double)n;
    cv[(u64)j * B + x] = sv / (double)n;
}

__global__ void __launch_bounds__(256) kmeans_centroids_kernel(u32 B, u32 k, const u32 *ctl, const double *cu, const double *cv, double *out) {
    const u32 j = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= B) return;
    const bool on = ctl[KM_NACTIVE] != 0 && ctl[KM_STATUS] == 0 && j < min(ctl[KM_KEFF], k);
    out[((u64)j * 2) * B + x] = on ? cu[(u64)j * B + x] : 0.0;
    out[((u64)j * 2 + 1) * B + x] = on ? cv[(u64)j * B + x] : 0.0;
}

}  // namespace rk
