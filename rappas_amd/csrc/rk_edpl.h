// rk_edpl.h -- #included by rk_kernels.hip behind rk_epca.h: the EDPL kernel (include/rappas_place.h holds the
// definition).  edpl[r] = 2 * the sum over the pairs i < j of a read's usable rows of (lwr_i * lwr_j) * d(branch_i, branch_j), d the
// path length between the midpoints of the two edges.  One double a read, written; no atomics, one owner and one fixed order per sum,
// so the bits depend on neither grid nor stream.  The launch and the entry points are in rk_samples_impl.h, the tables' builder and
// the host twin in rk_samples_host.h.
//
// edpl_kernel: a wave takes 64 reads, as masses_kernel does.  A lane loads n_rows of one read; the wave then walks the 64 * K rows
// lane after lane along the flattened arrays (the branch and lwr loads coalesce) and the lane that holds a row gathers what a pair
// needs of its branch -- pos and the pre-order interval, one 16-byte EdplEntry -- and puts weight, pos and interval into the wave's
// stage in the LDS, at read * (K | 1) + row (the odd stride keeps the owners' 8-byte reads off each other's banks).  A row that is
// not usable (branch >= B, never an index; lwr not above 0, NaN included) is staged with weight 0 and skipped by that mark.  Then
// lane l owns the pairs of read l: i ascending, j > i ascending, row i in registers, row j from the stage.  Per pair: two compares
// for the ancestor case, else two 16-bit reads of the sparse table, two of the depths, one binary64 read of D[l]: five dependent-free
// or once-dependent reads whatever the depth of the tree.
//   LDS_TABLES   the block of dpar | depth | table (rk_samples_host.h) is copied into the LDS of every block once, ahead of the stages;
//                one block a CU, of as many waves as the LDS behind the tables holds stages for (the launch decides: the kernel takes
//                its waves from blockDim), so that the copy is paid once a CU and the walk's loads have waves to hide behind
//   otherwise    the same words are read from global memory (2.75 MB at 65 535 branches: L2-resident); blocks of four waves
// The per-node entries are read from global memory in both forms: once a row, not once a pair.
// No 64-bit shift anywhere.
#pragma once
#include "rk_epca.h"

namespace rk {

struct EdplEntry {  // rk::EdplNode of the host side
    double pos;
    u32 pre, end;
};

constexpr u32 EDPL_MAX_WAVES = 16;  // waves of a block: 4 without the tables, up to 16 with them
// bytes of the stage of one wave: weight and pos (binary64) and pre | end << 16 for 64 reads of K | 1 rows
__host__ __device__ constexpr u32 edpl_stage_bytes(u32 K) { return 64u * (K | 1u) * 20u; }

// d(a, b) from the staged words of the two rows; pa != pb is not required
__device__ __forceinline__ double edpl_distance(double pos_a, u32 pe_a, double pos_b, u32 pe_b, u32 B, const double *dpar, const unsigned short *depth,
                                                const unsigned short *table) {
    const u32 pa = pe_a & 0xFFFFu, pb = pe_b & 0xFFFFu;
    if (pa == pb) return 0.0;
    const bool a_first = pa < pb;
    const u32 pf = a_first ? pa : pb, ps = a_first ? pb : pa, end_f = (a_first ? pe_a : pe_b) >> 16;
    if (ps < end_f) return a_first ? pos_b - pos_a : pos_a - pos_b;
    const u32 j = 31u - (u32)__builtin_clz(ps - pf);
    const unsigned short *row = table + j * B;  // (levels * B < 2^20)
    const u32 c1 = row[pf + 1u], c2 = row[ps + 1u - (1u << j)];
    const double dl = dpar[depth[c2] < depth[c1] ? c2 : c1];
    return (pos_a - dl) + (pos_b - dl);
}

template <bool LDS_TABLES>
__global__ void __launch_bounds__(64 * EDPL_MAX_WAVES) edpl_kernel(u64 n_reads, u32 K, u32 B, u32 lca_words, const unsigned char *n_rows, const unsigned short *branch,
                                                               const double *lwr, const EdplEntry *node, const u64 *lca, double *out) {
    // LDS_TABLES: the lca_words words of the tables | a stage per wave; otherwise the stages alone
    extern __shared__ u64 edpl_lds[];
    const u32 t_words = LDS_TABLES ? lca_words : 0u;
    if (LDS_TABLES) {
        for (u32 i = threadIdx.x; i < lca_words; i += blockDim.x) edpl_lds[i] = lca[i];
        __syncthreads();
    }
    const u64 *tables = LDS_TABLES ? edpl_lds : lca;
    const double *dpar = (const double *)tables;
    const unsigned short *depth = (const unsigned short *)(tables + B), *table = depth + B;
    const u32 Kp = K | 1u, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *s_w = (double *)(edpl_lds + t_words + (u64)wv * (edpl_stage_bytes(K) / 8u)), *s_pos = s_w + 64u * Kp;
    u32 *s_pe = (u32 *)(s_pos + 64u * Kp);
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 r0 = wave * 64; r0 < n_reads; r0 += n_waves * 64) {
        const u64 r = r0 + lane;
        u32 nr = 0;
        if (r < n_reads) {
            nr = n_rows[r];
            nr = nr < K ? nr : K;
        }
        for (u32 e = lane; e < 64u * K; e += 64) {  // (uniform trip count: the shuffle is executed by the whole wave)
            const u32 rr = e / K, j = e - rr * K;
            const u32 nr_e = (u32)__shfl((int)nr, (int)rr, 64);
            double w = 0.0, pos = 0.0;
            u32 pe = 0;
            if (j < nr_e) {  // (nr == 0 beyond the batch: no row of such a read is loaded)
                const u64 g = r0 * K + e;
                const u32 x = branch[g];
                if (x < B) {
                    const double l = lwr[g];
                    if (l > 0.0) {  // (NaN: not usable)
                        const EdplEntry nd = node[x];
                        w = l;
                        pos = nd.pos;
                        pe = nd.pre | (nd.end << 16);
                    }
                }
            }
            const u32 at = rr * Kp + j;
            s_w[at] = w;
            s_pos[at] = pos;
            s_pe[at] = pe;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the stage goes from the lanes that hold the rows to the lane that owns the read
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        const u32 base = lane * Kp;
        for (u32 i = 0; i + 1 < nr; i++) {
            const double wi = s_w[base + i];
            if (!(wi > 0.0)) continue;
            const double pos_i = s_pos[base + i];
            const u32 pe_i = s_pe[base + i];
            for (u32 j = i + 1; j < nr; j++) {
                const double wj = s_w[base + j];
                if (!(wj > 0.0)) continue;
                const double ww = wi * wj, d = edpl_distance(pos_i, pe_i, s_pos[base + j], s_pe[base + j], B, dpar, depth, table);
                const double term = ww * d;
                acc = acc + term;
            }
        }
        if (r < n_reads) out[r] = 2.0 * acc;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next step's rows overwrite the stage
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace rk
