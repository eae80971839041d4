// rk_diversity.h -- #included by rk_kernels.hip: the kernels of the per-sample diversity measures (include/rappas_place.h holds the
// definition).  After clade_masses_kernel the clade sums are on the device sample-major, as the masses are: a block
// that owns one (sample, chunk) reads its nodes as contiguous 8-byte words and needs neither the node-major profiles nor their
// transpose.  The terms are those of rk_divmath.h, the text the host twin compiles.  Plain launches in stream order, no atomics, no
// grid-wide wait; every sum has one owner and the order the definition fixes.
//   diversity_kernel<NT>     the hot path: (chunk of KR_CHUNK_IDS ids) x (sample), 256 threads = the 256 lanes of the definition.  A
//                            thread owns 5 + 2 NT running sums in registers and up to 8 nodes; per node two divisions, up to four
//                            logarithms (reused by every theta) and 4 NT exponentials, all binary64 VALU work.  The lane partials are
//                            folded by halving in the LDS, every column in the same step -> part[sample][chunk][column]
//   diversity_reduce_kernel  one thread a (sample, column): the chunk rule of rk_samplemath.h; the NaN row of a sample without
//                            mass, whose partials were never written and are not read
// Not part of the C ABI.
#pragma once
#include "rk_divmath.h"
#include "rk_samples.h"

namespace rk {

static_assert(KR_CHUNK_IDS % DIVERSITY_LANES == 0, "a lane takes whole strides of a chunk");

struct DiversityThetas {  // the caller's thetas as a kernel argument: no copy to order, nothing of the caller's read after the call
    double v[DIVERSITY_MAX_THETA];
};

template <u32 NT>
__global__ void __launch_bounds__(DIVERSITY_LANES) diversity_kernel(u32 B, u64 W, u32 root, u32 n_chunks, DiversityThetas thetas, const u64 *masses, const u64 *clade,
                                                                    const double *h, double *part) {
    constexpr u32 C = DIVERSITY_FIXED + 2 * NT;
    __shared__ double fold[C][DIVERSITY_LANES];
    const u32 tid = threadIdx.x, chunk = blockIdx.x, s = blockIdx.y;
    const u64 *c = clade + (u64)s * B, *m = masses + (u64)s * W;
    const u64 T = c[root];
    if (T == 0) return;  // (the whole block: the reduce writes the row)
    const u32 x_lo = chunk * KR_CHUNK_IDS, x_hi = min(x_lo + KR_CHUNK_IDS, B);
    double theta[NT > 0 ? NT : 1];
#pragma unroll
    for (u32 i = 0; i < NT; i++) theta[i] = thetas.v[i];
    double acc[C];
#pragma unroll
    for (u32 i = 0; i < C; i++) acc[i] = 0.0;
    for (u32 x = x_lo + tid; x < x_hi; x += DIVERSITY_LANES) diversity_node<NT>(c[x], m[x], T, h[x], theta, acc);
#pragma unroll
    for (u32 i = 0; i < C; i++) fold[i][tid] = acc[i];
    for (u32 stride = DIVERSITY_LANES / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        if (tid < stride) {
#pragma unroll
            for (u32 i = 0; i < C; i++) fold[i][tid] = fold[i][tid] + fold[i][tid + stride];
        }
    }
    __syncthreads();
    if (tid < C) part[((u64)s * n_chunks + chunk) * C + tid] = fold[tid][0];
}

__global__ void __launch_bounds__(256) diversity_reduce_kernel(u32 B, u32 S, u32 root, u32 n_chunks, u32 n_cols, const u64 *clade, const double *part, double *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= (u64)S * n_cols) return;
    const u32 s = (u32)(i / n_cols), col = (u32)(i % n_cols);
    if (clade[(u64)s * B + root] == 0) {
        out[i] = divmath_double(DIVERSITY_NAN);
        return;
    }
    const double *p = part + (u64)s * n_chunks * n_cols + col;
    out[i] = chunk_sum(n_chunks, [&](u32 k) { return p[(u64)k * n_cols]; });
}

}  // namespace rk
