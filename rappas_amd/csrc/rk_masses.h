// rk_masses.h -- #included by rk_kernels.hip: the two edge-mass kernels and the pieces they are written over, each
// defined once -- the term of a row, the claim of a slot of the LDS cache, the attribution of skipped rows to the lanes that own
// their reads, the flush of the four totals and of the claimed slots.  The launches and the entry points are in rk_masses_impl.h,
// the host twins in rk_masses_host.h.  Not part of the C ABI.
#pragma once
#include "rk_device.h"

namespace rk {

// ------------------------------------------------------------------------------------------------
// Edge masses: the per-branch LWR sums of a result set.  out = mass_q30[B] | best[B] | four totals, 64-bit words the
// call ADDS into.  Every term is an integer -- an LWR enters as q = rint(min(l, 1) * 2^30), times the read's weight -- so the sums do
// not depend on the order of the atomic adds.  The reference has no counterpart (it writes one jplace record per read).
//
// masses_kernel: a histogram with hot spots (a clade-shaped batch puts most rows on a handful of branches).  A wave takes 64 reads,
// as merge_results_kernel does: a lane loads n_rows and the weight of one read, then the wave walks the 64 * K rows lane after lane
// along the flattened arrays (the branch and lwr loads coalesce) and takes n_rows and w of the read that owns the row by shuffle.
//   LDS_BINS   small trees: the block's mass and best live in the LDS (64-bit integer LDS atomics), are flushed once at the end, the
//              non-zero bins only, one global atomic per bin and block; the grid is a small multiple of the CU count, not a block
//              per 256 reads, since the flush costs blocks x B.
//   CACHE      large trees (B above the LDS limit): 64-bit global atomics into `out`, behind a per-block LDS table of MASS_CACHE_SLOTS
//              slots {branch key, mass, best} for the busiest bins.  A lane with a counted row of branch x reads the two keys of
//              the pair of slots mass_cache_slot(x) names: a key that is x is a hit; an empty key is claimed with a 32-bit LDS
//              compare-and-swap, and the claim counts as a hit when it succeeds or finds x already there.  A hit adds in the LDS;
//              anything else does the global atomics exactly as the direct variant.  A slot keeps its branch until the block ends
//              (no eviction), so a key that was read non-empty is final and claim, add and flush need no order between them.  After
//              the last barrier the block flushes the non-zero words of its claimed slots, one global atomic each.
//              A row either adds in the LDS or issues the direct variant's atomics, and a non-zero flushed word has had at least
//              one row that the direct variant would have sent to that very address (which sends the mass word even when it is
//              zero): on the same grid the cached variant never issues more global atomics than the direct one, on any input.
//              A wave-uniform hit-rate test after which a wave stops consulting the table, and a sum of equal branches among the
//              lanes of a wave before the atomics, were built and measured: neither helps a shipped case (DESIGN.md 4.7 has the
//              numbers) and neither is here.
//   otherwise  large trees, direct: 64-bit global atomics straight into `out` (developer build: RK_MASSES_VARIANT=global).
// A row whose branch is >= B is never an index: it is skipped and counted (word 2B+3), and takes no part in any other word.  That
// needs the number of skipped rows per READ while the rows sit in other lanes: the wave ballots the skip (all zero on the engine's
// own results) and, in the rare case, walks the set bits to the lanes that own the reads.  The four totals stay in registers, are
// reduced across the wave by shuffles and added to four LDS words, which the block flushes with the bins.
// No 64-bit shift by a per-lane count anywhere.
// ------------------------------------------------------------------------------------------------
constexpr u32 MASS_NO_BRANCH = 0xFFFFFFFFu;  // no slot; an empty key of the cache (a branch id is below 65 536)
// 512 slots of 20 bytes and the totals are 10 272 bytes of LDS: the eight blocks a CU that the wave limit gives the direct variant stay
constexpr u32 MASS_CACHE_SLOTS = 512;
// The first slot of x's pair: the top bits of a multiplicative hash, so that the consecutive pre-order ids of a clade neighbourhood,
// and ids a power of two apart, land in different pairs.
__device__ __forceinline__ u32 mass_cache_slot(u32 x) { return ((x * 0x9E3779B1u) >> 24) << 1; }
static_assert(MASS_CACHE_SLOTS == 512, "mass_cache_slot: 8 bits of pair index, two slots a pair");

// The term of row j of a read of weight w on branch x: false when the row is skipped (x >= B: never an index, its LWR is not
// loaded); else cv, the weighted mass, and cb, the weight for best (row 0 only).
__device__ __forceinline__ bool mass_row_term(u32 x, u32 B, const double *lwr, u32 w, u32 j, u64 &cv, u64 &cb) {
    if (x >= B) return false;
    const double l = *lwr;
    const u32 q = l >= 0.0 ? (u32)__builtin_rint(fmin(l, 1.0) * 1073741824.0) : 0u;  // (NaN: 0)
    cv = (u64)w * q;
    cb = j == 0 ? w : 0u;
    return true;
}

// The slot of the cache that holds key ck (never MASS_NO_BRANCH), claimed now if one of its pair is empty; MASS_NO_BRANCH when both
// hold other keys.
__device__ __forceinline__ u32 mass_cache_claim(u32 *key, u32 ck) {
    const u32 s0 = mass_cache_slot(ck);
    u32 k0 = __hip_atomic_load(&key[s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    u32 k1 = __hip_atomic_load(&key[s0 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k0 == MASS_NO_BRANCH) {
        k0 = atomicCAS(&key[s0], MASS_NO_BRANCH, ck);
        if (k0 == MASS_NO_BRANCH) k0 = ck;
    }
    if (k0 == ck) return s0;
    if (k1 == MASS_NO_BRANCH) {
        k1 = atomicCAS(&key[s0 + 1], MASS_NO_BRANCH, ck);
        if (k1 == MASS_NO_BRANCH) k1 = ck;
    }
    return k1 == ck ? s0 + 1 : MASS_NO_BRANCH;
}

// The rows skipped in one step of the walk, handed to the lanes that own their reads: lane b holds row e0 + b of the 64 * K, a row
// of read (e0 + b) / K.  Executed by the whole wave; the loop is wave-uniform and never entered on the engine's own results.
__device__ __forceinline__ void mass_skips_to_owners(bool skipped, u32 e0, u32 K, u32 lane, u32 &my_skips) {
    u64 sk = __ballot(skipped);
    while (sk) {
        const u32 bit = (u32)__ffsll((long long)sk) - 1u;
        sk &= sk - 1;
        if (lane == (e0 + bit) / K) my_skips++;
    }
}

// the four sums of a wave: reduced across it, lane 0 adds the non-zero ones at tot[0 .. 3]; the registers start again at zero
__device__ __forceinline__ void mass_totals_flush(u64 *tot, u32 lane, u64 &t_all, u64 &t_placed, u64 &t_rows, u64 &t_skip) {
    for (int o = 32; o > 0; o >>= 1) {
        t_all += __shfl_down(t_all, o, 64);
        t_placed += __shfl_down(t_placed, o, 64);
        t_rows += __shfl_down(t_rows, o, 64);
        t_skip += __shfl_down(t_skip, o, 64);
    }
    if (lane == 0) {
        if (t_all) atomicAdd(&tot[0], t_all);
        if (t_placed) atomicAdd(&tot[1], t_placed);
        if (t_rows) atomicAdd(&tot[2], t_rows);
        if (t_skip) atomicAdd(&tot[3], t_skip);
    }
    t_all = t_placed = t_rows = t_skip = 0;
}

// After the last barrier: the non-zero words of the claimed slots to their bins, one global atomic each.  bin_of(key) is the word of
// `out` that holds the mass of the key's bin (a claimed slot holds a counted row's key: in range); its best lies B words behind.
template <class F>
__device__ __forceinline__ void mass_cache_flush(const u64 *mass_lds, const u32 *key, u64 *out, u32 B, F bin_of) {
    for (u32 i = threadIdx.x; i < MASS_CACHE_SLOTS; i += 256) {
        const u32 ck = key[i];
        if (ck != MASS_NO_BRANCH) {
            const u32 bin = bin_of(ck);
            const u64 v = mass_lds[i], b = mass_lds[MASS_CACHE_SLOTS + i];
            if (v) atomicAdd(&out[bin], v);
            if (b) atomicAdd(&out[bin + B], b);
        }
    }
}

template <bool LDS_BINS, bool CACHE>
__global__ void __launch_bounds__(256) masses_kernel(u64 n_reads, u32 K, u32 B, const unsigned char *n_rows, const unsigned short *branch,
                                                     const double *lwr, const u32 *weights, u64 *out) {
    static_assert(!(LDS_BINS && CACHE), "the cache stands in front of the global atomics");
    // LDS_BINS: mass[B] | best[B] | totals[4]; CACHE: mass[S] | best[S] | totals[4] | key[S] (32-bit); otherwise totals[4]
    extern __shared__ u64 mass_lds[];
    const u32 n_lds = LDS_BINS ? 2u * B + 4u : CACHE ? 2u * MASS_CACHE_SLOTS + 4u : 4u;
    for (u32 i = threadIdx.x; i < n_lds; i += 256) mass_lds[i] = 0;
    u32 *const key = (u32 *)(mass_lds + n_lds);
    if (CACHE)
        for (u32 i = threadIdx.x; i < MASS_CACHE_SLOTS; i += 256) key[i] = MASS_NO_BRANCH;
    __syncthreads();
    u64 *tot = mass_lds + (n_lds - 4u);
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    u64 t_all = 0, t_placed = 0, t_rows = 0, t_skip = 0;
    for (u64 r0 = wave * 64; r0 < n_reads; r0 += n_waves * 64) {
        const u64 r = r0 + lane;
        u32 nr = 0, w = 0;
        if (r < n_reads) {
            nr = n_rows[r];
            nr = nr < K ? nr : K;
            w = weights ? weights[r] : 1u;
        }
        u32 my_skips = 0;  // rows of THIS lane's read with a branch >= B
        for (u32 e = lane; e < 64u * K; e += 64) {  // (uniform trip count: shuffles and the ballot are executed by the whole wave)
            const u32 rr = e / K, j = e - rr * K;
            const u32 nr_e = (u32)__shfl((int)nr, (int)rr, 64), w_e = (u32)__shfl((int)w, (int)rr, 64);
            bool skipped = false;
            if (j < nr_e) {  // (nr == 0 beyond the batch: no row of such a read is loaded)
                const u64 g = r0 * K + e;
                const u32 x = branch[g];
                u64 cv, cb;
                if (mass_row_term(x, B, &lwr[g], w_e, j, cv, cb)) {
                    const u32 slot = CACHE ? mass_cache_claim(key, x) : MASS_NO_BRANCH;
                    if (LDS_BINS) {
                        atomicAdd(&mass_lds[x], cv);
                        if (cb) atomicAdd(&mass_lds[B + x], cb);
                    } else if (slot != MASS_NO_BRANCH) {
                        atomicAdd(&mass_lds[slot], cv);
                        if (cb) atomicAdd(&mass_lds[MASS_CACHE_SLOTS + slot], cb);
                    } else {
                        atomicAdd(&out[x], cv);
                        if (cb) atomicAdd(&out[B + x], cb);
                    }
                } else {
                    skipped = true;
                }
            }
            mass_skips_to_owners(skipped, e - lane, K, lane, my_skips);
        }
        const u32 counted = nr - my_skips;
        t_all += w;  // (w == 0 beyond the batch)
        if (counted) t_placed += w;
        t_rows += (u64)w * counted;
        t_skip += my_skips;
    }
    mass_totals_flush(tot, lane, t_all, t_placed, t_rows, t_skip);
    __syncthreads();
    if (CACHE) {  // the claimed slots, then the totals
        mass_cache_flush(mass_lds, key, out, B, [](u32 x) { return x; });
        if (threadIdx.x < 4 && tot[threadIdx.x]) atomicAdd(&out[2u * (u64)B + threadIdx.x], tot[threadIdx.x]);
        return;
    }
    u64 *dst = LDS_BINS ? out : out + 2u * (u64)B;
    for (u32 i = threadIdx.x; i < n_lds; i += 256) {
        const u64 v = mass_lds[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

// ------------------------------------------------------------------------------------------------
// Per-sample edge masses: the sums of masses_kernel, one mass buffer per sample, from a membership list of
// (read, sample, weight) entries.  out = S buffers of W = 2B + 4 words | one word: the entries skipped for sample >= S or read >=
// n_reads (never an index, as a branch >= B is not).  The call ADDS; every term is an integer.
//
// masses_samples_kernel: a wave takes 64 ENTRIES.  A lane loads its entry's read, sample and weight and n_rows of that read; an entry
// out of range becomes an empty lane (no rows, no totals) and is counted by ballot.  The wave then walks the 64 * K rows as
// masses_kernel does: read, sample, weight and row count reach the lane that holds a row by shuffle -- two shuffles a step more than
// masses_kernel's, which is why that one stays a kernel of its own -- the row lies at read * K + j (m_read == nullptr: entry i is
// read i, the coalesced walk of masses_kernel; otherwise K-row segments per read), its bin is sample * W + x in 32-bit arithmetic
// (S * W + 1 <= 2^29).
//   LDS_BINS   S * W + 1 <= 8192 words: every word of `out` is an LDS bin (64-bit integer LDS atomics), the totals and the skipped
//              entries among them; the block flushes its non-zero words.  Grid as masses_kernel's LDS variant.
//   otherwise  global atomics behind the LDS cache of masses_kernel: the same 512 slots in pairs, claimed by compare-and-swap, never
//              evicted, flushed at the end.  The key is sample << 16 | x -- never MASS_NO_BRANCH, since x < B <= 65535.
// The three totals and the skipped-row count of an entry belong to its sample.  While the 64 entries of a step carry one sample
// (a wave-uniform test: entries sorted or in runs), they stay in registers, per lane, across steps; when the sample changes, and at
// the end, they are reduced by shuffles and added once.  A step with several samples adds per lane.  Either add goes to the LDS
// bins, or -- the cached form -- to a second small LDS table of MASS_TOTAL_SLOTS slots {sample key, four totals}, slot sample mod
// MASS_TOTAL_SLOTS, claimed and flushed as the bins' slots are; a sample that does not hold its slot adds to global memory.
// (Per-lane global atomics alone put 10^7 entries of 8 samples on 24 addresses: 50 ms where the table takes 2.5)
// No 64-bit shift by a per-lane count anywhere.
// ------------------------------------------------------------------------------------------------
constexpr u32 MASS_NO_SAMPLE = 0xFFFFFFFFu;  // no run of one sample is open in this wave; an empty key of the totals' table (a sample index is below 65 535)
constexpr u32 MASS_TOTAL_SLOTS = 64;         // 64 * (4 * 8 + 4) = 2 304 bytes of LDS beside the bins' 10 256
static_assert((MASS_TOTAL_SLOTS & (MASS_TOTAL_SLOTS - 1)) == 0, "the slot of a sample is its low bits");

template <bool LDS_BINS>
__global__ void __launch_bounds__(256) masses_samples_kernel(u32 n_reads, u64 n_members, u32 K, u32 B, u32 S, const unsigned char *n_rows,
                                                             const unsigned short *branch, const double *lwr, const u32 *m_read,
                                                             const u32 *m_sample, const u32 *m_weight, u64 *out) {
    // LDS_BINS: the S * W + 1 words of `out`; otherwise mass[SLOTS] | best[SLOTS] | skipped entries, pad | totals[TOTAL_SLOTS][4] |
    // key[SLOTS] | total key[TOTAL_SLOTS] (32-bit)
    extern __shared__ u64 mass_lds[];
    const u32 W = 2u * B + 4u, SW = S * W;
    constexpr u32 TOT0 = 2u * MASS_CACHE_SLOTS + 2u;  // the first word of the totals' table
    const u32 n_lds = LDS_BINS ? SW + 1u : TOT0 + 4u * MASS_TOTAL_SLOTS;
    for (u32 i = threadIdx.x; i < n_lds; i += 256) mass_lds[i] = 0;
    u32 *const key = (u32 *)(mass_lds + n_lds), *const tkey = key + MASS_CACHE_SLOTS;
    if (!LDS_BINS)
        for (u32 i = threadIdx.x; i < MASS_CACHE_SLOTS + MASS_TOTAL_SLOTS; i += 256) key[i] = MASS_NO_BRANCH;  // (both tables' keys)
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    // where the four totals of sample s are added: its LDS bins; or (the cached form) its slot of the totals' table, if the sample
    // holds it or can claim it, else the words of `out`
    auto totals_of = [&](u32 s) -> u64 * {
        if (LDS_BINS) return mass_lds + (s * W + 2u * B);
        const u32 ts = s & (MASS_TOTAL_SLOTS - 1u);
        u32 tk = __hip_atomic_load(&tkey[ts], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tk == MASS_NO_SAMPLE) {
            tk = atomicCAS(&tkey[ts], MASS_NO_SAMPLE, s);
            if (tk == MASS_NO_SAMPLE) tk = s;
        }
        return tk == s ? mass_lds + (TOT0 + 4u * ts) : out + (s * W + 2u * B);
    };
    u32 run = MASS_NO_SAMPLE;  // wave-uniform: the sample whose totals the registers hold
    u64 t_all = 0, t_placed = 0, t_rows = 0, t_skip = 0;
    u32 bad_entries = 0;       // (lane 0 counts for the wave)
    for (u64 i0 = wave * 64; i0 < n_members; i0 += n_waves * 64) {
        const u64 i = i0 + lane;
        u32 rd = 0, sm = 0, w = 0, nr = 0;
        bool valid = false, bad = false;
        if (i < n_members) {
            rd = m_read ? m_read[i] : (u32)i;
            sm = m_sample[i];
            valid = rd < n_reads && sm < S;
            bad = !valid;
            if (valid) {
                w = m_weight ? m_weight[i] : 1u;
                nr = n_rows[rd];
                nr = nr < K ? nr : K;
            }
        }
        const u64 bad_mask = __ballot(bad);
        if (lane == 0) bad_entries += (u32)__popcll(bad_mask);
        u32 my_skips = 0;  // rows of THIS lane's entry with a branch >= B
        for (u32 e = lane; e < 64u * K; e += 64) {  // (uniform trip count: shuffles and the ballot are executed by the whole wave)
            const u32 rr = e / K, j = e - rr * K;
            const u32 nr_e = (u32)__shfl((int)nr, (int)rr, 64), w_e = (u32)__shfl((int)w, (int)rr, 64);
            const u32 rd_e = (u32)__shfl((int)rd, (int)rr, 64), sm_e = (u32)__shfl((int)sm, (int)rr, 64);
            bool skipped = false;
            if (j < nr_e) {  // (nr == 0 for an empty lane: no row of such an entry is loaded)
                const u64 g = (u64)rd_e * K + j;
                const u32 x = branch[g];
                u64 cv, cb;
                if (mass_row_term(x, B, &lwr[g], w_e, j, cv, cb)) {
                    const u32 bin = sm_e * W + x;
                    const u32 slot = LDS_BINS ? MASS_NO_BRANCH : mass_cache_claim(key, (sm_e << 16) | x);
                    if (LDS_BINS) {
                        atomicAdd(&mass_lds[bin], cv);
                        if (cb) atomicAdd(&mass_lds[bin + B], cb);
                    } else if (slot != MASS_NO_BRANCH) {
                        atomicAdd(&mass_lds[slot], cv);
                        if (cb) atomicAdd(&mass_lds[MASS_CACHE_SLOTS + slot], cb);
                    } else {
                        atomicAdd(&out[bin], cv);
                        if (cb) atomicAdd(&out[bin + B], cb);
                    }
                } else {
                    skipped = true;
                }
            }
            mass_skips_to_owners(skipped, e - lane, K, lane, my_skips);
        }
        // this step's totals: into the open run when all its entries carry that one sample, else the run is closed first
        const u64 valid_mask = __ballot(valid);
        if (valid_mask == 0) continue;
        const u32 first = (u32)__ffsll((long long)valid_mask) - 1u;
        const u32 s_first = (u32)__shfl((int)sm, (int)first, 64);
        const bool uniform = __ballot(valid && sm != s_first) == 0;
        if (run != MASS_NO_SAMPLE && !(uniform && s_first == run)) {
            mass_totals_flush(totals_of(run), lane, t_all, t_placed, t_rows, t_skip);
            run = MASS_NO_SAMPLE;
        }
        const u32 counted = nr - my_skips;
        const u64 a = w, p = counted ? w : 0u, r = (u64)w * counted;  // (w == 0 and nr == 0 in an empty lane)
        if (uniform) {
            run = s_first;
            t_all += a; t_placed += p; t_rows += r; t_skip += my_skips;
        } else if (valid) {
            u64 *tot = totals_of(sm);
            if (a) atomicAdd(&tot[0], a);
            if (p) atomicAdd(&tot[1], p);
            if (r) atomicAdd(&tot[2], r);
            if (my_skips) atomicAdd(&tot[3], (u64)my_skips);
        }
    }
    if (run != MASS_NO_SAMPLE) mass_totals_flush(totals_of(run), lane, t_all, t_placed, t_rows, t_skip);
    if (lane == 0 && bad_entries) atomicAdd(&mass_lds[LDS_BINS ? SW : 2u * MASS_CACHE_SLOTS], (u64)bad_entries);
    __syncthreads();
    if (LDS_BINS) {
        for (u32 i = threadIdx.x; i < n_lds; i += 256) {
            const u64 v = mass_lds[i];
            if (v) atomicAdd(&out[i], v);
        }
        return;
    }
    mass_cache_flush(mass_lds, key, out, B, [W](u32 ck) { return (ck >> 16) * W + (ck & 0xFFFFu); });
    for (u32 i = threadIdx.x; i < 4u * MASS_TOTAL_SLOTS; i += 256) {  // the claimed totals' non-zero words to their samples
        const u32 tk = tkey[i >> 2];
        const u64 v = mass_lds[TOT0 + i];
        if (tk != MASS_NO_SAMPLE && v) atomicAdd(&out[tk * W + 2u * B + (i & 3u)], v);
    }
    if (threadIdx.x == 0 && mass_lds[2u * MASS_CACHE_SLOTS]) atomicAdd(&out[SW], mass_lds[2u * MASS_CACHE_SLOTS]);
}

}  // namespace rk
