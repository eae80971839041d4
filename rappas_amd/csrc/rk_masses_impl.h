// rk_masses_impl.h -- #included by rk_engine.hip: the edge-mass entry points (rk_masses_accumulate_device / _host and their per-sample
// forms) over masses_kernel and masses_samples_kernel (rk_masses.h) and their host twins (rk_masses_host.h).  The
// argument tests the four calls share, the grid rule of the two launches and the thread fan-out of the two host calls exist once.
// The calls work on the result of any placement entry point; they touch no placement kernel, no handle state and no launch scratch.
#pragma once

#include "rk_masses_host.h"

// Trees of up to this many branches keep mass[B] | best[B] | totals[4] in the LDS of every block: (2 * 4094 + 4) * 8 = 64 KB, so that
// two blocks still share a CU.  Above it the kernel adds straight into the buffer (DESIGN.md 4.7 holds the runs behind the value).
constexpr uint32_t RK_MASSES_LDS_MAX_BRANCHES = 4094;
constexpr uint32_t RK_MASSES_LDS_BLOCKS_PER_CU = 4;  // the flush costs blocks x B global atomics: a fixed multiple of the CU count
constexpr uint64_t RK_MASSES_SAMPLES_MAX_WORDS = 1ull << 29;  // 4 GiB: a word index is a 32-bit value inside the kernel
constexpr uint64_t RK_MASSES_SAMPLES_LDS_WORDS = 8192;        // the 64 KB of masses_kernel's LDS variant

extern "C" uint64_t rk_masses_words(uint32_t n_branches) { return n_branches >= 1 && n_branches <= 65535 ? 2ull * n_branches + 4 : 0; }

extern "C" uint64_t rk_masses_samples_words(uint32_t n_branches, uint32_t n_samples) {
    const uint64_t W = rk_masses_words(n_branches);
    if (!W || n_samples < 1 || n_samples > 65535) return 0;
    const uint64_t words = (uint64_t)n_samples * W + 1;
    return words <= RK_MASSES_SAMPLES_MAX_WORDS ? words : 0;
}

// The argument tests the four calls share, in two halves: the counts; then, in a call that has work, the arrays (score and flags are
// not read: they may be NULL).  `note` ends the n_reads text; a whole-batch call has no member_sample and passes has_samples = true.
static int masses_counts(const char *who, uint32_t K, uint64_t n_reads, const char *note) {
    if (K < 1 || K > 16) return fail(RK_ERR_INVALID, "%s: keep_at_most=%u outside 1..16", who, K);
    if (n_reads >= (1ull << 32)) return fail(RK_ERR_INVALID, "%s: n_reads=%llu, at most 2^32 - 1 per call%s", who, (unsigned long long)n_reads, note);
    return RK_OK;
}
static int masses_arrays(const char *who, const rk_result *res, bool has_samples, const uint64_t *masses) {
    if (!res || !res->n_rows || !res->branch || !res->lwr) return fail(RK_ERR_INVALID, "%s: null result array (n_rows, branch and lwr are read)", who);
    if (!has_samples) return fail(RK_ERR_INVALID, "%s: null member_sample", who);
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    return RK_OK;
}

// the tests of the two whole-batch calls
static int masses_args(const char *who, uint32_t K, uint64_t n_reads, const rk_result *res, const uint64_t *masses) {
    int rc = masses_counts(who, K, n_reads, " (the buffers of several calls add up)");
    if (rc || n_reads == 0) return rc;
    return masses_arrays(who, res, true, masses);
}

// the tests of the two per-sample calls: what is their own stands between the halves (n_reads == 0 does not end these calls)
static int masses_samples_args(const char *who, uint32_t B, uint32_t K, uint64_t n_reads, const rk_result *res, uint32_t S, uint64_t n_members,
                               const uint32_t *member_read, const uint32_t *member_sample, const uint64_t *masses) {
    if (int rc = masses_counts(who, K, n_reads, "")) return rc;
    if (n_members >= (1ull << 32)) return fail(RK_ERR_INVALID, "%s: n_members=%llu, at most 2^32 - 1 per call (the buffers of several calls add up)", who, (unsigned long long)n_members);
    if (!rk_masses_samples_words(B, S))
        return fail(RK_ERR_INVALID, "%s: n_samples=%u on %u branches: 1..65535 samples and at most 2^29 words (n_samples * (2 * n_branches + 4) + 1)", who, S, B);
    if (!member_read && n_members != n_reads)
        return fail(RK_ERR_INVALID, "%s: without member_read entry i is read i: n_members=%llu must equal n_reads=%llu", who, (unsigned long long)n_members, (unsigned long long)n_reads);
    if (n_members == 0) return RK_OK;
    return masses_arrays(who, res, member_sample != nullptr, masses);
}

// The grid of both launches over `units` reads or entries (a block's four waves take 64 each per step).  The LDS form flushes blocks x
// bins words, so its grid is a small multiple of the CU count; otherwise a block per 256 units, as the strand kernels have.
static unsigned masses_blocks(rk_db *db, bool lds, uint64_t units, uint32_t per_cu = RK_MASSES_LDS_BLOCKS_PER_CU) {
    const uint64_t tiles = (units + 255) / 256;
    return lds ? (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)db->cu_count * per_cu)) : strand_blocks(db, units);
}

// masses_kernel: LDS bins for small trees; for large ones global atomics behind a per-block LDS cache of the busiest bins
static int launch_masses(rk_db *db, uint32_t K, uint64_t n_reads, const rk_result *res, const uint32_t *weights, uint64_t *masses, hipStream_t s) {
    const uint32_t B = db->info.n_branches;
    bool lds = B <= RK_MASSES_LDS_MAX_BRANCHES;
    bool cache = !lds;
    uint32_t per_cu = RK_MASSES_LDS_BLOCKS_PER_CU;
    if (const char *v = rk_knob("RK_MASSES_VARIANT")) {  // developer builds: "lds" | "global" | "cache" (scripts/masses_rate.py)
        if (strstr(v, "global")) lds = false, cache = false;
        if (strstr(v, "cache")) lds = false, cache = true;
        if (strstr(v, "lds") && B <= RK_MASSES_LDS_MAX_BRANCHES) lds = true, cache = false;
    }
    if (const char *v = rk_knob("RK_MASSES_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(v));
    const unsigned blocks = masses_blocks(db, lds, n_reads, per_cu);
    const size_t lds_bytes = lds ? (size_t)(2 * B + 4) * 8 : cache ? (size_t)(2 * MASS_CACHE_SLOTS + 4) * 8 + (size_t)MASS_CACHE_SLOTS * 4 : 4 * 8;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds_bytes, s, (u64)n_reads, K, B, (const unsigned char *)res->n_rows, (const unsigned short *)res->branch,
                           (const double *)res->lwr, weights, (u64 *)masses);
    };
    if (lds) launch(masses_kernel<true, false>);
    else if (cache) launch(masses_kernel<false, true>);
    else launch(masses_kernel<false, false>);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_masses_accumulate_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, const uint32_t *d_weights,
                                           uint64_t *d_masses, void *stream) {
    if (!db) return fail(RK_ERR_INVALID, "rk_masses_accumulate_device: null handle");
    int rc = masses_args("rk_masses_accumulate_device", keep_at_most, n_reads, d_res, d_masses);
    if (rc || n_reads == 0) return rc;
    HIP_TRY(hipSetDevice(db->info.device));
    return launch_masses(db, keep_at_most, n_reads, d_res, d_weights, d_masses, (hipStream_t)stream);
}

// The thread fan-out of the two host calls: work(t, m) for t = 0 .. T - 1, T - 1 of them on threads of their own, joined on every way
// out; a thread that would not start has its share done here.  `partial`: every t sums into `words` words of its own, added to
// `masses` at the end (integers: any order gives the same words); otherwise every t adds straight into `masses`.
template <class Work>
static int masses_fan_out(const char *who, uint64_t T, uint64_t words, bool partial, uint64_t *masses, Work work) {
    std::vector<uint64_t> part;
    if (partial) {
        try {
            part.assign(T * words, 0);
        } catch (const std::bad_alloc &) {
            return fail(RK_ERR_NOMEM, "%s: no memory for %llu partial buffers", who, (unsigned long long)T);
        }
    }
    auto share = [&](uint64_t t) { work(t, partial ? part.data() + t * words : masses); };
    {
        struct JoinAll {
            std::vector<std::thread> v;
            ~JoinAll() { for (std::thread &t : v) if (t.joinable()) t.join(); }
        } th;
        try {
            th.v.reserve(T);
            for (uint64_t t = 1; t < T; t++) th.v.emplace_back([&share, t]() { share(t); });
        } catch (const std::exception &) {  // (a share that adds straight into `masses` may already be under way: none is given up)
        }
        share(0);
        for (uint64_t t = th.v.size() + 1; t < T; t++) share(t);
    }
    for (uint64_t t = 0; partial && t < T; t++)
        for (uint64_t i = 0; i < words; i++) masses[i] += part[t * words + i];
    return RK_OK;
}

extern "C" int rk_masses_accumulate_host(uint32_t n_branches, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, const uint32_t *weights,
                                         uint64_t *masses, uint32_t n_threads) {
    const char *who = "rk_masses_accumulate_host";
    if (n_branches < 1 || n_branches > 65535) return fail(RK_ERR_INVALID, "%s: n_branches=%u must be in 1..65535", who, n_branches);
    int rc = masses_args(who, keep_at_most, n_reads, res, masses);
    if (rc || n_reads == 0) return rc;
    unsigned hw = std::thread::hardware_concurrency();
    uint64_t T = n_threads ? n_threads : std::min(hw ? hw : 1u, 16u);
    T = std::max<uint64_t>(1, std::min<uint64_t>({T, 256, (n_reads + 4095) / 4096}));  // (a thread pays for a buffer of its own)
    return masses_fan_out(who, T, 2ull * n_branches + 4, T > 1, masses, [&](uint64_t t, uint64_t *m) {
        rk::masses_range(n_branches, keep_at_most, n_reads * t / T, n_reads * (t + 1) / T, res->n_rows, res->branch, res->lwr, weights, m);
    });
}

// masses_samples_kernel: a kernel of its own -- rk_masses_accumulate_device launches what it always did
extern "C" int rk_masses_accumulate_samples_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, uint32_t n_samples,
                                                   uint64_t n_members, const uint32_t *d_member_read, const uint32_t *d_member_sample,
                                                   const uint32_t *d_member_weight, uint64_t *d_masses, void *stream) {
    const char *who = "rk_masses_accumulate_samples_device";
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    const uint32_t B = db->info.n_branches;
    int rc = masses_samples_args(who, B, keep_at_most, n_reads, d_res, n_samples, n_members, d_member_read, d_member_sample, d_masses);
    if (rc || n_members == 0) return rc;
    HIP_TRY(hipSetDevice(db->info.device));
    const uint64_t words = rk_masses_samples_words(B, n_samples);
    const bool lds = words <= RK_MASSES_SAMPLES_LDS_WORDS;
    const unsigned blocks = masses_blocks(db, lds, n_members);
    const size_t lds_bytes = lds ? (size_t)words * 8 : (size_t)(2 * MASS_CACHE_SLOTS + 2 + 4 * MASS_TOTAL_SLOTS) * 8 + (size_t)(MASS_CACHE_SLOTS + MASS_TOTAL_SLOTS) * 4;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds_bytes, (hipStream_t)stream, (u32)n_reads, (u64)n_members, keep_at_most, B, n_samples,
                           (const unsigned char *)d_res->n_rows, (const unsigned short *)d_res->branch, (const double *)d_res->lwr, d_member_read, d_member_sample,
                           d_member_weight, (u64 *)d_masses);
    };
    if (lds) launch(masses_samples_kernel<true>);
    else launch(masses_samples_kernel<false>);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

// Threads take ranges of entries and sum into words of their own while T buffers stay small; beyond that they take ranges of SAMPLES,
// every thread walks the whole list and adds its samples' entries straight into the caller's words (no partial buffers).
extern "C" int rk_masses_accumulate_samples_host(uint32_t n_branches, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, uint32_t n_samples,
                                                 uint64_t n_members, const uint32_t *member_read, const uint32_t *member_sample,
                                                 const uint32_t *member_weight, uint64_t *masses, uint32_t n_threads) {
    const char *who = "rk_masses_accumulate_samples_host";
    if (n_branches < 1 || n_branches > 65535) return fail(RK_ERR_INVALID, "%s: n_branches=%u must be in 1..65535", who, n_branches);
    int rc = masses_samples_args(who, n_branches, keep_at_most, n_reads, res, n_samples, n_members, member_read, member_sample, masses);
    if (rc || n_members == 0) return rc;
    const uint32_t B = n_branches, K = keep_at_most, S = n_samples;
    const uint64_t words = rk_masses_samples_words(B, S);
    unsigned hw = std::thread::hardware_concurrency();
    uint64_t T = n_threads ? n_threads : std::min(hw ? hw : 1u, 16u);
    T = std::max<uint64_t>(1, std::min<uint64_t>({T, 16, (n_members + 4095) / 4096}));
    const bool by_sample = T * words > (1ull << 21);  // partial buffers of 16 MB at the most
    if (by_sample) T = std::min<uint64_t>(T, S);
    return masses_fan_out(who, T, words, T > 1 && !by_sample, masses, [&](uint64_t t, uint64_t *m) {
        const uint64_t lo = by_sample ? 0 : n_members * t / T, hi = by_sample ? n_members : n_members * (t + 1) / T;
        const uint32_t s_lo = by_sample ? (uint32_t)(S * t / T) : 0, s_hi = by_sample ? (uint32_t)(S * (t + 1) / T) : S;
        rk::masses_samples_range(B, K, S, n_reads, res->n_rows, res->branch, res->lwr, lo, hi, member_read, member_sample, member_weight, s_lo, s_hi,
                                 !by_sample || t == 0, m);
    });
}
