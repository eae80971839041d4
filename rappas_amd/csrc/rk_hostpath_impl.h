// rk_hostpath_impl.h -- #included by rk_engine.hip: the host-buffer entry points (rk_place_batch*, rk_reserve_host_path) and the chunk
// pipeline behind them.  A batch is cut into chunks (rk_chunks.h); each chunk is staged, uploaded, placed, downloaded and drained
// through one of the handle's four workspaces (rk_hostbuf_impl.h), whose buffers are kept (grow-only) in the rk_db between calls.
// The entry points differ in the placement step of a chunk and nothing else (HostStep).
#pragma once

#include "rk_chunks.h"

namespace {
// A few worker threads that live for the duration of ONE host call: run(fn) executes fn(part, parts) on every worker and on the
// caller and returns when all are done (a chunk of 2^18 reads is packed in under a millisecond -- starting threads per chunk would
// cost as much as the work).  Joined in the destructor, so no path out of the call leaves a thread behind.
class ForkJoin {
  public:
    explicit ForkJoin(unsigned workers, const NodeCpus *node = nullptr) {  // node: the workers run on the CPUs next to the GPU
        for (unsigned i = 0; i < workers; i++) th_.emplace_back([this, i, node]() { pin_this_thread(node); loop(i + 1); });
    }
    ~ForkJoin() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; gen_.fetch_add(1); }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    unsigned parts() const { return (unsigned)th_.size() + 1; }
    void run(const std::function<void(unsigned, unsigned)> &fn) {  // the workers and the caller, each one part; returns when all are done
        if (th_.empty()) { fn(0, 1); return; }
        post(&fn, 0, parts());
        fn(0, parts());
        wait();
    }
    // the workers alone, while the caller does something else; wait() before the next start() / run().  Without workers the
    // function runs in start().
    void start(std::function<void(unsigned, unsigned)> fn) {
        if (th_.empty()) { fn(0, 1); return; }
        own_ = std::move(fn);
        post(&own_, 1, (unsigned)th_.size());
    }
    void wait() {
        for (int spin = 0; spin < 4000 && left_.load(std::memory_order_acquire) != 0; spin++) cpu_relax();
        if (left_.load(std::memory_order_acquire) == 0) return;
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&]() { return left_.load() == 0; });
    }

  private:
    static void cpu_relax() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    void post(const std::function<void(unsigned, unsigned)> *fn, unsigned base, unsigned parts) {
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = fn; base_ = base; parts_ = parts;
            left_.store((unsigned)th_.size(), std::memory_order_release);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
    }
    // A chunk of the host path is staged in well under a millisecond, so a worker that has just finished one job spins for a few
    // tens of microseconds before it blocks: the next job usually arrives within that time and a futex wake-up costs as much.
    void loop(unsigned me) {
        uint64_t seen = 0;
        while (true) {
            for (int spin = 0; spin < 3000 && gen_.load(std::memory_order_acquire) == seen; spin++) cpu_relax();  // (~30 us; a hosting JVM has pools of its own to feed)
            const std::function<void(unsigned, unsigned)> *fn;
            unsigned part, parts;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return gen_.load() != seen; });
                seen = gen_.load();
                if (stop_) return;
                fn = fn_;
                part = me - base_;
                parts = parts_;
            }
            (*fn)(part, parts);
            if (left_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(m_);
                done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned, unsigned)> *fn_ = nullptr;
    std::function<void(unsigned, unsigned)> own_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<unsigned> left_{0};
    unsigned base_ = 0, parts_ = 1;
    bool stop_ = false;
};

// rk_place_batch_multi runs one host call per GPU at the same time: each takes its share of the thread budget
thread_local unsigned tl_concurrent_calls = 1;
unsigned host_threads(uint64_t n_reads, unsigned asked) {
    unsigned hw = std::thread::hardware_concurrency();
    unsigned T = asked ? asked : std::max(2u, std::min(hw ? hw : 1u, 16u * tl_concurrent_calls) / tl_concurrent_calls);
    if (!asked && T > 16u) T = 16u;
    return n_reads < 4096 ? 1u : T;
}
}  // namespace

#define RK_TRY(expr) do { int rc_ = (expr); if (rc_ != RK_OK) return rc_; } while (0)

static int hip_rc(hipError_t e, const char *what) { return e == hipSuccess ? RK_OK : fail(RK_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); }
static int h2d(void *dst, const void *src, size_t bytes, hipStream_t s) {
    return hip_rc(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync (host to device)");
}

// what the host hands over: ASCII reads (packed on the device) or records already packed on the host (rk_pack_reads_host)
struct HostInput {
    const uint8_t *ascii = nullptr;   // concatenated reads; with `packed` set: only consulted for reads flagged AMBIGUOUS
    const uint64_t *off = nullptr;    // [n + 1]
    const uint32_t *packed = nullptr; // [n][wpr]
    uint32_t wpr = 0;
    const uint32_t *lens = nullptr;   // [n] or NULL (fixed_len)
    uint32_t fixed_len = 0;
    const uint32_t *flags = nullptr;  // [n] or NULL
};

// The placement step of a chunk -- all that differs between the host entry points, with the packer spec that follows from it:
//   FORWARD     rk_place_packed_device
//   STRANDS     rk_place_packed_device_strands on `strand`, its workspace in w.strands
//   TRANSLATED  rk_place_packed_device_translated, its workspace in w.translated, the frame bytes travelling with the result set.
//               The characters are DNA on an amino-acid handle, which has no DNA table on the device: they are always packed on
//               the host (DNA spec, k = 1), whatever memory they live in, and never cross the link.
struct HostStep {
    enum Kind { FORWARD, STRANDS, TRANSLATED } kind = FORWARD;
    uint32_t strand = RK_STRAND_FORWARD;
    uint8_t *frame_out = nullptr;
};

// Where a chunk's results go -- orthogonal to HostStep::kind.  Without `masses` the whole result set is downloaded into the caller's
// arrays.  With it (rk_place_batch*_masses) the chunk is summed where it lies: rk_masses_accumulate_device on the chunk's stream, its
// device result set, its weights and the handle's device mass buffer; only the flags come back (the counters are taken from them),
// and `out` holds the caller's flags_out and nothing else.
struct HostSink {
    uint64_t *masses = nullptr;         // the caller's buffer: the device buffer's words are ADDED into it after the last chunk
    const uint32_t *weights = nullptr;  // [n] or NULL
    // The membership form (rk_place_batch*_masses_samples; n_samples != 0, weights unused): `masses` is a sample mass buffer, a chunk
    // [lo, hi) stages the entries member_off[lo] .. member_off[hi] as (read - lo, sample, weight) and hands them to
    // rk_masses_accumulate_samples_device.  member_off NULL: one entry per read, entry r is read r.
    uint32_t n_samples = 0;
    const uint64_t *member_off = nullptr;     // [n + 1] or NULL
    const uint32_t *member_sample = nullptr;  // [entries]
    const uint32_t *member_weight = nullptr;  // [entries] or NULL
};

// the chunk's read limit: the one place that reads the developer knob
static uint64_t chunk_max_reads() {
    if (const char *e = rk_knob("RK_CHUNK_READS")) {
        const long v = atol(e);
        if (v >= (long)rk::CHUNK_MIN_READS_KNOB) return (uint64_t)v;
    }
    return rk::CHUNK_MAX_READS;
}

// bytes of a chunk's page-locked staging block: the records, then the lengths and the flags that go with them
static size_t staged_bytes(uint64_t n, uint32_t wpr, bool lens, bool flags) { return (size_t)n * wpr * 4 + (lens ? n * 4 : 0) + (flags ? n * 4 : 0); }

// what enqueue() needs of a workspace for a chunk of n reads: records, lengths, flags and the result set on the device, and -- for
// pageable result arrays -- the result set's staging.  rk_reserve_host_path asks for a full chunk through it.
static int reserve_chunk(rk_workspace &w, uint64_t n, uint32_t wpr, uint32_t K, bool frames, bool stage_results, const NodeCpus *node, int device) {
    RK_TRY(w.packed.reserve((size_t)n * wpr * 4));
    RK_TRY(w.lens.reserve(n * 4));
    RK_TRY(w.flags.reserve(n * 4));
    RK_TRY(w.res.reserve(n, K, frames));
    return stage_results ? w.h_res.reserve(n, K, frames, node, device) : RK_OK;
}

// The first argument tests of a host entry point, `who`-parameterised like check_fixed_len; reads_missing: what to say when the reads
// are not there ("null reads"), or null.  check_host_batch makes the rest once the call is known to have reads; plan_chunk has the
// 2^28 symbol limit.
static int check_host_call(const char *who, const rk_db *db, const rk_params *p, const rk_result *out, const char *reads_missing) {
    if (!db || !out) return fail(RK_ERR_INVALID, "%s: null argument", who);
    RK_TRY(check_params(p));
    return reads_missing ? fail(RK_ERR_INVALID, "%s: %s", who, reads_missing) : RK_OK;
}
static int check_host_batch(const char *who, uint64_t n_reads, const HostInput &in, const rk_result *out, const HostStep &step, bool masses_sink) {
    if (!masses_sink && (!result_complete(out) || (step.kind == HostStep::TRANSLATED && !step.frame_out))) return fail(RK_ERR_INVALID, "%s: null result array", who);
    if (in.off)  // (a compare and nothing else: 0.4 ms for 4 000 000 reads; the 2^28 symbol limit is tested chunk by chunk, where next_chunk has the lengths)
        for (uint64_t r = 0; r < n_reads; r++)
            if (in.off[r + 1] < in.off[r]) return fail(RK_ERR_INVALID, "%s: seq_off not monotone at read %llu", who, (unsigned long long)r);
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// One host call.  Four workspaces in flight.  The call's worker threads stage chunk c + 1 (pack its characters / copy
// its records into page-locked memory) while this thread enqueues chunk c, and a second host thread waits for the stream of the
// oldest chunk and moves its results into the caller's arrays: staging, enqueueing, the GPU's work and the result copies of different
// chunks overlap (one host thread doing everything by turns kept the GPU waiting: 1.6e8 reads/s on C2).
// The caller holds db->host_mutex and has made the device current and the workspaces' streams.
// ------------------------------------------------------------------------------------------------
class HostPath {
    static constexpr unsigned NWS = 4;
    // A chunk's host side (plan + stage) runs one chunk ahead of its device side (enqueue).
    struct Plan {
        uint64_t r0 = 0, r1 = 0, n = 0;
        uint32_t wpr = 0;
        unsigned wi = 0;
        size_t pb = 0;
        bool staged_async = false;
        std::atomic<uint32_t> flags{0};  // OR of the flags the host packer set
        bool need_ascii = false;         // (enqueue) the chunk's characters travel: nbytes of them
        uint64_t nbytes = 0;
    };
    bool translated() const { return step_.kind == HostStep::TRANSLATED; }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    static bool is_pinned(const void *ptr) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeHost;
    }

  public:
    HostPath(rk_db *db, const rk_params *p, uint64_t n_reads, const HostInput &in, rk_result *out, const HostStep &step, const char *who,
             const HostSink &sink = HostSink{})
        : db_(db), p_(p), n_reads_(n_reads), in_(in), out_(out), step_(step), sink_(sink), who_(who), K_(p->keep_at_most), device_(db->info.device),
          node_(&gpu_node_cpus(db->info.device)), max_reads_(chunk_max_reads()), timing_(rk_knob("RK_HOST_TIMING") != nullptr) {
        // Caller buffers from rk_host_alloc (or otherwise page-locked) are the DMA's source / target directly; pageable ones
        // (the usual case behind JNI) go through page-locked staging with threaded copies
        packed_in_ = in.packed != nullptr;
        in_pinned_ = packed_in_ ? is_pinned(in.packed) : is_pinned(in.ascii);
        if (sink_.masses)  // only the flags come back: into the caller's flags_out if it is page-locked, else into the staging flags
            out_pinned_ = out->flags && is_pinned(out->flags);
        else
            out_pinned_ = is_pinned(out->n_rows) && is_pinned(out->branch) && is_pinned(out->score) && is_pinned(out->lwr) && is_pinned(out->flags) &&
                          (!translated() || is_pinned(step.frame_out));
        weights_pinned_ = sink_.weights && is_pinned(sink_.weights);
        // pageable characters are packed on the host (rk_pack_host.cpp) by this call's worker threads; page-locked ones go to the
        // device as they are (no host work at all) and are packed there
        host_pack_ = translated() || (!packed_in_ && !in_pinned_);
        if (translated()) build_alphabet(RK_ALPHABET_DNA, false, alpha_), spec_ = pack_spec(alpha_, RK_ALPHABET_DNA, 2, 1, 0);
        else if (host_pack_) build_alphabet(db->info.alphabet, db->shape.convert_uo != 0, alpha_), spec_ = pack_spec(alpha_, db->info.alphabet, db->info.bits_per_symbol, db->info.k, 0);
        // host threads of this call: staging / packing on one side, result copies on the other (both only for pageable memory)
        const bool stages = host_pack_ || !in_pinned_ || stage_weights();
        n_stage_ = stages ? std::max(1u, host_threads(n_reads, 0) * 5 / 8) : 0u;
        n_drain_ = out_pinned_ ? 0u : std::max(1u, host_threads(n_reads, 0) * 3 / 8);
        if (const char *e = rk_knob("RK_STAGE_THREADS")) n_stage_ = (unsigned)std::max(1, atoi(e));  // developer knobs
        if (const char *e = rk_knob("RK_DRAIN_THREADS")) n_drain_ = (unsigned)std::max(1, atoi(e));
        pool_.emplace(n_stage_ ? n_stage_ - 1 : 0, node_);
    }

    // On every way out, a thrown exception included (a joinable std::thread that is destroyed calls std::terminate, which would take
    // the hosting JVM down): the workers have let go of the caller's arrays, the drainer is joined, no stream holds work.
    ~HostPath() { finish(true); }

    int run(rk_counters *counters) {
        if (sink_.masses) RK_TRY(masses_begin());
        drainer_ = std::thread([this]() { drainer_loop(); });
        int status = plan_chunk(plans_[0], 0, 0);
        if (status == RK_OK) status = stage_start(plans_[0]);
        for (unsigned cur = 0; status == RK_OK; cur ^= 1) {
            status = enqueue(plans_[cur], plans_[cur ^ 1]);
            if (plans_[cur].r1 >= n_reads_) break;
        }
        finish(status != RK_OK);
        if (timing_) {
            fprintf(stderr, "%s: GPU %d on NUMA node %d, %d of this process's CPUs there, staging threads %s; %u staging + %u drain threads\n", who_, device_,
                    node_->node, node_->ok ? CPU_COUNT(&node_->set) : 0, node_->ok ? "kept there" : "not pinned", n_stage_, n_drain_);
            fprintf(stderr, "%s: %u chunks; submit thread: stage input %.1f ms, stage+enqueue %.1f ms; drain thread: wait for stream %.1f ms, move results %.1f ms\n",
                    who_, chunk_no_, t_stage_ * 1e3, t_enq_ * 1e3, t_wait_ * 1e3, t_drain_ * 1e3);
        }
        if (status == RK_OK && drain_status_ != RK_OK) status = fail(drain_status_, "%s", drain_msg_.c_str());
        if (status == RK_OK && sink_.masses) status = masses_end();
        if (status == RK_OK && counters) *counters = ct_;
        return status;
    }

  private:
    // The masses sink's device buffer, one per handle: zeroed here, and the zeroing waited for, so that it lies before every chunk's
    // accumulate on all four streams (which then add into it side by side: integer atomics).
    size_t masses_bytes() const {
        return (size_t)(sink_.n_samples ? rk_masses_samples_words(db_->info.n_branches, sink_.n_samples) : rk_masses_words(db_->info.n_branches)) * 8;
    }
    // The chunk's membership entries: sample | read - lo | weight, three arrays of m words in one page-locked block (filled here, on
    // the submit thread: 12 bytes an entry), one copy to the device, then the per-sample sums on the chunk's stream.
    int masses_samples(const Plan &c, rk_workspace &w, const rk_result &dres) {
        const uint64_t e0 = sink_.member_off ? sink_.member_off[c.r0] : c.r0, e1 = sink_.member_off ? sink_.member_off[c.r1] : c.r1, m = e1 - e0;
        if (m == 0) return RK_OK;
        if (m >= (1ull << 32)) return fail(RK_ERR_INVALID, "%s: %llu membership entries in one chunk of reads, at most 2^32 - 1", who_, (unsigned long long)m);
        const bool reads = sink_.member_off != nullptr, wts = sink_.member_weight != nullptr;
        const size_t bytes = (size_t)m * 4 * (1 + (reads ? 1 : 0) + (wts ? 1 : 0));
        RK_TRY(w.h_members.reserve(bytes, node_, device_));
        RK_TRY(w.members.reserve(bytes));
        uint32_t *hs = w.h_members.as<uint32_t>(), *hr = hs + m, *hw = hr + (reads ? m : 0);
        memcpy(hs, sink_.member_sample + e0, m * 4);
        if (wts) memcpy(hw, sink_.member_weight + e0, m * 4);
        if (reads)
            for (uint64_t r = c.r0; r < c.r1; r++)
                for (uint64_t e = sink_.member_off[r]; e < sink_.member_off[r + 1]; e++) hr[e - e0] = (uint32_t)(r - c.r0);
        RK_TRY(h2d(w.members.p, hs, bytes, w.stream));
        const uint32_t *ds = w.members.as<uint32_t>(), *dr = ds + m, *dw = dr + (reads ? m : 0);
        return rk_masses_accumulate_samples_device(db_, K_, c.n, &dres, sink_.n_samples, m, reads ? dr : nullptr, ds, wts ? dw : nullptr,
                                                   db_->d_masses.as<uint64_t>(), w.stream);
    }
    int masses_begin() {
        hipStream_t s = db_->ws[0].stream;
        RK_TRY(db_->d_masses.reserve(masses_bytes()));
        RK_TRY(db_->h_masses.reserve(masses_bytes(), node_, device_));
        db_->masses_samples = sink_.n_samples;  // (rk_kr_distances_batch reads the buffer where it lies)
        RK_TRY(hip_rc(hipMemsetAsync(db_->d_masses.p, 0, masses_bytes(), s), "hipMemsetAsync"));
        return hip_rc(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    // every chunk is drained (finish): one copy brings the words to the host, where they are ADDED into the caller's buffer -- the
    // only place that writes it, reached on success alone
    int masses_end() {
        hipStream_t s = db_->ws[0].stream;
        RK_TRY(hip_rc(hipMemcpyAsync(db_->h_masses.p, db_->d_masses.p, masses_bytes(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync (device to host)"));
        RK_TRY(hip_rc(hipStreamSynchronize(s), "hipStreamSynchronize"));
        const uint64_t *src = db_->h_masses.as<uint64_t>();
        for (size_t i = 0, n = masses_bytes() / 8; i < n; i++) sink_.masses[i] += src[i];
        return RK_OK;
    }

    // bytes of the chunk's staging block ahead of its weights (pageable weights lie behind the records, lengths and flags)
    size_t staged_base(const Plan &c) const {
        if (host_pack_) return staged_bytes(c.n, c.wpr, true, true);
        if (packed_in_ && !in_pinned_) return staged_bytes(c.n, c.wpr, in_.lens != nullptr, in_.flags != nullptr);
        return 0;
    }
    bool stage_weights() const { return sink_.weights && !weights_pinned_; }

    // bounds, record width, workspace (waits until it is free)
    int plan_chunk(Plan &c, uint64_t from, unsigned no) {
        const rk::Chunk ch = rk::next_chunk(packed_in_ ? nullptr : in_.off, from, n_reads_, max_reads_, rk::CHUNK_MAX_BYTES);
        if (ch.max_len > 0x7FFFFFFFull / 8) return fail(RK_ERR_UNSUPPORTED, "%s: read longer than 2^28 symbols", who_);
        c.r0 = from; c.r1 = ch.r1; c.n = ch.r1 - from;
        c.wpr = packed_in_ ? in_.wpr : translated() ? (uint32_t)std::max<uint64_t>(1, (ch.max_len * 2 + 31) / 32) : rk_packed_words(db_, (uint32_t)ch.max_len);
        c.wi = no % NWS;
        c.pb = c.n * c.wpr * 4;
        c.staged_async = false;
        c.flags.store(0);
        // the workspace was last used four chunks ago: its results must have left the staging buffers before it is overwritten
        std::unique_lock<std::mutex> lk(qm_);
        qcv_.wait(lk, [&]() { return !ws_busy_[c.wi]; });
        if (drain_status_ != RK_OK) return fail(drain_status_, "%s", drain_msg_.c_str());
        return RK_OK;
    }

    // host work of a chunk that needs no HIP call: started on the worker threads, joined with pool_->wait()
    int stage_start(Plan &c) {
        rk_workspace &w = db_->ws[c.wi];
        const uint64_t n = c.n, c0 = c.r0;
        if (host_pack_) {
            // pageable characters (the usual case behind JNI): packed HERE, by the call's worker threads, straight into the
            // page-locked staging buffer -- 48 instead of 158 bytes per 150-bp read cross the link, no copy of the characters
            RK_TRY(w.h_packed.reserve(staged_base(c) + (stage_weights() ? n * 4 : 0), node_, device_));
            uint32_t *hp = w.h_packed.as<uint32_t>(), *hl = hp + n * c.wpr, *hf = hl + n;
            rk::PackSpec P = spec_;
            P.words_per_read = c.wpr;
            const uint8_t *seq_ascii = in_.ascii;
            const uint64_t *seq_off = in_.off;
            Plan *pc = &c;
            const uint32_t *wsrc = stage_weights() ? sink_.weights + c0 : nullptr;  // pageable weights: behind the flags, a range a worker
            uint32_t *wdst = hf + n;
            pool_->start([=](unsigned part, unsigned parts) {
                const uint64_t lo = n * part / parts, hi = n * (part + 1) / parts;
                pc->flags.fetch_or(rk::pack_reads_range(P, seq_ascii, seq_off, c0 + lo, c0 + hi, c0, hp, hl, hf));
                if (wsrc && hi > lo) memcpy(wdst + lo, wsrc + lo, (hi - lo) * 4);
            });
            c.staged_async = true;
        } else if (packed_in_ && !in_pinned_) {
            const size_t pb = c.pb;
            RK_TRY(w.h_packed.reserve(staged_base(c) + (stage_weights() ? n * 4 : 0), node_, device_));
            const char *src = (const char *)(in_.packed + c0 * c.wpr);
            char *dst = (char *)w.h_packed.p;
            const char *wsrc = stage_weights() ? (const char *)(sink_.weights + c0) : nullptr;
            char *wdst = dst + staged_base(c);
            const size_t wb = n * 4;
            pool_->start([=](unsigned part, unsigned parts) {
                const size_t a = pb * part / parts, b = pb * (part + 1) / parts;
                if (b > a) memcpy(dst + a, src + a, b - a);
                const size_t wa = wb * part / parts, we = wb * (part + 1) / parts;
                if (wsrc && we > wa) memcpy(wdst + wa, wsrc + wa, we - wa);
            });
            c.staged_async = true;
        } else if (stage_weights()) {  // page-locked reads, pageable weights: the block holds the weights alone
            RK_TRY(w.h_packed.reserve(n * 4, node_, device_));
            const char *wsrc = (const char *)(sink_.weights + c0);
            char *wdst = (char *)w.h_packed.p;
            const size_t wb = n * 4;
            pool_->start([=](unsigned part, unsigned parts) {
                const size_t wa = wb * part / parts, we = wb * (part + 1) / parts;
                if (we > wa) memcpy(wdst + wa, wsrc + wa, we - wa);
            });
            c.staged_async = true;
        }
        return RK_OK;
    }

    // the device side of a staged chunk: upload, the placement step, download -- and the host side of the next chunk started on the way
    int enqueue(Plan &c, Plan &next) {
        rk_workspace &w = db_->ws[c.wi];
        double t2 = now();
        if (c.staged_async) pool_->wait();
        t_stage_ += now() - t2;
        // packed input: the ASCII of the chunk travels only if one of its reads carries the AMBIGUOUS flag (the ambiguity kernel
        // works on characters); otherwise 38 instead of 150 bytes per 150-bp read cross the link
        const bool chars_direct = !packed_in_ && !host_pack_;  // page-locked characters: the DMA's source as they are
        c.need_ascii = chars_direct;
        if (host_pack_) c.need_ascii = !translated() && (c.flags.load() & RK_FLAG_AMBIGUOUS) != 0;
        if (packed_in_ && in_.flags && in_.ascii && in_.off)
            for (uint64_t r = c.r0; r < c.r1 && !c.need_ascii; r++) c.need_ascii = (in_.flags[r] & RK_FLAG_AMBIGUOUS) != 0;
        c.nbytes = c.need_ascii ? in_.off[c.r1] - in_.off[c.r0] : 0;
        if (c.nbytes && !chars_direct) {  // (rare: a chunk with ambiguity codes) its characters, staged by every thread
            RK_TRY(w.h_ascii.reserve(c.nbytes, node_, device_));
            const uint8_t *src = in_.ascii + in_.off[c.r0];
            uint8_t *dst = w.h_ascii.as<uint8_t>();
            pool_->run([&](unsigned part, unsigned parts) {
                const uint64_t a = c.nbytes * part / parts, b = c.nbytes * (part + 1) / parts;
                if (b > a) memcpy(dst + a, src + a, b - a);
            });
        }
        // the next chunk's host side starts now and runs while this chunk is enqueued
        if (c.r1 < n_reads_) {
            RK_TRY(plan_chunk(next, c.r1, chunk_no_ + 1));
            RK_TRY(stage_start(next));
        }
        t2 = now();
        RK_TRY(reserve_chunk(w, c.n, c.wpr, K_, translated(), !out_pinned_ && !sink_.masses, node_, device_));
        if (sink_.masses) {  // of the page-locked staging set only the flags; the chunk's weights on the device
            if (!out_pinned_) RK_TRY(w.h_res.flags.reserve(c.n * 4, node_, device_));
            if (sink_.weights) RK_TRY(w.weights.reserve(c.n * 4));
        }
        RK_TRY(upload(c, w));
        RK_TRY(place(c, w));
        if (sink_.masses) {
            // summed where it lies; the flags alone come back (a result set whose other arrays are null: download skips them)
            const rk_result dres = w.res.view();
            if (sink_.n_samples) RK_TRY(masses_samples(c, w, dres));
            else RK_TRY(rk_masses_accumulate_device(db_, K_, c.n, &dres, sink_.weights ? w.weights.as<uint32_t>() : nullptr, db_->d_masses.as<uint64_t>(), w.stream));
            const rk_result staged{nullptr, nullptr, nullptr, nullptr, w.h_res.flags.as<uint32_t>()};
            RK_TRY(hip_rc(out_pinned_ ? w.res.download(w.stream, *out_, nullptr, c.r0, c.n, K_) : w.res.download(w.stream, staged, nullptr, 0, c.n, K_),
                          "hipMemcpyAsync (device to host)"));
        } else {
            // the result set: into page-locked caller arrays as they are, else into the staging set the drainer copies from
            RK_TRY(hip_rc(out_pinned_ ? w.res.download(w.stream, *out_, step_.frame_out, c.r0, c.n, K_)
                                      : w.res.download(w.stream, w.h_res.view(), translated() ? w.h_res.frame() : nullptr, 0, c.n, K_),
                          "hipMemcpyAsync (device to host)"));
        }
        w.pending = true; w.pend_r0 = c.r0; w.pend_n = c.n;  // (page-locked caller arrays: nothing to copy, the flags are still counted)
        { std::lock_guard<std::mutex> lk(qm_); ws_busy_[c.wi] = true; submitted_.push_back(c.wi); }
        qcv_.notify_all();
        t_enq_ += now() - t2;
        chunk_no_++;
        return RK_OK;
    }

    int upload(const Plan &c, rk_workspace &w) {
        hipStream_t s = w.stream;
        const uint64_t n = c.n, r0 = c.r0;
        const size_t pb = c.pb;
        if (c.need_ascii) {
            RK_TRY(w.ascii.reserve(c.nbytes));
            RK_TRY(w.off.reserve((n + 1) * 8));
            RK_TRY(w.h_off.reserve((n + 1) * 8, node_, device_));
            uint64_t *ho = w.h_off.as<uint64_t>();
            for (uint64_t i = 0; i <= n; i++) ho[i] = in_.off[r0 + i] - in_.off[r0];
            if (c.nbytes) RK_TRY(h2d(w.ascii.p, !packed_in_ && !host_pack_ ? (const void *)(in_.ascii + in_.off[r0]) : w.h_ascii.p, c.nbytes, s));
            RK_TRY(h2d(w.off.p, w.h_off.p, (n + 1) * 8, s));
        }
        char *staged = (char *)w.h_packed.p;
        if (sink_.weights) {  // 4 bytes a read: from page-locked caller memory as they are, else from the staging block (stage_start)
            RK_TRY(h2d(w.weights.p, weights_pinned_ ? (const void *)(sink_.weights + r0) : staged + staged_base(c), n * 4, s));
        }
        if (host_pack_) {
            RK_TRY(h2d(w.packed.p, staged, pb, s));
            RK_TRY(h2d(w.lens.p, staged + pb, n * 4, s));
            RK_TRY(h2d(w.flags.p, staged + pb + n * 4, n * 4, s));
        } else if (packed_in_) {
            // packed records (+ lengths, flags): straight from page-locked caller memory, else through the staging block.  (Lengths
            // and flags are small, but they must not be read after this call returns: the block keeps them when the memory is pageable.)
            const size_t lb = in_.lens ? n * 4 : 0, fb = in_.flags ? n * 4 : 0;
            if (!in_pinned_) {
                if (lb) memcpy(staged + pb, in_.lens + r0, lb);
                if (fb) memcpy(staged + pb + lb, in_.flags + r0, fb);
            }
            RK_TRY(h2d(w.packed.p, in_pinned_ ? (const void *)(in_.packed + r0 * c.wpr) : staged, pb, s));
            if (lb) RK_TRY(h2d(w.lens.p, in_pinned_ ? (const void *)(in_.lens + r0) : staged + pb, lb, s));
            if (fb) RK_TRY(h2d(w.flags.p, in_pinned_ ? (const void *)(in_.flags + r0) : staged + pb + lb, fb, s));
        } else {
            RK_TRY(rk_pack_reads_device(db_, n, w.ascii.as<uint8_t>(), w.off.as<uint64_t>(), c.wpr, w.packed.as<uint32_t>(), w.lens.as<uint32_t>(),
                                        w.flags.as<uint32_t>(), s));
        }
        return RK_OK;
    }

    // the placement step
    int place(const Plan &c, rk_workspace &w) {
        const rk_result dres = w.res.view();
        const uint32_t *packed = w.packed.as<uint32_t>();
        const uint32_t *d_lens = (!packed_in_ || in_.lens) ? w.lens.as<uint32_t>() : nullptr;  // (host-packed chunks carry both)
        const uint32_t *d_flags = (!packed_in_ || in_.flags) ? w.flags.as<uint32_t>() : nullptr;
        const uint32_t fixed_len = packed_in_ ? in_.fixed_len : 0;
        const uint8_t *d_ascii = c.need_ascii ? w.ascii.as<uint8_t>() : nullptr;
        const uint64_t *d_off = c.need_ascii ? w.off.as<uint64_t>() : nullptr;
        switch (step_.kind) {
        case HostStep::FORWARD:
            return rk_place_packed_device(db_, p_, c.n, packed, c.wpr, d_lens, fixed_len, d_flags, d_ascii, d_off, &dres, w.stream);
        case HostStep::STRANDS: {
            // the other strand's records, its result set and -- a chunk whose characters travel -- their reverse complement: part
            // of the workspace (a chunk of empty reads has characters of length 0: one byte of room keeps the call's test quiet)
            const uint64_t wb = rk_strands_work_bytes(db_, c.n, c.wpr, K_, c.need_ascii ? std::max<uint64_t>(c.nbytes, 1) : 0);
            RK_TRY(w.strands.reserve(wb));
            return rk_place_packed_device_strands(db_, p_, step_.strand, c.n, packed, c.wpr, d_lens, fixed_len, d_flags, d_ascii, d_off, &dres, w.strands.p, wb,
                                                  w.stream);
        }
        case HostStep::TRANSLATED: {
            const uint64_t wb = rk_translated_work_bytes(db_, c.n, c.wpr, K_);
            if (!wb) return RK_ERR_INVALID;
            RK_TRY(w.translated.reserve(wb));
            return rk_place_packed_device_translated(db_, p_, c.n, packed, c.wpr, d_lens, 0, d_flags, &dres, w.res.frame(), w.translated.p, wb, w.stream);
        }
        }
        return fail(RK_ERR_INVALID, "%s: unknown placement step", who_);
    }

    // staged results of the workspace's last chunk -> the caller's arrays; the counters, chunk by chunk
    void drain(rk_workspace &w, ForkJoin &dpool) {
        if (!w.pending) return;
        const uint64_t a0 = w.pend_r0, m = w.pend_n;
        if (sink_.masses) {  // the flags: counted where they arrived, copied to flags_out when one is given
            if (!out_pinned_ && out_->flags) memcpy(out_->flags + a0, w.h_res.flags.p, m * 4);
            rk::count_flags(out_pinned_ ? out_->flags + a0 : w.h_res.flags.as<uint32_t>(), m, ct_);
            w.pending = false;
            return;
        }
        if (!out_pinned_) {
            // the drain thread's workers, each a range of reads over the arrays (103 bytes per read at K = 7)
            dpool.run([&](unsigned part, unsigned parts) {
                const uint64_t lo = m * part / parts, c = m * (part + 1) / parts - lo;
                if (c) w.h_res.copy_range(*out_, step_.frame_out, a0, lo, c, K_);
            });
        }
        rk::count_flags(out_->flags + a0, m, ct_);
        w.pending = false;
    }

    // the second host thread: waits for the stream of the oldest submitted chunk, drains it, frees its workspace
    void drainer_loop() {
        pin_this_thread(node_);
        (void)hipSetDevice(device_);
        std::unique_ptr<ForkJoin> dpool;
        try {
            dpool.reset(new ForkJoin(n_drain_ ? n_drain_ - 1 : 0, node_));
        } catch (...) {  // no worker threads: this thread copies alone
        }
        ForkJoin none(0);
        auto failed = [&](rk_workspace &w, int code, const std::string &msg) {  // the first error is the one reported
            std::lock_guard<std::mutex> lk(qm_);
            if (drain_status_ == RK_OK) { drain_status_ = code; drain_msg_ = msg; }
            w.pending = false;
        };
        while (true) {
            unsigned wi;
            {
                std::unique_lock<std::mutex> lk(qm_);
                qcv_.wait(lk, [&]() { return !submitted_.empty() || closing_; });
                if (submitted_.empty()) return;
                wi = submitted_.front();
                submitted_.pop_front();
            }
            rk_workspace &w = db_->ws[wi];
            const double t0 = now();
            const hipError_t he = hipStreamSynchronize(w.stream);
            const double t1 = now();
            bool ok;
            { std::lock_guard<std::mutex> lk(qm_); ok = drain_status_ == RK_OK; }
            if (he != hipSuccess) {
                failed(w, RK_ERR_HIP, std::string("hipStreamSynchronize failed: ") + hipGetErrorString(he));
            } else if (ok) {
                try {
                    drain(w, dpool ? *dpool : none);
                } catch (...) {
                    failed(w, RK_ERR_NOMEM, "out of host memory while moving results");
                }
            } else w.pending = false;
            t_wait_ += t1 - t0; t_drain_ += now() - t1;
            { std::lock_guard<std::mutex> lk(qm_); ws_busy_[wi] = false; }
            qcv_.notify_all();
        }
    }

    // every submitted chunk drained and the drainer joined; the workers first, as an error may leave the next chunk's staging running,
    // which reads the caller's arrays.  failed: some streams may still hold work of a half-enqueued chunk.
    void finish(bool failed) {
        if (finished_) return;
        finished_ = true;
        pool_->wait();
        if (drainer_.joinable()) {
            { std::lock_guard<std::mutex> lk(qm_); closing_ = true; }
            qcv_.notify_all();
            drainer_.join();
        }
        for (rk_workspace &w : db_->ws) {
            if (w.stream && failed) (void)hipStreamSynchronize(w.stream);
            w.pending = false;
        }
    }

    rk_db *const db_;
    const rk_params *const p_;
    const uint64_t n_reads_;
    const HostInput in_;
    rk_result *const out_;
    const HostStep step_;
    const HostSink sink_;
    const char *const who_;
    const uint32_t K_;
    const int device_;
    const NodeCpus *const node_;  // the CPUs next to the GPU: staging threads and page-locked buffers live there
    const uint64_t max_reads_;
    bool packed_in_, in_pinned_, out_pinned_, host_pack_, weights_pinned_;
    Alphabet alpha_;              // host_pack_: the packer's table and its spec (the record width is the chunk's)
    rk::PackSpec spec_{};
    unsigned n_stage_ = 0, n_drain_ = 0;
    std::optional<ForkJoin> pool_;
    Plan plans_[2];
    unsigned chunk_no_ = 0;
    rk_counters ct_{};            // (the drainer's, read after it is joined -- as are t_wait_ and t_drain_)
    // the queue between this thread and the drainer
    std::mutex qm_;
    std::condition_variable qcv_;
    std::deque<unsigned> submitted_;  // workspace indices in submission order
    bool ws_busy_[NWS] = {false, false, false, false};
    bool closing_ = false, finished_ = false;
    int drain_status_ = RK_OK;
    std::string drain_msg_;
    std::thread drainer_;
    // developer knob: RK_HOST_TIMING=1 prints where the host threads of this call spent their time (stderr)
    const bool timing_;
    double t_wait_ = 0, t_drain_ = 0, t_stage_ = 0, t_enq_ = 0;
};

static int place_host(rk_db *db, const rk_params *p, uint64_t n_reads, const HostInput &in, rk_result *out, rk_counters *counters, const char *who,
                      const HostStep &step = HostStep{}, const HostSink &sink = HostSink{}) {
    if (n_reads == 0) { if (counters) *counters = rk_counters{}; return RK_OK; }
    RK_TRY(check_host_batch(who, n_reads, in, out, step, sink.masses != nullptr));
    std::lock_guard<std::mutex> lock(db->host_mutex);  // the workspaces belong to the db: one host call at a time
    HIP_TRY(hipSetDevice(db->info.device));
    for (rk_workspace &w : db->ws)
        if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    HostPath path(db, p, n_reads, in, out, step, who, sink);
    return path.run(counters);
}

// What the first rk_place_batch / rk_place_batch_packed of a handle would set up on its way -- the four workspaces' streams, device
// buffers and page-locked staging buffers for full chunks of reads of up to max_read_len symbols, the launches' scratch -- done ahead
// of time (a caller does this while it is still reading its input: ~80 ms that the first batch then does not pay).
extern "C" int rk_reserve_host_path(rk_db *db, uint32_t keep_at_most, uint32_t max_read_len) {
    if (!db) return fail(RK_ERR_INVALID, "rk_reserve_host_path: null handle");
    if (keep_at_most < 1 || keep_at_most > 16) return fail(RK_ERR_INVALID, "keep_at_most=%u outside 1..16", keep_at_most);
    RK_GUARD_BEGIN
    int prev = 0;
    (void)hipGetDevice(&prev);
    struct Restore { int p; ~Restore() { (void)hipSetDevice(p); } } restore{prev};
    {
        std::lock_guard<std::mutex> lock(db->host_mutex);
        HIP_TRY(hipSetDevice(db->info.device));
        const uint64_t n = rk::CHUNK_MAX_READS;
        const uint32_t wpr = rk_packed_words(db, max_read_len ? max_read_len : 1);
        const NodeCpus *node = &gpu_node_cpus(db->info.device);
        // the masses sink's buffer, device and host side (rk_place_batch*_masses)
        RK_TRY(db->d_masses.reserve((size_t)rk_masses_words(db->info.n_branches) * 8));
        RK_TRY(db->h_masses.reserve((size_t)rk_masses_words(db->info.n_branches) * 8, node, db->info.device));
        for (rk_workspace &w : db->ws) {
            if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
            RK_TRY(reserve_chunk(w, n, wpr, keep_at_most, false, true, node, db->info.device));
            RK_TRY(w.h_packed.reserve(staged_bytes(n, wpr, true, true), node, db->info.device));
            (void)launch_scratch(db, w.stream, 1024 + (size_t)n / 4 + 256 + (size_t)n * 5 + 512);
        }
    }
    // ... and one small batch through the whole path: the runtime loads a kernel's code to the device at its first launch
    // (tens of milliseconds for the packer, the placement kernel and the tile-order pre-pass together)
    const uint64_t m = 32768;  // (the pre-pass starts at this many reads)
    const uint32_t len = std::max<uint32_t>(db->info.k, std::min<uint32_t>(max_read_len ? max_read_len : 1u, 64u));
    std::vector<uint8_t> seq((size_t)m * len, db->info.alphabet == RK_ALPHABET_DNA ? (uint8_t)'A' : (uint8_t)'R');
    std::vector<uint64_t> off(m + 1);
    for (uint64_t i = 0; i <= m; i++) off[i] = i * len;
    std::vector<double> block((work_result(nullptr, 0, m, keep_at_most, nullptr) + 7) / 8);  // the result set, laid out in one block
    rk_result res;
    (void)work_result((char *)block.data(), 0, m, keep_at_most, &res);
    rk_params p{keep_at_most, 0.01f, RK_AMB_MEAN, -INFINITY};
    return rk_place_batch(db, &p, m, seq.data(), off.data(), &res, nullptr);
    RK_GUARD_END("rk_reserve_host_path")
}

extern "C" int rk_place_batch(rk_db *db, const rk_params *p, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off, rk_result *out,
                              rk_counters *counters) {
    const char *who = "rk_place_batch";
    RK_TRY(check_host_call(who, db, p, out, n_reads && (!seq_ascii || !seq_off) ? "null reads" : nullptr));
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off;
    RK_GUARD_BEGIN
    return place_host(db, p, n_reads, in, out, counters, who);
    RK_GUARD_END(who)
}

extern "C" int rk_place_batch_strands(rk_db *db, const rk_params *p, uint32_t strand, uint64_t n_reads, const uint8_t *seq_ascii,
                                      const uint64_t *seq_off, rk_result *out, rk_counters *counters) {
    const char *who = "rk_place_batch_strands";
    RK_TRY(strands_handle(db, who));
    if (strand > RK_STRAND_BOTH) return fail(RK_ERR_INVALID, "%s: strand=%u (0 forward, 1 reverse, 2 both)", who, strand);
    RK_TRY(check_host_call(who, db, p, out, n_reads && (!seq_ascii || !seq_off) ? "null reads" : nullptr));
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off;
    HostStep step;
    if (strand != RK_STRAND_FORWARD) { step.kind = HostStep::STRANDS; step.strand = strand; }
    RK_GUARD_BEGIN
    return place_host(db, p, n_reads, in, out, counters, who, step);
    RK_GUARD_END(who)
}

extern "C" int rk_place_batch_packed(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                                     const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                                     const uint64_t *seq_off, rk_result *out, rk_counters *counters) {
    const char *who = "rk_place_batch_packed";
    RK_TRY(check_host_call(who, db, p, out, n_reads && (!packed || words_per_read == 0) ? "null packed reads" : nullptr));
    RK_TRY(check_fixed_len(who, lens, fixed_len, db->info.bits_per_symbol, words_per_read));
    if ((seq_ascii == nullptr) != (seq_off == nullptr)) return fail(RK_ERR_INVALID, "%s: seq_ascii and seq_off go together", who);
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off; in.packed = packed; in.wpr = words_per_read; in.lens = lens; in.fixed_len = fixed_len; in.flags = flags;
    RK_GUARD_BEGIN
    return place_host(db, p, n_reads, in, out, counters, who);
    RK_GUARD_END(who)
}

// DNA characters from the host onto an amino-acid database: the pipeline with the translated step (HostStep).  Six placement passes a
// chunk are the cost, not the copies around them; staging and draining overlap them all the same.
extern "C" int rk_place_batch_translated(rk_db *db, const rk_params *p, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off,
                                         rk_result *out, uint8_t *frame_out, rk_counters *counters) {
    const char *who = "rk_place_batch_translated";
    RK_TRY(translated_handle(db, who));
    RK_TRY(check_host_call(who, db, p, out, n_reads && (!seq_ascii || !seq_off) ? "null reads" : nullptr));
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off;
    HostStep step;
    step.kind = HostStep::TRANSLATED; step.frame_out = frame_out;
    RK_GUARD_BEGIN
    return place_host(db, p, n_reads, in, out, counters, who, step);
    RK_GUARD_END(who)
}

// Profile-only placement: the pipeline of the entry point that `step` names with the masses sink behind it (HostSink).  The tests of
// the arguments come first and in the header's order; until they have passed nothing is launched and nothing is written.
static HostSink weights_sink(const uint32_t *weights) {
    HostSink s;
    s.weights = weights;
    return s;
}
static HostSink members_sink(uint32_t n_samples, const uint64_t *member_off, const uint32_t *member_sample, const uint32_t *member_weight) {
    HostSink s;
    s.n_samples = n_samples; s.member_off = member_off; s.member_sample = member_sample; s.member_weight = member_weight;
    return s;
}
// the membership arguments of a host call, in one pass up front
static int check_members(const char *who, uint32_t B, uint64_t n_reads, const HostSink &sink) {
    if (!rk_masses_samples_words(B, sink.n_samples))
        return fail(RK_ERR_INVALID, "%s: n_samples=%u on %u branches: 1..65535 samples and at most 2^29 words (n_samples * (2 * n_branches + 4) + 1)", who, sink.n_samples, B);
    if (sink.member_off) {
        if (sink.member_off[0] != 0) return fail(RK_ERR_INVALID, "%s: member_off[0]=%llu must be 0", who, (unsigned long long)sink.member_off[0]);
        for (uint64_t r = 0; r < n_reads; r++)
            if (sink.member_off[r + 1] < sink.member_off[r]) return fail(RK_ERR_INVALID, "%s: member_off not monotone at read %llu", who, (unsigned long long)r);
    }
    const uint64_t entries = sink.member_off ? sink.member_off[n_reads] : n_reads;
    if (entries && !sink.member_sample) return fail(RK_ERR_INVALID, "%s: null member_sample", who);
    return RK_OK;
}

static int place_host_masses(const char *who, rk_db *db, const rk_params *p, uint32_t step_code, uint64_t n_reads, const HostInput &in,
                             const char *reads_missing, HostSink sink, uint64_t *masses, uint32_t *flags_out, rk_counters *counters) {
    RK_TRY(check_params(p));  // (what needs no handle first: a machine without a GPU can test it)
    if (step_code > RK_STEP_TRANSLATED) return fail(RK_ERR_INVALID, "%s: step=%u (0 forward, 1 reverse, 2 both, 3 translated)", who, step_code);
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    HostStep step;
    if (step_code == RK_STEP_TRANSLATED) {
        RK_TRY(translated_handle(db, who));
        step.kind = HostStep::TRANSLATED;
    } else if (step_code != RK_STRAND_FORWARD) {
        RK_TRY(strands_handle(db, who));
        step.kind = HostStep::STRANDS; step.strand = step_code;
    }
    if (reads_missing) return fail(RK_ERR_INVALID, "%s: %s", who, reads_missing);
    rk_result out{nullptr, nullptr, nullptr, nullptr, flags_out};
    if (sink.n_samples) RK_TRY(check_members(who, db->info.n_branches, n_reads, sink));
    sink.masses = masses;
    return place_host(db, p, n_reads, in, &out, counters, who, step, sink);
}

extern "C" int rk_place_batch_masses(rk_db *db, const rk_params *p, uint32_t step, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off,
                                     const uint32_t *weights, uint64_t *masses, uint32_t *flags_out, rk_counters *counters) {
    const char *who = "rk_place_batch_masses";
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off;
    RK_GUARD_BEGIN
    return place_host_masses(who, db, p, step, n_reads, in, n_reads && (!seq_ascii || !seq_off) ? "null reads" : nullptr, weights_sink(weights), masses, flags_out, counters);
    RK_GUARD_END(who)
}

extern "C" int rk_place_batch_packed_masses(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                                            const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                                            const uint64_t *seq_off, const uint32_t *weights, uint64_t *masses, uint32_t *flags_out,
                                            rk_counters *counters) {
    const char *who = "rk_place_batch_packed_masses";
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    RK_TRY(check_params(p));
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (n_reads && (!packed || words_per_read == 0)) return fail(RK_ERR_INVALID, "%s: null packed reads", who);
    RK_TRY(check_fixed_len(who, lens, fixed_len, db->info.bits_per_symbol, words_per_read));
    if ((seq_ascii == nullptr) != (seq_off == nullptr)) return fail(RK_ERR_INVALID, "%s: seq_ascii and seq_off go together", who);
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off; in.packed = packed; in.wpr = words_per_read; in.lens = lens; in.fixed_len = fixed_len; in.flags = flags;
    RK_GUARD_BEGIN
    return place_host_masses(who, db, p, RK_STRAND_FORWARD, n_reads, in, nullptr, weights_sink(weights), masses, flags_out, counters);
    RK_GUARD_END(who)
}

// Per-sample profile-only placement: the same pipelines with the membership form of the masses sink
extern "C" int rk_place_batch_masses_samples(rk_db *db, const rk_params *p, uint32_t step, uint64_t n_reads, const uint8_t *seq_ascii,
                                             const uint64_t *seq_off, uint32_t n_samples, const uint64_t *member_off, const uint32_t *member_sample,
                                             const uint32_t *member_weight, uint64_t *masses, uint32_t *flags_out, rk_counters *counters) {
    const char *who = "rk_place_batch_masses_samples";
    if (n_samples == 0) return fail(RK_ERR_INVALID, "%s: n_samples=0 (1..65535)", who);
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off;
    RK_GUARD_BEGIN
    return place_host_masses(who, db, p, step, n_reads, in, n_reads && (!seq_ascii || !seq_off) ? "null reads" : nullptr,
                             members_sink(n_samples, member_off, member_sample, member_weight), masses, flags_out, counters);
    RK_GUARD_END(who)
}

extern "C" int rk_place_batch_packed_masses_samples(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *packed, uint32_t words_per_read,
                                                    const uint32_t *lens, uint32_t fixed_len, const uint32_t *flags, const uint8_t *seq_ascii,
                                                    const uint64_t *seq_off, uint32_t n_samples, const uint64_t *member_off,
                                                    const uint32_t *member_sample, const uint32_t *member_weight, uint64_t *masses,
                                                    uint32_t *flags_out, rk_counters *counters) {
    const char *who = "rk_place_batch_packed_masses_samples";
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    RK_TRY(check_params(p));
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (n_samples == 0) return fail(RK_ERR_INVALID, "%s: n_samples=0 (1..65535)", who);
    if (n_reads && (!packed || words_per_read == 0)) return fail(RK_ERR_INVALID, "%s: null packed reads", who);
    RK_TRY(check_fixed_len(who, lens, fixed_len, db->info.bits_per_symbol, words_per_read));
    if ((seq_ascii == nullptr) != (seq_off == nullptr)) return fail(RK_ERR_INVALID, "%s: seq_ascii and seq_off go together", who);
    HostInput in;
    in.ascii = seq_ascii; in.off = seq_off; in.packed = packed; in.wpr = words_per_read; in.lens = lens; in.fixed_len = fixed_len; in.flags = flags;
    RK_GUARD_BEGIN
    return place_host_masses(who, db, p, RK_STRAND_FORWARD, n_reads, in, nullptr, members_sink(n_samples, member_off, member_sample, member_weight), masses,
                             flags_out, counters);
    RK_GUARD_END(who)
}

// one host thread per device handle; contiguous shards; see include/rappas_place.h
extern "C" int rk_place_batch_multi(rk_db *const *dbs, uint32_t n_dbs, const rk_params *p, uint64_t n_reads,
                                    const uint8_t *seq_ascii, const uint64_t *seq_off, rk_result *out, rk_counters *counters) {
    if (!dbs || n_dbs == 0 || !out) return fail(RK_ERR_INVALID, "rk_place_batch_multi: null argument");
    for (uint32_t g = 0; g < n_dbs; g++)
        if (!dbs[g]) return fail(RK_ERR_INVALID, "rk_place_batch_multi: dbs[%u] is null", g);
    int rc = check_params(p);
    if (rc) return rc;
    if (n_dbs == 1 || n_reads == 0) return rk_place_batch(dbs[0], p, n_reads, seq_ascii, seq_off, out, counters);
    if (!seq_ascii || !seq_off) return fail(RK_ERR_INVALID, "rk_place_batch_multi: null reads");
    if (!result_complete(out)) return fail(RK_ERR_INVALID, "rk_place_batch_multi: null result array");
    const uint32_t K = p->keep_at_most;
    RK_GUARD_BEGIN
    std::vector<int> codes(n_dbs, RK_OK);
    std::vector<std::string> msgs(n_dbs);
    std::vector<rk_counters> cts(n_dbs);
    // developer / test knob: the first attempt of this shard reports a device failure (exercises the re-queue below)
#ifdef RK_DEV_KNOBS
    const int inject = rk_knob("RK_TEST_FAIL_SHARD") ? atoi(rk_knob("RK_TEST_FAIL_SHARD")) : -1;
#endif
    auto run_shard = [&](uint32_t g, uint32_t on, bool first_attempt) {  // shard g of the batch on handle `on`, in the calling thread
        const uint64_t lo = n_reads * g / n_dbs, hi = n_reads * (g + 1) / n_dbs;
        cts[g] = rk_counters{};
        codes[g] = RK_OK;
        if (hi == lo) return;
#ifdef RK_DEV_KNOBS
        if (first_attempt && inject == (int)g) {
            codes[g] = RK_ERR_HIP;
            msgs[g] = "injected failure (RK_TEST_FAIL_SHARD)";
            return;
        }
#else
        (void)first_attempt;
#endif
        rk_result r = result_slice(*out, lo, K);
        tl_concurrent_calls = first_attempt ? n_dbs : 1u;  // (this shard's thread: the host threads its call starts are 1 / n_dbs of the budget)
        codes[g] = rk_place_batch(dbs[on], p, hi - lo, seq_ascii, seq_off + lo, &r, &cts[g]);
        tl_concurrent_calls = 1;
        try {
            if (codes[g] != RK_OK) msgs[g] = rk_last_error();  // the message lives in this thread: hand it over
        } catch (...) {  // (nothing may leave a thread's function: std::terminate would take the hosting process down)
        }
    };
    struct JoinAll {  // joined on every way out of the scope, a throwing emplace_back included
        std::vector<std::thread> v;
        ~JoinAll() { for (std::thread &t : v) if (t.joinable()) t.join(); }
    };
    {
        JoinAll workers;
        workers.v.reserve(n_dbs);
        for (uint32_t g = 0; g < n_dbs; g++) workers.v.emplace_back([&, g]() { run_shard(g, g, true); });
    }
    // A shard whose device failed (per-GPU failure => shard re-queued on another GPU) is placed again on
    // the handles that did finish, one after the other, each attempt in a fresh host thread; the process is never restarted.
    // Argument errors (RK_ERR_INVALID / RK_ERR_UNSUPPORTED) would fail anywhere and are not retried.
    std::vector<char> healthy(n_dbs);
    for (uint32_t g = 0; g < n_dbs; g++) healthy[g] = codes[g] == RK_OK;
    std::string note;
    for (uint32_t g = 0; g < n_dbs; g++) {
        if (codes[g] == RK_OK || codes[g] == RK_ERR_INVALID || codes[g] == RK_ERR_UNSUPPORTED) continue;
        const std::string first_msg = msgs[g];
        const int first_code = codes[g];
        for (uint32_t h = 0; h < n_dbs && codes[g] != RK_OK; h++) {
            if (!healthy[h]) continue;
            {
                JoinAll one;
                one.v.emplace_back([&, g, h]() { run_shard(g, h, false); });
            }
            if (codes[g] == RK_OK) {
                char buf[256];
                snprintf(buf, sizeof(buf), "shard %u failed on device %d (%d: %.120s) and was placed on device %d; ", g, dbs[g]->info.device,
                         first_code, first_msg.c_str(), dbs[h]->info.device);
                note += buf;
            }
        }
        if (codes[g] != RK_OK) { codes[g] = first_code; msgs[g] = first_msg; }
    }
    rk_counters total{};
    for (uint32_t g = 0; g < n_dbs; g++) {
        if (codes[g] != RK_OK) return fail(codes[g], "rk_place_batch_multi: shard %u (device %d): %s", g, dbs[g]->info.device, msgs[g].c_str());
        rk::add(total, cts[g]);
    }
    if (counters) *counters = total;
    // success, but the caller can still learn which device dropped out: rk_last_error() carries the note (empty otherwise)
    (void)fail(RK_OK, "%s", note.c_str());
    return RK_OK;
    RK_GUARD_END("rk_place_batch_multi")
}
#undef RK_TRY
