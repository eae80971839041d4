// rk_samples_impl.h -- #included by rk_engine.hip: the sample-level entry points -- the tree handle (rk_tree_*),
// the clade sums of sample mass buffers (rk_clade_masses_device / _host), the KR distance matrix (rk_kr_distances_device / _host /
// _batch), the squash clustering over it (rk_squash_device / _host / _batch) and the edge principal components (rk_epca_device / _host /
// _batch / _finish_host) and the per-read EDPL (rk_edpl_device / _host / _batch, rk_tree_distance_host)
// and the phylogenetic k-means of the samples (rk_kmeans_device / _host / _batch)
// and the per-sample diversity measures (rk_diversity_device / _host / _batch, rk_diversity_math_host)
// and the edge statistics (rk_edgestat_device / _host / _batch / _finish_host)
// -- over the kernels of rk_samples.h, rk_epca.h, rk_edpl.h, rk_kmeans.h, rk_diversity.h and rk_edgestat.h and the host twins of rk_samples_host.h and rk_edgestat_host.h.  The calls read mass buffers that any masses call filled; they touch no placement kernel and no launch
// scratch, and only the _batch calls touch a database handle.
// What the analyses share exists once, ahead of them: the range tests (samples_range, squash_range, kmeans_range, diversity_range, epca_range), which
// the _host calls and the prepare step of every analysis read; the prepare step (tests, then the workspace plan, carved by Carve and
// measured by plan_fits), which _work_bytes and _device read; the workspace test of a device call (work_args); the tile grid of the two S x S matrices
// (launch_tiles); what the four host calls over the KR profiles start from (HostProfiles) and the thread count of every host call
// (host_threads); the frame of the five _batch calls (samples_batch) over what rk_edpl_batch shares with them (batch_handles,
// batch_stream, BatchBufs).  An analysis is a plan, a launch function, a host body and a few lines for each of its entry points.
#pragma once

#include "rk_samples_host.h"
#include "rk_edgestat_host.h"

static_assert(RK_KR_CHUNK == rk::KR_CHUNK && RK_KR_CHUNK == KR_CHUNK_IDS, "one chunk rule for the header, the host twin and the kernel");
constexpr uint64_t RK_KR_MAX_PART_BYTES = 1ull << 28;  // per-chunk partials while they stay below 256 MiB: beyond, the tiles alone fill the device
// A plan beyond this is refused (plan_fits).  Within the limits of the calls none comes near it: clade | U | V of 65535 samples on
// 65535 branches are 1.03e11 bytes, the partials of an S x S matrix at most RK_KR_MAX_PART_BYTES, and what an analysis adds stays
// below 2^31 (k-means at k = 64: 1.1e9).  Only a developer build whose RK_KR_PART_BYTES lifts the limit of the partials gets there.
constexpr uint64_t RK_KR_MAX_WORK_BYTES = 1ull << 40;

struct rk_tree {
    int32_t device = 0;
    uint32_t B = 0, root = 0;
    // one block: node_at[B] | end_at[B] | span_node[n_span] | span_end[n_span] | span_off[chunks + 1] (32-bit), then h[B] (binary64)
    void *d_block = nullptr;
    const u32 *node_at = nullptr, *end_at = nullptr, *span_node = nullptr, *span_end = nullptr, *span_off = nullptr;
    const double *h = nullptr;
    // behind h, for the distance between two branches (rk_edpl_device): node[B] (16 bytes each), then the lca_words 8-byte words of
    // dpar | depth | table as rk::tree_dist_build lays them out
    const EdplEntry *node = nullptr;
    const u64 *lca = nullptr;
    uint32_t lca_words = 0, cu_count = 256;
};

extern "C" int rk_tree_validate(uint32_t n_branches, const int32_t *parent, const float *branch_len) {
    RK_GUARD_BEGIN
    rk::TreeWalk w;
    return rk::tree_walk("rk_tree_validate", n_branches, parent, branch_len, true, w, g_err, sizeof(g_err)) ? RK_ERR_INVALID : RK_OK;
    RK_GUARD_END("rk_tree_validate")
}

extern "C" void rk_tree_destroy(rk_tree *t) {
    if (!t) return;
    if (t->d_block) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(t->device);
        (void)hipFree(t->d_block);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    delete t;
}

extern "C" int rk_tree_create(int32_t device, uint32_t n_branches, const int32_t *parent, const float *branch_len, rk_tree **out) {
    const char *who = "rk_tree_create";
    RK_GUARD_BEGIN
    if (!out) return fail(RK_ERR_INVALID, "%s: null out", who);
    *out = nullptr;
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, branch_len, true, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    const uint32_t B = n_branches, n_chunks = (B + CLADE_CHUNK - 1) / CLADE_CHUNK;
    // the nodes whose pre-order interval leaves the chunk it starts in, by the chunk it ends in (clade_masses_kernel)
    std::vector<uint32_t> end_at(B), span_off(n_chunks + 1, 0);
    for (uint32_t p = 0; p < B; p++) {
        end_at[p] = p + w.size[w.node_at[p]];
        if ((end_at[p] - 1) / CLADE_CHUNK != p / CLADE_CHUNK) span_off[(end_at[p] - 1) / CLADE_CHUNK + 1]++;
    }
    for (uint32_t c = 0; c < n_chunks; c++) span_off[c + 1] += span_off[c];
    const uint32_t n_span = span_off[n_chunks];
    std::vector<uint32_t> span_node(n_span), span_end(n_span), fill(span_off.begin(), span_off.end() - 1);
    for (uint32_t p = 0; p < B; p++)
        if ((end_at[p] - 1) / CLADE_CHUNK != p / CLADE_CHUNK) {
            const uint32_t k = fill[(end_at[p] - 1) / CLADE_CHUNK]++;
            span_node[k] = w.node_at[p];
            span_end[k] = end_at[p];
        }
    std::vector<double> h(B);
    for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(branch_len, x, w.root);
    rk::TreeDist dist;
    rk::tree_dist_build(w, parent, branch_len, dist);

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fail(RK_ERR_NO_DEVICE, "%s: no HIP device", who);
    if (device < 0 || device >= n_dev) return fail(RK_ERR_INVALID, "%s: device %d of %d", who, device, n_dev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rk_tree, void (*)(rk_tree *)> t(new (std::nothrow) rk_tree, rk_tree_destroy);
    if (!t) return fail(RK_ERR_NOMEM, "%s: no memory", who);
    t->device = device;
    t->B = B;
    t->root = w.root;
    const size_t n32 = 2 * (size_t)B + 2 * (size_t)n_span + n_chunks + 1, h_at = (n32 * 4 + 15) / 16 * 16;
    const size_t node_at = (h_at + (size_t)B * 8 + 15) / 16 * 16, lca_at = node_at + (size_t)B * sizeof(EdplEntry);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) t->cu_count = (uint32_t)cus;
    HIP_TRY(hipMalloc(&t->d_block, lca_at + dist.lca.size() * 8));
    u32 *d32 = (u32 *)t->d_block;
    t->node_at = d32;
    t->end_at = d32 + B;
    t->span_node = d32 + 2 * (size_t)B;
    t->span_end = t->span_node + n_span;
    t->span_off = t->span_end + n_span;
    t->h = (const double *)((char *)t->d_block + h_at);
    HIP_TRY(hipMemcpy((void *)t->node_at, w.node_at.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void *)t->end_at, end_at.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    if (n_span) {
        HIP_TRY(hipMemcpy((void *)t->span_node, span_node.data(), (size_t)n_span * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((void *)t->span_end, span_end.data(), (size_t)n_span * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy((void *)t->span_off, span_off.data(), (size_t)(n_chunks + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void *)t->h, h.data(), (size_t)B * 8, hipMemcpyHostToDevice));
    t->node = (const EdplEntry *)((char *)t->d_block + node_at);
    t->lca = (const u64 *)((char *)t->d_block + lca_at);
    t->lca_words = (uint32_t)dist.lca.size();
    HIP_TRY(hipMemcpy((void *)t->node, dist.node.data(), (size_t)B * sizeof(EdplEntry), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void *)t->lca, dist.lca.data(), dist.lca.size() * 8, hipMemcpyHostToDevice));
    *out = t.release();
    return RK_OK;
    RK_GUARD_END(who)
}

// ------------------------------------------------------------------------------------------------
// What the sample-level calls share.
// ------------------------------------------------------------------------------------------------
static int samples_range(const char *who, uint32_t S) {
    if (S < 1 || S > 65535) return fail(RK_ERR_INVALID, "%s: n_samples=%u must be in 1..65535", who, S);
    return RK_OK;
}

// Hands out the parts of a workspace in order: take(bytes, align) is the offset of the next part, total() the size of the whole
struct Carve {
    uint64_t at = 0;
    uint64_t take(uint64_t bytes, uint64_t align = 8) {
        const uint64_t here = (at + align - 1) / align * align;
        at = here + bytes;
        return here;
    }
    uint64_t total() const { return (at + 15) / 16 * 16; }
};

// the last test of every prepare step: the size of the finished plan
static int plan_fits(const char *who, const rk_tree *t, uint32_t S, uint64_t bytes) {
    if (bytes > RK_KR_MAX_WORK_BYTES) return fail(RK_ERR_INVALID, "%s: n_samples=%u on %u branches needs a workspace beyond 2^40 bytes", who, S, t->B);
    return RK_OK;
}

// the workspace test at the end of a device call's tests; `sizer` is the call that tells the size
static int work_args(const char *who, const char *sizer, const void *d_work, uint64_t work_bytes, uint64_t need) {
    if (!d_work || work_bytes < need)
        return fail(RK_ERR_INVALID, "%s: workspace of %llu bytes, %llu needed (%s)", who, (unsigned long long)(d_work ? work_bytes : 0), (unsigned long long)need, sizer);
    if ((uintptr_t)d_work % 16) return fail(RK_ERR_INVALID, "%s: the workspace must be 16-byte aligned", who);
    return RK_OK;
}

// the threads of a host call: the caller's count, or the CPUs up to 16; never more than 16, nor than the items there are to deal
static uint64_t host_threads(uint32_t n_threads, uint64_t items) {
    const unsigned hw = std::thread::hardware_concurrency();
    const uint64_t T = n_threads ? n_threads : std::min(hw ? hw : 1u, 16u);
    return std::max<uint64_t>(1, std::min<uint64_t>({T, 16, items}));
}

// What the host calls over the KR profiles start from (the caller has tested n_samples): the walk of the tree, the clade sums and the
// profiles u and v of every sample [S][B], the half lengths h[B], which samples have mass, and the thread count of the call.  The
// samples are dealt round to the threads.
struct HostProfiles {
    rk::TreeWalk w;
    std::vector<uint64_t> clade;
    std::vector<double> u, v, h;
    std::vector<uint8_t> active;
    uint32_t n_active = 0;
    uint64_t T = 1;
    int build(const char *who, uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t n_threads) {
        if (rk::tree_walk(who, n_branches, parent, branch_len, true, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
        if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
        const uint64_t B = n_branches, S = n_samples, W = rk_masses_words(n_branches);
        clade.resize(S * B);
        u.resize(S * B);
        v.resize(S * B);
        h.resize(B);
        active.resize(S);
        for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(branch_len, x, w.root);
        T = host_threads(n_threads, S);
        int rc = masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
            for (uint64_t s = th; s < S; s += T) {
                rk::clade_masses_sample(w, parent, masses + s * W, clade.data() + s * B);
                rk::kr_profiles_sample((uint32_t)B, w.root, masses + s * W, clade.data() + s * B, u.data() + s * B, v.data() + s * B);
            }
        });
        if (rc) return rc;
        for (uint64_t s = 0; s < S; s++) n_active += active[s] = clade[s * B + w.root] != 0;
        return RK_OK;
    }
};

// What every _batch call tests first: both handles, and that the tree is the database's
static int batch_handles(const char *who, const rk_db *db, const rk_tree *t) {
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (t->B != db->info.n_branches || t->device != db->info.device)
        return fail(RK_ERR_INVALID, "%s: the tree has %u branches on device %d, the database %u on device %d", who, t->B, t->device, db->info.n_branches, db->info.device);
    return RK_OK;
}
// the stream of a _batch call, on the database's device (the caller holds host_mutex)
static int batch_stream(rk_db *db, hipStream_t &s) {
    HIP_TRY(hipSetDevice(db->info.device));
    if (!db->ws[0].stream) HIP_TRY(hipStreamCreateWithFlags(&db->ws[0].stream, hipStreamNonBlocking));
    s = db->ws[0].stream;
    return RK_OK;
}
// the device buffers of a _batch call: allocated for the call, freed on every way out
struct BatchBufs {
    GrowBuf work, out, in;
    ~BatchBufs() { work.release(); out.release(); in.release(); }
};

// The frame of the five _batch calls over a sample mass buffer (the caller has tested its arguments): the buffer on the host -- or,
// masses == NULL, the one the last per-sample profile-only call (rk_place_batch_masses_samples, rk_place_batch_packed_masses_samples)
// left on the device in the handle --, a workspace of `need` bytes and `out_bytes` for the outputs on the device;
// queue(d_masses, d_out, d_work, stream) queues the device call and the downloads of its outputs, and the frame waits for them.
template <class Queue>
static int samples_batch(const char *who, rk_db *db, uint32_t n_samples, const uint64_t *masses, uint64_t need, uint64_t out_bytes, Queue queue) {
    const uint32_t B = db->info.n_branches;
    const uint64_t words = rk_masses_samples_words(B, n_samples);
    if (!words) return fail(RK_ERR_INVALID, "%s: n_samples=%u on %u branches is beyond the limits of a sample mass buffer", who, n_samples, B);
    std::lock_guard<std::mutex> lock(db->host_mutex);
    if (!masses && (db->masses_samples != n_samples || !db->d_masses.p))
        return fail(RK_ERR_INVALID, "%s: the handle holds the buffer of %u samples, not of %u (the last per-sample profile-only call leaves it)", who, db->masses_samples, n_samples);
    hipStream_t s;
    if (int rc = batch_stream(db, s)) return rc;
    BatchBufs b;
    if (int rc = b.work.reserve(need)) return rc;
    if (int rc = b.out.reserve(out_bytes)) return rc;
    const uint64_t *d_masses = db->d_masses.as<uint64_t>();
    if (masses) {
        if (int rc = b.in.reserve(words * 8)) return rc;
        HIP_TRY(hipMemcpyAsync(b.in.p, masses, words * 8, hipMemcpyHostToDevice, s));
        d_masses = b.in.as<uint64_t>();
    }
    if (int rc = queue(d_masses, (char *)b.out.p, b.work.p, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// Clade sums and KR distances: rk_clade_masses_device / _host, rk_kr_work_bytes / rk_kr_distances_device / _host / _batch.
// ------------------------------------------------------------------------------------------------
extern "C" int rk_clade_masses_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint64_t *d_clade, void *stream) {
    const char *who = "rk_clade_masses_device";
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = samples_range(who, n_samples)) return rc;
    if (!d_masses || !d_clade) return fail(RK_ERR_INVALID, "%s: null %s", who, d_masses ? "output" : "mass buffer");
    HIP_TRY(hipSetDevice(t->device));
    hipLaunchKernelGGL(clade_masses_kernel, dim3(n_samples), dim3(256), 0, (hipStream_t)stream, t->B, (u64)rk_masses_words(t->B), t->node_at, t->end_at, t->span_node,
                       t->span_end, t->span_off, (const u64 *)d_masses, (u64 *)d_clade);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_clade_masses_host(uint32_t n_branches, const int32_t *parent, uint32_t n_samples, const uint64_t *masses, uint64_t *clade) {
    const char *who = "rk_clade_masses_host";
    RK_GUARD_BEGIN
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, nullptr, false, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    if (int rc = samples_range(who, n_samples)) return rc;
    if (!masses || !clade) return fail(RK_ERR_INVALID, "%s: null %s", who, masses ? "output" : "mass buffer");
    const uint64_t B = n_branches, W = rk_masses_words(n_branches);
    for (uint64_t s = 0; s < n_samples; s++) rk::clade_masses_sample(w, parent, masses + s * W, clade + s * B);
    return RK_OK;
    RK_GUARD_END(who)
}

// The workspace of rk_kr_distances_device: clade[S][B] (64-bit) | u[B][S] | v[B][S] | the partials, chunks x S x S, when they are used.
// The analyses that start from the profiles carve theirs behind a plan without the pair partials: `to_part` is then the rule alone.
struct KrPlan {
    uint32_t n_chunks;
    bool to_part;
    uint64_t clade_at, u_at, v_at, part_at, bytes;
};
static KrPlan kr_plan(Carve &c, uint32_t B, uint32_t S, bool pair_partials) {
    const uint64_t sb = (uint64_t)S * B * 8, ss = (uint64_t)S * S * 8;
    KrPlan p;
    p.n_chunks = (B + RK_KR_CHUNK - 1) / RK_KR_CHUNK;
    uint64_t part_limit = RK_KR_MAX_PART_BYTES;
    if (const char *v = rk_knob("RK_KR_PART_BYTES")) part_limit = strtoull(v, nullptr, 10);  // developer builds: both forms on small shapes
    p.to_part = p.n_chunks > 1 && ss * p.n_chunks <= part_limit;
    p.clade_at = c.take(sb);
    p.u_at = c.take(sb);
    p.v_at = c.take(sb);
    p.part_at = c.take(pair_partials && p.to_part ? ss * p.n_chunks : 0);
    p.bytes = c.at;
    return p;
}
// the tests of rk_kr_work_bytes and rk_kr_distances_device, and the plan
static int kr_prepare(const char *who, const rk_tree *t, uint32_t S, KrPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = samples_range(who, S)) return rc;
    Carve c;
    p = kr_plan(c, t->B, S, true);
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_kr_work_bytes(const rk_tree *t, uint32_t n_samples) {
    KrPlan p;
    return kr_prepare("rk_kr_work_bytes", t, n_samples, p) ? 0 : p.bytes;
}

// The triangular grid of tiles over an S x S matrix that kr_pairs_kernel and epca_gram_kernel share: tiles(grid, side, chunks a block,
// to_part) launches the kernel; where the plan has per-chunk partials a block takes one chunk, and kr_reduce_kernel sums them into `out`.
template <class Tiles>
static int launch_tiles(uint32_t S, const KrPlan &p, const double *part, double *out, hipStream_t s, Tiles tiles) {
    const uint32_t side = (S + KR_TILE - 1) / KR_TILE;
    const uint64_t n_tiles = (uint64_t)side * (side + 1) / 2;
    tiles(dim3((unsigned)n_tiles, p.to_part ? p.n_chunks : 1), side, p.to_part ? 1u : p.n_chunks, p.to_part ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    if (p.to_part) {
        const uint64_t n = (uint64_t)S * S;
        hipLaunchKernelGGL(kr_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (u64)n, p.n_chunks, part, out);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

// The launches behind rk_kr_distances_device, each on its own for scripts/kr_rate.py (developer builds time them one by one).
static int kr_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, double *d_out, void *d_work, const KrPlan &p, hipStream_t s, unsigned steps = 7) {
    const uint32_t B = t->B;
    u64 *clade = (u64 *)((char *)d_work + p.clade_at);
    double *U = (double *)((char *)d_work + p.u_at), *V = (double *)((char *)d_work + p.v_at), *part = (double *)((char *)d_work + p.part_at);
    if (steps & 1) {
        hipLaunchKernelGGL(clade_masses_kernel, dim3(S), dim3(256), 0, s, B, (u64)rk_masses_words(B), t->node_at, t->end_at, t->span_node, t->span_end, t->span_off,
                           (const u64 *)d_masses, clade);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 2) {
        hipLaunchKernelGGL(kr_profiles_kernel, dim3((B + 31) / 32, (S + 31) / 32), dim3(256), 0, s, B, S, (u64)rk_masses_words(B), t->root, (const u64 *)d_masses,
                           (const u64 *)clade, U, V);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 4)
        return launch_tiles(S, p, part, d_out, s, [&](dim3 grid, uint32_t side, uint32_t chunks, uint32_t to_part) {
            hipLaunchKernelGGL(kr_pairs_kernel, grid, dim3(256), 0, s, B, S, side, chunks, to_part, (const double *)U, (const double *)V, t->h, d_out, part);
        });
    return RK_OK;
}

extern "C" int rk_kr_distances_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, double *d_out, void *d_work, uint64_t work_bytes,
                                      void *stream) {
    const char *who = "rk_kr_distances_device";
    KrPlan p;
    if (int rc = kr_prepare(who, t, n_samples, p)) return rc;
    if (!d_masses || !d_out) return fail(RK_ERR_INVALID, "%s: null %s", who, d_masses ? "output" : "mass buffer");
    if (int rc = work_args(who, "rk_kr_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 7;
    if (const char *v = rk_knob("RK_KR_STEPS")) steps = (unsigned)atoi(v);  // developer builds: bit 0 clade, 1 profiles, 2 pairs (scripts/kr_rate.py)
    return kr_launch(t, n_samples, d_masses, d_out, d_work, p, (hipStream_t)stream, steps);
}

extern "C" int rk_kr_distances_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses,
                                    double *out, uint32_t n_threads) {
    const char *who = "rk_kr_distances_host";
    RK_GUARD_BEGIN
    if (int rc = samples_range(who, n_samples)) return rc;
    if (!out) return fail(RK_ERR_INVALID, "%s: null output", who);
    HostProfiles p;
    if (int rc = p.build(who, n_branches, parent, branch_len, n_samples, masses, n_threads)) return rc;
    // rows of the matrix, dealt round to the threads (row s has S - s pairs: dealt, not cut into ranges)
    return masses_fan_out(who, p.T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        rk::kr_rows(n_branches, n_samples, p.h.data(), p.u.data(), p.v.data(), (uint32_t)th, (uint32_t)p.T, out);
    });
    RK_GUARD_END(who)
}

// The drivers' call: the matrix of a sample mass buffer to the host (samples_batch).  Workspace and matrix are allocated for the call
// and freed; it waits for the result.
extern "C" int rk_kr_distances_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, double *out) {
    const char *who = "rk_kr_distances_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    KrPlan p;
    if (int rc = kr_prepare(who, t, n_samples, p)) return rc;
    if (!out) return fail(RK_ERR_INVALID, "%s: null output", who);
    const uint64_t out_bytes = (uint64_t)n_samples * n_samples * 8;
    return samples_batch(who, db, n_samples, masses, p.bytes, out_bytes, [&](const uint64_t *d_masses, char *d_out, void *d_work, hipStream_t s) -> int {
        if (int rc = rk_kr_distances_device(t, n_samples, d_masses, (double *)d_out, d_work, p.bytes, s)) return rc;
        HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// Squash clustering: rk_squash_work_bytes / _device / _host / _batch.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(rk_squash_merge) == 24 && sizeof(SquashRow) == 24 && sizeof(rk::SquashMerge) == 24 && offsetof(rk_squash_merge, distance) == 16 &&
                  offsetof(SquashRow, distance) == 16 && offsetof(rk::SquashMerge, distance) == 16,
              "one row layout for the header, the host twin and the kernels");
static_assert(RK_SQUASH_NONE == SQUASH_FILLER && RK_SQUASH_NONE == rk::SQUASH_NONE, "one filler word");

// The workspace of rk_squash_device: the KR workspace | D[S][S] | ua[B] | va[B] | part[chunks][S] | the pick scratch | active[S] | size[S]
struct SquashPlan {
    KrPlan kr;
    uint32_t pick_blocks;
    uint64_t d_at, ua_at, va_at, part_at, scratch_at, active_at, size_at, bytes;
};
static int squash_range(const char *who, uint32_t S) {
    if (S < 2 || S > RK_SQUASH_MAX_SAMPLES) return fail(RK_ERR_INVALID, "%s: n_samples=%u must be in 2..%u", who, S, RK_SQUASH_MAX_SAMPLES);
    return RK_OK;
}
// the tests of rk_squash_work_bytes and rk_squash_device, and the plan
static int squash_prepare(const char *who, const rk_tree *t, uint32_t S, SquashPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = squash_range(who, S)) return rc;
    const uint64_t B = t->B;
    Carve c;
    p.kr = kr_plan(c, t->B, S, true);
    p.pick_blocks = std::min<uint32_t>(S - 1, SQUASH_PICK_BLOCKS);
    p.d_at = c.take((uint64_t)S * S * 8, 16);
    p.ua_at = c.take(B * 8);
    p.va_at = c.take(B * 8);
    p.part_at = c.take((uint64_t)p.kr.n_chunks * S * 8);
    p.scratch_at = c.take((uint64_t)p.pick_blocks * sizeof(SquashBest));
    p.active_at = c.take((uint64_t)S * 4, 4);
    p.size_at = c.take((uint64_t)S * 4, 4);
    p.bytes = c.total();
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_squash_work_bytes(const rk_tree *t, uint32_t n_samples) {
    SquashPlan p;
    return squash_prepare("rk_squash_work_bytes", t, n_samples, p) ? 0 : p.bytes;
}

// The launches behind rk_squash_device.  `steps` (developer builds, scripts/squash_rate.py): bit 0 the KR matrix and the start, 1 the
// pick, 2 the merge, 3 the row step, 4 its reduce.
static int squash_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, rk_squash_merge *d_merges, uint32_t *d_n_merges, void *d_work, const SquashPlan &p,
                         hipStream_t s, unsigned steps = 31) {
    const uint32_t B = t->B, n_chunks = p.kr.n_chunks;
    char *w = (char *)d_work;
    const u64 *clade = (const u64 *)(w + p.kr.clade_at);
    double *U = (double *)(w + p.kr.u_at), *V = (double *)(w + p.kr.v_at), *D = (double *)(w + p.d_at);
    double *ua = (double *)(w + p.ua_at), *va = (double *)(w + p.va_at), *part = (double *)(w + p.part_at);
    SquashBest *scratch = (SquashBest *)(w + p.scratch_at);
    u32 *active = (u32 *)(w + p.active_at), *size = (u32 *)(w + p.size_at);
    SquashRow *merges = (SquashRow *)d_merges;
    if (steps & 1) {
        if (int rc = kr_launch(t, S, d_masses, D, d_work, p.kr, s)) return rc;
        hipLaunchKernelGGL(squash_init_kernel, dim3(1), dim3(256), 0, s, B, S, t->root, clade, active, size, (u32 *)d_n_merges);
        HIP_TRY(hipGetLastError());
    }
    const dim3 row_grid(n_chunks, (S + SQUASH_GROUP - 1) / SQUASH_GROUP);
    for (uint32_t k = 0; k + 1 < S; k++) {
        if (steps & 2) {
            hipLaunchKernelGGL(squash_pick_kernel, dim3(p.pick_blocks), dim3(256), 0, s, S, (const double *)D, (const u32 *)active, scratch);
            hipLaunchKernelGGL(squash_pick_finish_kernel, dim3(1), dim3(256), 0, s, p.pick_blocks, k, (const SquashBest *)scratch, active, size, merges);
        }
        if (steps & 4)
            hipLaunchKernelGGL(squash_merge_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, S, k, (const SquashRow *)merges, (const u32 *)size, U, V, ua, va);
        if (steps & 8)
            hipLaunchKernelGGL(squash_row_kernel, row_grid, dim3(SQUASH_GROUP), 0, s, B, S, k, (const SquashRow *)merges, (const u32 *)active, (const double *)U,
                               (const double *)V, t->h, (const double *)ua, (const double *)va, part);
        if (steps & 16)
            hipLaunchKernelGGL(squash_row_reduce_kernel, dim3((S + 255) / 256), dim3(256), 0, s, S, k, n_chunks, (const SquashRow *)merges, (const u32 *)active,
                               (const double *)part, D);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

extern "C" int rk_squash_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, rk_squash_merge *d_merges, uint32_t *d_n_merges, void *d_work,
                                uint64_t work_bytes, void *stream) {
    const char *who = "rk_squash_device";
    SquashPlan p;
    if (int rc = squash_prepare(who, t, n_samples, p)) return rc;
    if (!d_masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (!d_merges || !d_n_merges) return fail(RK_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d_merges % 8 || (uintptr_t)d_n_merges % 4) return fail(RK_ERR_INVALID, "%s: the rows must be 8-byte aligned, the count 4-byte aligned", who);
    if (int rc = work_args(who, "rk_squash_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 31;
    if (const char *v = rk_knob("RK_SQUASH_STEPS")) steps = (unsigned)atoi(v);  // developer builds (scripts/squash_rate.py)
    if (!(steps & 1) || !(steps & 2)) steps &= 1;                               // (the steps behind the pick read the row it writes, the pick the start)
    return squash_launch(t, n_samples, d_masses, d_merges, d_n_merges, d_work, p, (hipStream_t)stream, steps);
}

extern "C" int rk_squash_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses,
                              rk_squash_merge *merges, uint32_t *n_merges, uint32_t n_threads) {
    const char *who = "rk_squash_host";
    RK_GUARD_BEGIN
    if (int rc = squash_range(who, n_samples)) return rc;
    if (!merges || !n_merges) return fail(RK_ERR_INVALID, "%s: null output", who);
    HostProfiles p;
    if (int rc = p.build(who, n_branches, parent, branch_len, n_samples, masses, n_threads)) return rc;
    const uint32_t B = n_branches, S = n_samples, T = (uint32_t)p.T;
    std::vector<double> D((uint64_t)S * S);
    int rc = masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        rk::kr_rows(B, S, p.h.data(), p.u.data(), p.v.data(), (uint32_t)th, T, D.data());
    });
    if (rc) return rc;
    *n_merges = rk::squash_steps(B, S, p.u.data(), p.v.data(), D.data(), p.active.data(), (rk::SquashMerge *)merges, [&](uint32_t a) {
        (void)masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
            rk::squash_row(B, S, p.h.data(), p.u.data(), p.v.data(), p.active.data(), a, (uint32_t)th, T, D.data());
        });
    });
    return RK_OK;
    RK_GUARD_END(who)
}

// The drivers' call: as rk_kr_distances_batch, with the rows and their count on the host at the end
extern "C" int rk_squash_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, rk_squash_merge *merges, uint32_t *n_merges) {
    const char *who = "rk_squash_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    SquashPlan p;
    if (int rc = squash_prepare(who, t, n_samples, p)) return rc;
    if (!merges || !n_merges) return fail(RK_ERR_INVALID, "%s: null output", who);
    const uint64_t rows_bytes = (uint64_t)(n_samples - 1) * sizeof(rk_squash_merge);  // the rows, then the count
    return samples_batch(who, db, n_samples, masses, p.bytes, rows_bytes + 8, [&](const uint64_t *d_masses, char *d_out, void *d_work, hipStream_t s) -> int {
        uint32_t *d_count = (uint32_t *)(d_out + rows_bytes);
        if (int rc = rk_squash_device(t, n_samples, d_masses, (rk_squash_merge *)d_out, d_count, d_work, p.bytes, s)) return rc;
        HIP_TRY(hipMemcpyAsync(merges, d_out, rows_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(n_merges, d_count, 4, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// Phylogenetic k-means: rk_kmeans_work_bytes / _device / _host / _batch.
// ------------------------------------------------------------------------------------------------
static_assert(RK_KMEANS_MAX_K == KMEANS_MAX_CENTROIDS && RK_KMEANS_MAX_K == rk::KMEANS_MAX_K && RK_KMEANS_GROUP == KMEANS_UPDATE_GROUP &&
                  RK_KMEANS_GROUP == rk::KMEANS_GROUP && RK_KMEANS_NONE == KMEANS_FILLER && RK_KMEANS_NONE == rk::KMEANS_NONE &&
                  RK_KMEANS_MAX_ROUNDS == rk::KMEANS_MAX_ROUNDS,
              "one set of constants for the header, the host twin and the kernels");

// The workspace of rk_kmeans_device: the KR workspace without its pair partials (clade | U | V) | cu[k][B] | cv[k][B] |
// part[chunks][k][S] | bestd[S] | mind[S] | best[S] | active[S] | members[k] | the control words
struct KmeansPlan {
    KrPlan kr;
    uint64_t cu_at, cv_at, part_at, bestd_at, mind_at, best_at, active_at, members_at, ctl_at, bytes;
};
static int kmeans_range(const char *who, uint32_t S, uint32_t k, uint32_t max_rounds) {
    if (int rc = samples_range(who, S)) return rc;
    if (k < 1 || k > RK_KMEANS_MAX_K) return fail(RK_ERR_INVALID, "%s: k=%u clusters must be in 1..%u", who, k, RK_KMEANS_MAX_K);
    if (max_rounds < 1 || max_rounds > RK_KMEANS_MAX_ROUNDS) return fail(RK_ERR_INVALID, "%s: max_rounds=%u must be in 1..%u", who, max_rounds, RK_KMEANS_MAX_ROUNDS);
    return RK_OK;
}
// the caller's seeds, on the host: k indices below S, no two the same
static int kmeans_seed_args(const char *who, uint32_t S, uint32_t k, const uint32_t *seeds) {
    if (!seeds) return RK_OK;
    for (uint32_t j = 0; j < k; j++) {
        if (seeds[j] >= S) return fail(RK_ERR_INVALID, "%s: seeds[%u]=%u, the buffer has %u samples", who, j, seeds[j], S);
        for (uint32_t i = 0; i < j; i++)
            if (seeds[i] == seeds[j]) return fail(RK_ERR_INVALID, "%s: seeds[%u] and seeds[%u] are both sample %u", who, i, j, seeds[j]);
    }
    return RK_OK;
}

// the tests of rk_kmeans_work_bytes and rk_kmeans_device, and the plan
static int kmeans_prepare(const char *who, const rk_tree *t, uint32_t S, uint32_t k, uint32_t max_rounds, KmeansPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = kmeans_range(who, S, k, max_rounds)) return rc;
    const uint64_t kb = (uint64_t)k * t->B * 8;
    Carve c;
    p.kr = kr_plan(c, t->B, S, false);
    p.cu_at = c.take(kb, 16);
    p.cv_at = c.take(kb);
    p.part_at = c.take((uint64_t)p.kr.n_chunks * k * S * 8);
    p.bestd_at = c.take((uint64_t)S * 8);
    p.mind_at = c.take((uint64_t)S * 8);
    p.best_at = c.take((uint64_t)S * 4, 4);
    p.active_at = c.take((uint64_t)S * 4, 4);
    p.members_at = c.take((uint64_t)k * 4, 4);
    p.ctl_at = c.take((uint64_t)KM_WORDS * 4, 4);
    p.bytes = c.total();
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_kmeans_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t k) {
    KmeansPlan p;
    return kmeans_prepare("rk_kmeans_work_bytes", t, n_samples, k, 1, p) ? 0 : p.bytes;
}

struct KmeansDeviceOut {
    uint32_t *assign;
    double *dist;
    uint32_t *sizes;
    double *within;
    uint32_t *info;
    double *centroids;
};

// The rung of kmeans_dist_kernel's ladder for k centroids: the largest -- none beyond the smallest that holds them all -- that still
// leaves four blocks a CU, and 1 where none does.  A block is one wave whose sums are KC dependent chains: more centroids a block
// stream U and V fewer times, fewer give more waves to hide the loads behind, and only a grid that fills the device gains from the
// first (profiles/kmeans_rate.txt: the measured best of every shape there is this rule's choice).
static uint32_t kmeans_rung(const rk_tree *t, uint32_t S, uint32_t k) {
    const uint64_t per_group = (uint64_t)((t->B + RK_KR_CHUNK - 1) / RK_KR_CHUNK) * ((S + KMEANS_WAVE - 1) / KMEANS_WAVE);
    for (uint32_t kc = 8; kc > 1; kc >>= 1)
        if (kc < 2 * k && per_group * ((k + kc - 1) / kc) >= 4ull * t->cu_count) return kc;
    return 1;
}

// The launches behind rk_kmeans_device.  `steps` (developer builds, scripts/kmeans_rate.py): bit 0 clade sums, profiles, the start and
// the seeding, 1 the distance step, 2 its reduce, 3 the assignment, 4 the update, 5 the centroid output.  `kc`: the rung of the ladder.
static int kmeans_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, uint32_t k, uint32_t max_rounds, const uint32_t *seeds, const KmeansDeviceOut &o,
                         void *d_work, const KmeansPlan &p, hipStream_t s, uint32_t kc, unsigned steps = 63) {
    const uint32_t B = t->B, n_chunks = p.kr.n_chunks;
    char *w = (char *)d_work;
    const u64 *clade = (const u64 *)(w + p.kr.clade_at);
    const double *U = (const double *)(w + p.kr.u_at), *V = (const double *)(w + p.kr.v_at);
    double *cu = (double *)(w + p.cu_at), *cv = (double *)(w + p.cv_at), *part = (double *)(w + p.part_at);
    double *bestd = (double *)(w + p.bestd_at), *mind = (double *)(w + p.mind_at);
    u32 *best = (u32 *)(w + p.best_at), *active = (u32 *)(w + p.active_at), *members = (u32 *)(w + p.members_at), *ctl = (u32 *)(w + p.ctl_at);
    const unsigned waves = (S + KMEANS_WAVE - 1) / KMEANS_WAVE, s_blocks = (S + 255) / 256, x_blocks = (B + 255) / 256;
    auto dist = [&](uint32_t rung, uint32_t j_base, uint32_t j_limit) {
        const dim3 grid(n_chunks, waves, (j_limit - j_base + rung - 1) / rung);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(KMEANS_WAVE), 0, s, B, S, k, j_base, j_limit, (const u32 *)ctl, (const u32 *)active, U, V, t->h, (const double *)cu,
                               (const double *)cv, part);
        };
        if (rung == 1) go(kmeans_dist_kernel<1>);
        else if (rung == 2) go(kmeans_dist_kernel<2>);
        else if (rung == 4) go(kmeans_dist_kernel<4>);
        else go(kmeans_dist_kernel<8>);
    };
    auto reduce = [&](uint32_t j_base, uint32_t j_limit) {
        hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(s_blocks), dim3(256), 0, s, S, k, n_chunks, j_base, j_limit, (const u32 *)ctl, (const u32 *)active,
                           (const double *)part, best, bestd);
    };
    if (steps & 1) {
        if (int rc = kr_launch(t, S, d_masses, nullptr, d_work, p.kr, s, 3)) return rc;
        KmeansSeeds given{};
        for (uint32_t j = 0; seeds && j < k; j++) given.s[j] = seeds[j];
        hipLaunchKernelGGL(kmeans_init_kernel, dim3(1), dim3(256), 0, s, B, S, k, t->root, seeds ? 1u : 0u, given, clade, ctl, active, (u32 *)o.assign, o.dist,
                           (u32 *)o.sizes, o.within, (u32 *)o.info);
        HIP_TRY(hipGetLastError());
        // the seeds' profiles as the first centroids; without caller's seeds, farthest-first: seed j from the distances to seed j - 1
        hipLaunchKernelGGL(kmeans_gather_kernel, dim3(x_blocks, seeds ? k : 1), dim3(256), 0, s, B, S, k, 0u, (const u32 *)ctl, U, V, cu, cv);
        for (uint32_t j = 1; !seeds && j < k; j++) {
            dist(1, j - 1, j);
            reduce(j - 1, j);
            hipLaunchKernelGGL(kmeans_seed_kernel, dim3(1), dim3(256), 0, s, S, k, j, ctl, active, (const double *)bestd, mind);
            hipLaunchKernelGGL(kmeans_gather_kernel, dim3(x_blocks, 1), dim3(256), 0, s, B, S, k, j, (const u32 *)ctl, U, V, cu, cv);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipGetLastError());
    }
    // the update kernel's lanes: 2^kp_log2 >= k clusters a node, and as many nodes a wave as fit while four blocks a CU are left
    uint32_t kp_log2 = 0;
    while ((1u << kp_log2) < k) kp_log2++;
    uint32_t nodes_log2 = 6 - kp_log2;
    while (nodes_log2 > 0 && (B >> nodes_log2) < 4 * t->cu_count) nodes_log2--;
    const uint32_t update_nodes = 1u << nodes_log2;
    for (uint32_t r = 0; r < max_rounds; r++) {
        if (steps & 2) dist(kc, 0, k);
        if (steps & 4) reduce(0, k);
        if (steps & 8)
            hipLaunchKernelGGL(kmeans_assign_kernel, dim3(1), dim3(256), 0, s, S, k, r, max_rounds, ctl, (const u32 *)active, (const u32 *)best, (const double *)bestd,
                               (u32 *)o.assign, o.dist, members, (u32 *)o.sizes, o.within, (u32 *)o.info);
        if (steps & 16)
            hipLaunchKernelGGL(kmeans_update_kernel, dim3((B + update_nodes - 1) / update_nodes), dim3(KMEANS_WAVE), 0, s, B, S, k, kp_log2, nodes_log2, (const u32 *)ctl,
                               (const u32 *)o.assign, (const u32 *)members, U, V, cu, cv);
        HIP_TRY(hipGetLastError());
    }
    if ((steps & 32) && o.centroids) {
        hipLaunchKernelGGL(kmeans_centroids_kernel, dim3(x_blocks, k), dim3(256), 0, s, B, k, (const u32 *)ctl, (const double *)cu, (const double *)cv, o.centroids);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

extern "C" int rk_kmeans_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t k, uint32_t max_rounds, const uint32_t *seeds,
                                uint32_t *d_assign, double *d_dist, uint32_t *d_sizes, double *d_within, uint32_t *d_info, double *d_centroids, void *d_work,
                                uint64_t work_bytes, void *stream) {
    const char *who = "rk_kmeans_device";
    KmeansPlan p;
    if (int rc = kmeans_prepare(who, t, n_samples, k, max_rounds, p)) return rc;
    if (!d_masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (!d_assign || !d_dist || !d_sizes || !d_within || !d_info) return fail(RK_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d_dist % 8 || (uintptr_t)d_within % 8 || (uintptr_t)d_centroids % 8 || (uintptr_t)d_assign % 4 || (uintptr_t)d_sizes % 4 || (uintptr_t)d_info % 4)
        return fail(RK_ERR_INVALID, "%s: the doubles must be 8-byte aligned, the 32-bit words 4-byte aligned", who);
    if (int rc = work_args(who, "rk_kmeans_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    if (int rc = kmeans_seed_args(who, n_samples, k, seeds)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 63;
    uint32_t kc = kmeans_rung(t, n_samples, k);
    if (const char *v = rk_knob("RK_KMEANS_STEPS")) steps = (unsigned)atoi(v);  // developer builds (scripts/kmeans_rate.py)
    if (const char *v = rk_knob("RK_KMEANS_KC")) {                              // developer builds: every rung of the ladder on one shape
        const uint32_t f = (uint32_t)atoi(v);
        if (f == 1 || f == 2 || f == 4 || f == 8) kc = f;
    }
    const KmeansDeviceOut o{d_assign, d_dist, d_sizes, d_within, d_info, d_centroids};
    return kmeans_launch(t, n_samples, d_masses, k, max_rounds, seeds, o, d_work, p, (hipStream_t)stream, kc, steps);
}

extern "C" int rk_kmeans_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t k,
                              uint32_t max_rounds, const uint32_t *seeds, uint32_t *assign, double *dist, uint32_t *sizes, double *within, uint32_t *info,
                              double *centroids, uint32_t n_threads) {
    const char *who = "rk_kmeans_host";
    RK_GUARD_BEGIN
    if (int rc = kmeans_range(who, n_samples, k, max_rounds)) return rc;
    if (!assign || !dist || !sizes || !within || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    if (int rc = kmeans_seed_args(who, n_samples, k, seeds)) return rc;
    HostProfiles p;
    if (int rc = p.build(who, n_branches, parent, branch_len, n_samples, masses, n_threads)) return rc;
    const uint64_t B = n_branches, S = n_samples, T = p.T;
    const std::vector<double> &u = p.u, &v = p.v, &h = p.h;
    const std::vector<uint8_t> &active = p.active;
    std::vector<double> cu(k * B), cv(k * B), Dc(k * S);
    const uint32_t n_active = p.n_active;
    uint32_t status = 0;
    for (uint32_t j = 0; seeds && j < k; j++) status |= !active[seeds[j]];
    const uint32_t k_eff = seeds ? k : std::min(k, n_active);
    const rk::KmeansOut o{assign, dist, sizes, within, info, centroids};
    if (n_active == 0 || status) {
        rk::kmeans_fill((uint32_t)B, (uint32_t)S, k, k_eff, n_active, status, o);
        return RK_OK;
    }
    // samples, then clusters, dealt round to the threads
    auto dist_step = [&](uint32_t j_lo, uint32_t j_hi) {
        (void)masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
            rk::kmeans_distances((uint32_t)B, (uint32_t)S, h.data(), u.data(), v.data(), active.data(), cu.data(), cv.data(), j_lo, j_hi, (uint32_t)th, (uint32_t)T, Dc.data());
        });
    };
    auto update_step = [&]() {
        (void)masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
            rk::kmeans_update((uint32_t)B, (uint32_t)S, k_eff, u.data(), v.data(), assign, (uint32_t)th, (uint32_t)T, cu.data(), cv.data());
        });
    };
    if (seeds) {
        for (uint64_t j = 0; j < k; j++)
            for (uint64_t x = 0; x < B; x++) {
                cu[j * B + x] = u[seeds[j] * B + x];
                cv[j * B + x] = v[seeds[j] * B + x];
            }
    } else {
        std::vector<uint32_t> found(k_eff);
        rk::kmeans_seed((uint32_t)B, (uint32_t)S, k_eff, u.data(), v.data(), active.data(), cu.data(), cv.data(), Dc.data(), found.data(), dist_step);
    }
    rk::kmeans_rounds((uint32_t)B, (uint32_t)S, k, k_eff, n_active, max_rounds, active.data(), cu.data(), cv.data(), Dc.data(), o, dist_step, update_step);
    return RK_OK;
    RK_GUARD_END(who)
}

// The drivers' call: as rk_squash_batch, with the outputs on the host at the end
extern "C" int rk_kmeans_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t k, uint32_t max_rounds, const uint32_t *seeds,
                               uint32_t *assign, double *dist, uint32_t *sizes, double *within, uint32_t *info, double *centroids) {
    const char *who = "rk_kmeans_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    KmeansPlan p;
    if (int rc = kmeans_prepare(who, t, n_samples, k, max_rounds, p)) return rc;
    if (!assign || !dist || !sizes || !within || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    // dist[S] | within[k] | centroids[k][2][B] when wanted | assign[S] | sizes[k] | info[4]
    Carve c;
    const uint64_t S = n_samples, cen_bytes = centroids ? (uint64_t)k * 2 * t->B * 8 : 0;
    const uint64_t dist_at = c.take(S * 8), within_at = c.take((uint64_t)k * 8), cen_at = c.take(cen_bytes);
    const uint64_t assign_at = c.take(S * 4, 4), sizes_at = c.take((uint64_t)k * 4, 4), info_at = c.take(16, 4);
    return samples_batch(who, db, n_samples, masses, p.bytes, c.at, [&](const uint64_t *d_masses, char *base, void *d_work, hipStream_t s) -> int {
        if (int rc = rk_kmeans_device(t, n_samples, d_masses, k, max_rounds, seeds, (uint32_t *)(base + assign_at), (double *)(base + dist_at),
                                      (uint32_t *)(base + sizes_at), (double *)(base + within_at), (uint32_t *)(base + info_at),
                                      centroids ? (double *)(base + cen_at) : nullptr, d_work, p.bytes, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(dist, base + dist_at, S * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(within, base + within_at, (uint64_t)k * 8, hipMemcpyDeviceToHost, s));
        if (centroids) HIP_TRY(hipMemcpyAsync(centroids, base + cen_at, cen_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(assign, base + assign_at, S * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sizes, base + sizes_at, (uint64_t)k * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(info, base + info_at, 16, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// Per-sample diversity measures: rk_diversity_work_bytes / _device / _host / _batch, rk_diversity_math_host.
// ------------------------------------------------------------------------------------------------
static_assert(RK_DIVERSITY_FIXED == rk::DIVERSITY_FIXED && RK_DIVERSITY_MAX_THETA == rk::DIVERSITY_MAX_THETA && RK_DIVERSITY_LANES == rk::DIVERSITY_LANES,
              "one set of constants for the header, the host twin and the kernels");

// The workspace of rk_diversity_device: clade[S][B] (64-bit) | part[S][chunks][5 + 2 n_theta]
struct DiversityPlan {
    uint32_t n_chunks, n_cols;
    uint64_t clade_at, part_at, bytes;
};
static int diversity_range(const char *who, uint32_t S, uint32_t n_theta) {
    if (int rc = samples_range(who, S)) return rc;
    if (n_theta > RK_DIVERSITY_MAX_THETA) return fail(RK_ERR_INVALID, "%s: n_theta=%u must be in 0..%u", who, n_theta, RK_DIVERSITY_MAX_THETA);
    return RK_OK;
}
// the caller's thetas, on the host: finite and in 0..8
static int diversity_theta_args(const char *who, uint32_t n_theta, const double *theta) {
    return rk::diversity_theta_args(who, n_theta, theta, g_err, sizeof(g_err)) ? RK_ERR_INVALID : RK_OK;
}
// the tests of rk_diversity_work_bytes and rk_diversity_device, and the plan
static int diversity_prepare(const char *who, const rk_tree *t, uint32_t S, uint32_t n_theta, DiversityPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = diversity_range(who, S, n_theta)) return rc;
    Carve c;
    p.n_chunks = (t->B + RK_KR_CHUNK - 1) / RK_KR_CHUNK;
    p.n_cols = RK_DIVERSITY_FIXED + 2 * n_theta;
    p.clade_at = c.take((uint64_t)S * t->B * 8);
    p.part_at = c.take((uint64_t)S * p.n_chunks * p.n_cols * 8);
    p.bytes = c.total();
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_diversity_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t n_theta) {
    DiversityPlan p;
    return diversity_prepare("rk_diversity_work_bytes", t, n_samples, n_theta, p) ? 0 : p.bytes;
}

// The launches behind rk_diversity_device.  `steps` (developer builds, scripts/diversity_rate.py): bit 0 the clade sums, 1 the measure
// kernel, 2 its reduce.
static int diversity_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, uint32_t n_theta, const double *theta, double *d_out, void *d_work,
                            const DiversityPlan &p, hipStream_t s, unsigned steps = 7) {
    const uint32_t B = t->B;
    u64 *clade = (u64 *)((char *)d_work + p.clade_at);
    double *part = (double *)((char *)d_work + p.part_at);
    const u64 W = (u64)rk_masses_words(B);
    if (steps & 1) {
        hipLaunchKernelGGL(clade_masses_kernel, dim3(S), dim3(256), 0, s, B, W, t->node_at, t->end_at, t->span_node, t->span_end, t->span_off, (const u64 *)d_masses, clade);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 2) {
        DiversityThetas th{};
        for (uint32_t i = 0; i < n_theta; i++) th.v[i] = theta[i];
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(p.n_chunks, S), dim3(DIVERSITY_LANES), 0, s, B, W, t->root, p.n_chunks, th, (const u64 *)d_masses, (const u64 *)clade, t->h, part);
        };
        switch (n_theta) {
        case 0: go(diversity_kernel<0>); break;
        case 1: go(diversity_kernel<1>); break;
        case 2: go(diversity_kernel<2>); break;
        case 3: go(diversity_kernel<3>); break;
        case 4: go(diversity_kernel<4>); break;
        case 5: go(diversity_kernel<5>); break;
        case 6: go(diversity_kernel<6>); break;
        case 7: go(diversity_kernel<7>); break;
        default: go(diversity_kernel<8>); break;
        }
        HIP_TRY(hipGetLastError());
    }
    if (steps & 4) {
        const uint64_t n = (uint64_t)S * p.n_cols;
        hipLaunchKernelGGL(diversity_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, B, S, t->root, p.n_chunks, p.n_cols, (const u64 *)clade,
                           (const double *)part, d_out);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

extern "C" int rk_diversity_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t n_theta, const double *theta, double *d_out, void *d_work,
                                   uint64_t work_bytes, void *stream) {
    const char *who = "rk_diversity_device";
    DiversityPlan p;
    if (int rc = diversity_prepare(who, t, n_samples, n_theta, p)) return rc;
    if (!d_masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (!d_out) return fail(RK_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d_out % 8) return fail(RK_ERR_INVALID, "%s: the doubles must be 8-byte aligned", who);
    if (int rc = work_args(who, "rk_diversity_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    if (int rc = diversity_theta_args(who, n_theta, theta)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 7;
    if (const char *v = rk_knob("RK_DIVERSITY_STEPS")) steps = (unsigned)atoi(v);  // developer builds (scripts/diversity_rate.py)
    return diversity_launch(t, n_samples, d_masses, n_theta, theta, d_out, d_work, p, (hipStream_t)stream, steps);
}

extern "C" int rk_diversity_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t n_theta,
                                 const double *theta, double *out, uint32_t n_threads) {
    const char *who = "rk_diversity_host";
    RK_GUARD_BEGIN
    if (int rc = diversity_range(who, n_samples, n_theta)) return rc;
    if (!out) return fail(RK_ERR_INVALID, "%s: null output", who);
    if (int rc = diversity_theta_args(who, n_theta, theta)) return rc;
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, branch_len, true, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    const uint64_t B = n_branches, S = n_samples, W = rk_masses_words(n_branches), C = RK_DIVERSITY_FIXED + 2 * (uint64_t)n_theta;
    std::vector<double> h(B);
    for (uint32_t x = 0; x < B; x++) h[x] = rk::kr_half_length(branch_len, x, w.root);
    const uint64_t T = host_threads(n_threads, S);
    // samples dealt round to the threads, each with clade sums of its own
    return masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        std::vector<uint64_t> clade(B);
        for (uint64_t s = th; s < S; s += T) {
            rk::clade_masses_sample(w, parent, masses + s * W, clade.data());
            rk::diversity_sample((uint32_t)B, w.root, masses + s * W, clade.data(), h.data(), n_theta, theta, out + s * C);
        }
    });
    RK_GUARD_END(who)
}

// The drivers' call: as rk_kmeans_batch, with the table [S][5 + 2 n_theta] on the host at the end
extern "C" int rk_diversity_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t n_theta, const double *theta, double *out) {
    const char *who = "rk_diversity_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    DiversityPlan p;
    if (int rc = diversity_prepare(who, t, n_samples, n_theta, p)) return rc;
    if (!out) return fail(RK_ERR_INVALID, "%s: null output", who);
    if (int rc = diversity_theta_args(who, n_theta, theta)) return rc;
    const uint64_t out_bytes = (uint64_t)n_samples * p.n_cols * 8;
    return samples_batch(who, db, n_samples, masses, p.bytes, out_bytes, [&](const uint64_t *d_masses, char *d_out, void *d_work, hipStream_t s) -> int {
        if (int rc = rk_diversity_device(t, n_samples, d_masses, n_theta, theta, (double *)d_out, d_work, p.bytes, s)) return rc;
        HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

// The functions of rk_divmath.h for the tests: out[i] = rk_log2(x[i]) (op 0), rk_exp2(x[i]) (1), pw(x[i], y[i]) (2)
extern "C" int rk_diversity_math_host(uint32_t op, uint64_t n, const double *x, const double *y, double *out) {
    const char *who = "rk_diversity_math_host";
    if (op > 2) return fail(RK_ERR_INVALID, "%s: op=%u must be 0 (log2), 1 (exp2) or 2 (pw)", who, op);
    if (n && (!x || !out)) return fail(RK_ERR_INVALID, "%s: null %s", who, x ? "output" : "input");
    if (n && op == 2 && !y) return fail(RK_ERR_INVALID, "%s: null theta array", who);
    for (uint64_t i = 0; i < n; i++)
        out[i] = op == 0 ? rk::rk_log2(x[i]) : op == 1 ? rk::rk_exp2(x[i]) : rk::rk_pw(x[i], rk::rk_log2(x[i]), y[i]);
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// Edge principal components: rk_epca_out_doubles / _work_bytes / _device / _host / _batch / _finish_host.
// ------------------------------------------------------------------------------------------------
static_assert(RK_EPCA_MAX_SAMPLES == rk::EPCA_MAX_SAMPLES && RK_EPCA_MAX_COMPONENTS == rk::EPCA_MAX_COMPONENTS && RK_EPCA_MAX_COMPONENTS == EPCA_MAX_K,
              "one set of limits for the header, the host twin and the kernels");

// The workspace of rk_epca_device: the KR workspace without its pair partials (clade | u, which becomes Xc | v) | G[S][S] | the Gram
// partials, chunks x S x S, when they are used | two column blocks [k][S] (the product reads one and writes the other) | active[S]
struct EpcaPlan {
    KrPlan kr;
    uint64_t g_at, part_at, qa_at, qb_at, active_at, bytes;
};
static int epca_range(const char *who, uint32_t S, uint32_t k, uint32_t iters) {
    if (S < 2 || S > RK_EPCA_MAX_SAMPLES) return fail(RK_ERR_INVALID, "%s: n_samples=%u must be in 2..%u", who, S, RK_EPCA_MAX_SAMPLES);
    if (k < 1 || k > RK_EPCA_MAX_COMPONENTS) return fail(RK_ERR_INVALID, "%s: k=%u components must be in 1..%u", who, k, RK_EPCA_MAX_COMPONENTS);
    if (iters < 1 || iters > rk::EPCA_MAX_ITERS) return fail(RK_ERR_INVALID, "%s: iters=%u must be in 1..%u", who, iters, rk::EPCA_MAX_ITERS);
    return RK_OK;
}
// the tests of rk_epca_work_bytes and rk_epca_device, and the plan
static int epca_prepare(const char *who, const rk_tree *t, uint32_t S, uint32_t k, uint32_t iters, EpcaPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = epca_range(who, S, k, iters)) return rc;
    const uint64_t ss = (uint64_t)S * S * 8;
    Carve c;
    p.kr = kr_plan(c, t->B, S, false);
    p.g_at = c.take(ss, 16);
    p.part_at = c.take(p.kr.to_part ? ss * p.kr.n_chunks : 0);
    p.qa_at = c.take((uint64_t)k * S * 8);
    p.qb_at = c.take((uint64_t)k * S * 8);
    p.active_at = c.take((uint64_t)S * 4, 4);
    p.bytes = c.total();
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_epca_out_doubles(uint32_t n_branches, uint32_t n_samples, uint32_t k) {
    if (n_branches < 1 || n_branches > 65535 || n_samples < 2 || n_samples > RK_EPCA_MAX_SAMPLES || k < 1 || k > RK_EPCA_MAX_COMPONENTS) return 0;
    return rk::epca_out_doubles(n_branches, n_samples, k);
}

extern "C" uint64_t rk_epca_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t k) {
    EpcaPlan p;
    return epca_prepare("rk_epca_work_bytes", t, n_samples, k, 1, p) ? 0 : p.bytes;
}

// The launches behind rk_epca_device.  `steps` (developer builds, scripts/epca_rate.py): bit 0 clade sums, profiles and the start,
// 1 the centring pass, 2 the Gram matrix, 3 the iterations, 4 the results and the loadings.  Every kernel keeps to the k columns and
// the S samples whatever the workspace holds, so any subset is safe to time on a workspace a whole call has used.
static int epca_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, uint32_t k, uint32_t iters, double *d_raw, uint32_t *d_info, void *d_work,
                       const EpcaPlan &p, hipStream_t s, unsigned steps = 31) {
    const uint32_t B = t->B;
    char *w = (char *)d_work;
    const u64 *clade = (const u64 *)(w + p.kr.clade_at);
    double *Xc = (double *)(w + p.kr.u_at), *V = (double *)(w + p.kr.v_at), *G = (double *)(w + p.g_at), *part = (double *)(w + p.part_at);
    double *qa = (double *)(w + p.qa_at), *qb = (double *)(w + p.qb_at);
    u32 *active = (u32 *)(w + p.active_at);
    const u32 *info = (const u32 *)d_info;
    const unsigned rows = (S + EPCA_WAVES - 1) / EPCA_WAVES, nodes = (B + EPCA_WAVES - 1) / EPCA_WAVES;
    if (steps & 1) {
        if (int rc = kr_launch(t, S, d_masses, nullptr, d_work, p.kr, s, 3)) return rc;
        hipLaunchKernelGGL(epca_init_kernel, dim3(1), dim3(256), 0, s, B, S, k, t->root, clade, active, (u32 *)d_info, qa);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 2) {
        hipLaunchKernelGGL(epca_centre_kernel, dim3(nodes), dim3(64 * EPCA_WAVES), 0, s, B, S, t->root, (const u32 *)active, info, Xc, (const double *)V);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 4) {
        int rc = launch_tiles(S, p.kr, part, G, s, [&](dim3 grid, uint32_t side, uint32_t chunks, uint32_t to_part) {
            hipLaunchKernelGGL(epca_gram_kernel, grid, dim3(256), 0, s, B, S, side, chunks, to_part, (const double *)Xc, G, part);
        });
        if (rc) return rc;
    }
    double *q = qa, *y = qb;
    if (steps & 8)
        for (uint32_t it = 0; it < iters; it++) {
            hipLaunchKernelGGL(epca_multiply_kernel, dim3(rows), dim3(64 * EPCA_WAVES), 0, s, S, k, info, (const double *)G, (const double *)q, y);
            hipLaunchKernelGGL(epca_orth_kernel, dim3(1), dim3(64 * EPCA_WAVES), 0, s, S, k, it == 0 ? 1u : 0u, info, y);
            HIP_TRY(hipGetLastError());
            std::swap(q, y);
        }
    if (steps & 16) {
        double *w_out = d_raw + 1 + (uint64_t)k * (3 + (uint64_t)S);
        hipLaunchKernelGGL(epca_multiply_kernel, dim3(rows), dim3(64 * EPCA_WAVES), 0, s, S, k, info, (const double *)G, (const double *)q, y);
        hipLaunchKernelGGL(epca_results_kernel, dim3(1), dim3(64 * EPCA_WAVES), 0, s, S, k, info, (const double *)G, (const double *)q, (const double *)y, d_raw);
        hipLaunchKernelGGL(epca_loadings_kernel, dim3(nodes), dim3(64 * EPCA_WAVES), 0, s, B, S, k, info, (const double *)Xc, (const double *)q, w_out);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

extern "C" int rk_epca_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t k, uint32_t iters, double *d_raw, uint32_t *d_info,
                              void *d_work, uint64_t work_bytes, void *stream) {
    const char *who = "rk_epca_device";
    EpcaPlan p;
    if (int rc = epca_prepare(who, t, n_samples, k, iters, p)) return rc;
    if (!d_masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (!d_raw || !d_info) return fail(RK_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d_raw % 8 || (uintptr_t)d_info % 4) return fail(RK_ERR_INVALID, "%s: the raw output must be 8-byte aligned, the info words 4-byte aligned", who);
    if (int rc = work_args(who, "rk_epca_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 31;
    if (const char *v = rk_knob("RK_EPCA_STEPS")) steps = (unsigned)atoi(v);  // developer builds (scripts/epca_rate.py)
    return epca_launch(t, n_samples, d_masses, k, iters, d_raw, d_info, d_work, p, (hipStream_t)stream, steps);
}

extern "C" int rk_epca_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_samples, const uint64_t *masses, uint32_t k,
                            uint32_t iters, double *raw, uint32_t *info, uint32_t n_threads) {
    const char *who = "rk_epca_host";
    RK_GUARD_BEGIN
    if (int rc = epca_range(who, n_samples, k, iters)) return rc;
    if (!raw || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    HostProfiles p;
    if (int rc = p.build(who, n_branches, parent, branch_len, n_samples, masses, n_threads)) return rc;
    const uint64_t B = n_branches, S = n_samples, T = p.T;
    std::vector<double> &u = p.u;  // (u becomes the centred matrix)
    std::vector<double> G(S * S), cols(2 * (uint64_t)k * S);
    const uint32_t n = p.n_active;
    const uint32_t k_eff = n < 2 ? 0u : std::min(k, n - 1);
    info[0] = n;
    info[1] = k_eff;
    const uint64_t n_out = rk::epca_out_doubles(n_branches, n_samples, k);
    for (uint64_t i = 0; i < n_out; i++) raw[i] = 0.0;
    if (!k_eff) return RK_OK;
    // nodes, then rows of G, dealt round to the threads
    int rc = masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        rk::epca_centre((uint32_t)B, (uint32_t)S, p.w.root, p.active.data(), n, u.data(), p.v.data(), (uint32_t)th, (uint32_t)T, u.data());
    });
    if (rc) return rc;
    rc = masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) { rk::epca_gram_rows((uint32_t)B, (uint32_t)S, u.data(), (uint32_t)th, (uint32_t)T, G.data()); });
    if (rc) return rc;
    rk::epca_iterate((uint32_t)B, (uint32_t)S, k, k_eff, iters, G.data(), u.data(), cols.data(), raw);
    return RK_OK;
    RK_GUARD_END(who)
}

// The drivers' call: as rk_kr_distances_batch, with the raw output and the two info words on the host at the end
extern "C" int rk_epca_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t k, uint32_t iters, double *raw, uint32_t *info) {
    const char *who = "rk_epca_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    EpcaPlan p;
    if (int rc = epca_prepare(who, t, n_samples, k, iters, p)) return rc;
    if (!raw || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    const uint64_t raw_bytes = rk::epca_out_doubles(t->B, n_samples, k) * 8;  // the raw output, then the info words
    return samples_batch(who, db, n_samples, masses, p.bytes, raw_bytes + 8, [&](const uint64_t *d_masses, char *d_out, void *d_work, hipStream_t s) -> int {
        uint32_t *d_info = (uint32_t *)(d_out + raw_bytes);
        if (int rc = rk_epca_device(t, n_samples, d_masses, k, iters, (double *)d_out, d_info, d_work, p.bytes, s)) return rc;
        HIP_TRY(hipMemcpyAsync(raw, d_out, raw_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(info, d_info, 8, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

extern "C" int rk_epca_finish_host(uint32_t n_branches, uint32_t n_samples, uint32_t k, const double *raw, double *eigenvalue, double *share, double *residual,
                                   double *projection, double *loading) {
    const char *who = "rk_epca_finish_host";
    if (!rk_epca_out_doubles(n_branches, n_samples, k))
        return fail(RK_ERR_INVALID, "%s: n_branches=%u, n_samples=%u, k=%u: out of 1..65535, 2..%u, 1..%u", who, n_branches, n_samples, k, RK_EPCA_MAX_SAMPLES, RK_EPCA_MAX_COMPONENTS);
    if (!raw) return fail(RK_ERR_INVALID, "%s: null raw output", who);
    if (!eigenvalue || !share || !residual || !projection || !loading) return fail(RK_ERR_INVALID, "%s: null output", who);
    rk::epca_finish(n_branches, n_samples, k, raw, eigenvalue, share, residual, projection, loading);
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// Edge statistics, edge dispersion and edge correlation: rk_edgestat_out_words / _work_bytes / _device / _host /
// _batch / _finish_host.
// ------------------------------------------------------------------------------------------------
static_assert(RK_EDGESTAT_MAX_SAMPLES == rk::EDGESTAT_MAX_SAMPLES && RK_EDGESTAT_MAX_FEATURES == rk::EDGESTAT_MAX_FEATURES && RK_EDGESTAT_MAX_FEATURES == EDGESTAT_MAX_F &&
                  rk::EDGESTAT_NAN == EDGESTAT_FILLER && RK_EDGESTAT_COUNT_MAX_SAMPLES <= EDGESTAT_COUNT_LIMIT,
              "one set of constants for the header, the host twin and the kernels");

// The workspace of rk_edgestat_device: clade[S][B] (64-bit) | P0[B][S] | P1[B][S] | gc[F][S] | gd[F][S] (32-bit) | active[S]
struct EdgestatPlan {
    uint64_t clade_at, p0_at, p1_at, gc_at, gd_at, active_at, bytes;
};
static int edgestat_range(const char *who, uint32_t S, uint32_t F) {
    if (S < 1 || S > RK_EDGESTAT_MAX_SAMPLES) return fail(RK_ERR_INVALID, "%s: n_samples=%u must be in 1..%u", who, S, RK_EDGESTAT_MAX_SAMPLES);
    if (F > RK_EDGESTAT_MAX_FEATURES) return fail(RK_ERR_INVALID, "%s: n_features=%u must be in 0..%u", who, F, RK_EDGESTAT_MAX_FEATURES);
    return RK_OK;
}
// the tests of rk_edgestat_work_bytes and rk_edgestat_device, and the plan
static int edgestat_prepare(const char *who, const rk_tree *t, uint32_t S, uint32_t F, EdgestatPlan &p) {
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    if (int rc = edgestat_range(who, S, F)) return rc;
    const uint64_t sb = (uint64_t)S * t->B * 8;
    Carve c;
    p.clade_at = c.take(sb);
    p.p0_at = c.take(sb);
    p.p1_at = c.take(sb);
    p.gc_at = c.take((uint64_t)F * S * 8);
    p.gd_at = c.take((uint64_t)F * S * 4, 4);
    p.active_at = c.take((uint64_t)S * 4, 4);
    p.bytes = c.total();
    return plan_fits(who, t, S, p.bytes);
}

extern "C" uint64_t rk_edgestat_out_words(uint32_t n_branches, uint32_t n_features) {
    if (n_branches < 1 || n_branches > 65535 || n_features > RK_EDGESTAT_MAX_FEATURES) return 0;
    return rk::edgestat_out_words(n_branches, n_features);
}

extern "C" uint64_t rk_edgestat_work_bytes(const rk_tree *t, uint32_t n_samples, uint32_t n_features) {
    EdgestatPlan p;
    return edgestat_prepare("rk_edgestat_work_bytes", t, n_samples, n_features, p) ? 0 : p.bytes;
}

// The launches behind rk_edgestat_device.  `steps` (developer builds, scripts/edgestat_rate.py): bit 0 the clade sums, 1 the profiles,
// 2 the start and the column prelude, 3 the edge kernel.  `cross`: rows of at most this many samples are ranked by counting.
static int edgestat_launch(const rk_tree *t, uint32_t S, const uint64_t *d_masses, uint32_t F, const double *d_meta, uint64_t *d_raw, uint32_t *d_info, void *d_work,
                           const EdgestatPlan &p, hipStream_t s, uint32_t cross, unsigned steps = 15) {
    const uint32_t B = t->B;
    char *w = (char *)d_work;
    u64 *clade = (u64 *)(w + p.clade_at);
    double *P0 = (double *)(w + p.p0_at), *P1 = (double *)(w + p.p1_at), *gc = (double *)(w + p.gc_at);
    int *gd = (int *)(w + p.gd_at);
    u32 *active = (u32 *)(w + p.active_at);
    const u64 W = (u64)rk_masses_words(B);
    const bool sort = S > cross;
    uint32_t N = 1;  // the sorted keys: S rounded up to a power of two
    while (N < S) N <<= 1;
    if (steps & 1) {
        hipLaunchKernelGGL(clade_masses_kernel, dim3(S), dim3(256), 0, s, B, W, t->node_at, t->end_at, t->span_node, t->span_end, t->span_off, (const u64 *)d_masses, clade);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 2) {
        hipLaunchKernelGGL(edgestat_profiles_kernel, dim3((B + 31) / 32, (S + 31) / 32), dim3(256), 0, s, B, S, W, t->root, (const u64 *)d_masses, (const u64 *)clade, P0, P1);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 4) {
        hipLaunchKernelGGL(edgestat_init_kernel, dim3(1), dim3(256), 0, s, B, S, F, t->root, (const u64 *)clade, d_meta, active, (u32 *)d_info);
        if (F)
            hipLaunchKernelGGL(edgestat_column_kernel, dim3(F), dim3(EDGESTAT_THREADS), (size_t)(sort ? N : S) * 8, s, B, S, F, N, sort ? 1u : 0u, (const u32 *)d_info,
                               (const u32 *)active, d_meta, gc, gd, (u64 *)d_raw);
        HIP_TRY(hipGetLastError());
    }
    if (steps & 8) {
        if (sort)
            hipLaunchKernelGGL(edgestat_edge_kernel<true>, dim3(2 * B), dim3(EDGESTAT_THREADS), (size_t)N * 8, s, B, S, F, N, (const u32 *)d_info, (const u32 *)active,
                               (const double *)P0, (const double *)P1, (const double *)gc, (const int *)gd, (u64 *)d_raw);
        else
            hipLaunchKernelGGL(edgestat_edge_kernel<false>, dim3((2 * B + EDGESTAT_WAVES - 1) / EDGESTAT_WAVES), dim3(EDGESTAT_THREADS), (size_t)EDGESTAT_WAVES * S * 8, s, B, S,
                               F, N, (const u32 *)d_info, (const u32 *)active, (const double *)P0, (const double *)P1, (const double *)gc, (const int *)gd, (u64 *)d_raw);
        HIP_TRY(hipGetLastError());
    }
    return RK_OK;
}

extern "C" int rk_edgestat_device(const rk_tree *t, uint32_t n_samples, const uint64_t *d_masses, uint32_t n_features, const double *d_meta, uint64_t *d_raw,
                                  uint32_t *d_info, void *d_work, uint64_t work_bytes, void *stream) {
    const char *who = "rk_edgestat_device";
    EdgestatPlan p;
    if (int rc = edgestat_prepare(who, t, n_samples, n_features, p)) return rc;
    if (!d_masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    if (n_features && !d_meta) return fail(RK_ERR_INVALID, "%s: null metadata with n_features=%u", who, n_features);
    if (!d_raw || !d_info) return fail(RK_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d_raw % 8 || (uintptr_t)d_meta % 8 || (uintptr_t)d_info % 4)
        return fail(RK_ERR_INVALID, "%s: the raw output and the metadata must be 8-byte aligned, the info words 4-byte aligned", who);
    if (int rc = work_args(who, "rk_edgestat_work_bytes", d_work, work_bytes, p.bytes)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    unsigned steps = 15;
    uint32_t cross = RK_EDGESTAT_COUNT_MAX_SAMPLES;
    if (const char *v = rk_knob("RK_EDGESTAT_STEPS")) steps = (unsigned)atoi(v);  // developer builds (scripts/edgestat_rate.py)
    if (const char *v = rk_knob("RK_EDGESTAT_COUNT_MAX")) cross = std::min<uint32_t>((uint32_t)atoi(v), EDGESTAT_COUNT_LIMIT);  // developer builds: both forms on one shape
    return edgestat_launch(t, n_samples, d_masses, n_features, d_meta, d_raw, d_info, d_work, p, (hipStream_t)stream, cross, steps);
}

extern "C" int rk_edgestat_host(uint32_t n_branches, const int32_t *parent, uint32_t n_samples, const uint64_t *masses, uint32_t n_features, const double *meta,
                                uint64_t *raw, uint32_t *info, uint32_t n_threads) {
    const char *who = "rk_edgestat_host";
    RK_GUARD_BEGIN
    if (int rc = edgestat_range(who, n_samples, n_features)) return rc;
    if (n_features && !meta) return fail(RK_ERR_INVALID, "%s: null metadata with n_features=%u", who, n_features);
    if (!raw || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, nullptr, false, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    if (!masses) return fail(RK_ERR_INVALID, "%s: null mass buffer", who);
    const uint64_t B = n_branches, S = n_samples, W = rk_masses_words(n_branches);
    std::vector<uint64_t> clade(S * B);
    uint64_t T = host_threads(n_threads, S);
    int rc = masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        for (uint64_t s = th; s < S; s += T) rk::clade_masses_sample(w, parent, masses + s * W, clade.data() + s * B);
    });
    if (rc) return rc;
    std::vector<uint8_t> active(S);
    uint32_t n = 0;
    for (uint64_t s = 0; s < S; s++) n += active[s] = clade[s * B + w.root] != 0;
    const uint64_t n_out = rk::edgestat_out_words(n_branches, n_features);
    info[0] = n;
    info[1] = 0;
    if (n == 0) {
        for (uint64_t i = 0; i < n_out; i++) raw[i] = 0;
        return RK_OK;
    }
    rk::EdgestatColumns col;
    rk::edgestat_columns(n_samples, n, n_features, active.data(), meta, col, raw + B * rk::edgestat_row_words(n_features));
    info[1] = col.unusable;
    // edges dealt round to the threads
    T = host_threads(n_threads, B);
    return masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        rk::edgestat_edges(n_branches, n_samples, W, w.root, n, n_features, active.data(), masses, clade.data(), col, (uint32_t)th, (uint32_t)T, raw);
    });
    RK_GUARD_END(who)
}

// The drivers' call: as rk_epca_batch, with the metadata uploaded behind the outputs; a value that is not finite is refused here
extern "C" int rk_edgestat_batch(rk_db *db, const rk_tree *t, uint32_t n_samples, const uint64_t *masses, uint32_t n_features, const double *meta, uint64_t *raw,
                                 uint32_t *info) {
    const char *who = "rk_edgestat_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    EdgestatPlan p;
    if (int rc = edgestat_prepare(who, t, n_samples, n_features, p)) return rc;
    if (n_features && !meta) return fail(RK_ERR_INVALID, "%s: null metadata with n_features=%u", who, n_features);
    if (!raw || !info) return fail(RK_ERR_INVALID, "%s: null output", who);
    for (uint64_t i = 0; i < (uint64_t)n_features * n_samples; i++)
        if (!std::isfinite(meta[i]))
            return fail(RK_ERR_INVALID, "%s: metadata column %u of sample %u is not finite", who, (uint32_t)(i / n_samples), (uint32_t)(i % n_samples));
    const uint64_t raw_bytes = rk::edgestat_out_words(t->B, n_features) * 8, meta_bytes = (uint64_t)n_features * n_samples * 8;  // raw | meta | info
    return samples_batch(who, db, n_samples, masses, p.bytes, raw_bytes + meta_bytes + 8, [&](const uint64_t *d_masses, char *d_out, void *d_work, hipStream_t s) -> int {
        double *d_meta = (double *)(d_out + raw_bytes);
        uint32_t *d_info = (uint32_t *)(d_out + raw_bytes + meta_bytes);
        if (meta_bytes) HIP_TRY(hipMemcpyAsync(d_meta, meta, meta_bytes, hipMemcpyHostToDevice, s));
        if (int rc = rk_edgestat_device(t, n_samples, d_masses, n_features, n_features ? d_meta : nullptr, (uint64_t *)d_out, d_info, d_work, p.bytes, s)) return rc;
        HIP_TRY(hipMemcpyAsync(raw, d_out, raw_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(info, d_info, 8, hipMemcpyDeviceToHost, s));
        return RK_OK;
    });
}

extern "C" int rk_edgestat_finish_host(uint32_t n_branches, uint32_t n_samples, uint32_t n_features, const uint64_t *raw, const uint32_t *info, double *table,
                                       double *feature_table) {
    const char *who = "rk_edgestat_finish_host";
    if (!rk_edgestat_out_words(n_branches, n_features)) return fail(RK_ERR_INVALID, "%s: n_branches=%u, n_features=%u: out of 1..65535, 0..%u", who, n_branches, n_features, RK_EDGESTAT_MAX_FEATURES);
    if (int rc = edgestat_range(who, n_samples, n_features)) return rc;
    if (!raw || !info) return fail(RK_ERR_INVALID, "%s: null raw output", who);
    if (!table || (n_features && !feature_table)) return fail(RK_ERR_INVALID, "%s: null output", who);
    if (info[0] > n_samples) return fail(RK_ERR_INVALID, "%s: info says %u active samples of %u", who, info[0], n_samples);
    rk::edgestat_finish(n_branches, n_features, raw, info, table, feature_table);
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// EDPL: rk_edpl_lds_bytes / rk_edpl_device / _host / _batch and rk_tree_distance_host.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(EdplEntry) == 16 && sizeof(rk::EdplNode) == 16 && offsetof(EdplEntry, pre) == 8 && offsetof(rk::EdplNode, pre) == 8 &&
                  offsetof(EdplEntry, end) == 12 && offsetof(rk::EdplNode, end) == 12,
              "one entry layout for the host's builder and the kernel");
static_assert(RK_EDPL_MAX_KEEP == rk::EDPL_MAX_K, "one limit for the header and the host twin");
// The tables of a tree go into the LDS of every block while they take at most this many bytes: behind them the 160 KB of a CU still
// hold the stages of four waves at K = 16 (87 040 bytes) and of ten at K = 7 (8 960 bytes each).
constexpr uint64_t RK_EDPL_LDS_MAX_BYTES = 65536;
constexpr uint64_t RK_EDPL_CU_LDS_BYTES = 160 * 1024;
constexpr uint32_t RK_EDPL_GLOBAL_WAVES = 4;          // without the tables: blocks of four waves, as many a CU as their stages allow
constexpr uint32_t RK_EDPL_GLOBAL_BLOCKS_PER_CU = 8;
constexpr uint64_t RK_EDPL_CHUNK_READS = 1ull << 22;  // rk_edpl_batch: reads a chunk (at K = 7, 75 MB up and 32 MB down)

// the rule that picks the form: the byte size of the tables against the limit (developer builds move the limit)
static bool edpl_tables_in_lds(const rk_tree *t) {
    uint64_t limit = RK_EDPL_LDS_MAX_BYTES;
    if (const char *v = rk_knob("RK_EDPL_LDS_BYTES")) limit = strtoull(v, nullptr, 10);  // developer builds: both forms on one small tree
    limit = std::min<uint64_t>(limit, RK_EDPL_CU_LDS_BYTES - RK_EDPL_GLOBAL_WAVES * edpl_stage_bytes(RK_EDPL_MAX_KEEP));  // (four waves' stages fit at any K)
    return (uint64_t)t->lca_words * 8 <= limit;
}

extern "C" uint64_t rk_edpl_lds_bytes(const rk_tree *t) {
    if (!t) {
        (void)fail(RK_ERR_INVALID, "rk_edpl_lds_bytes: null tree");
        return 0;
    }
    return edpl_tables_in_lds(t) ? (uint64_t)t->lca_words * 8 : 0;
}

// the tests of the three calls that read a result set, with the rules of masses_args
static int edpl_args(const char *who, uint32_t K, uint64_t n_reads, const rk_result *res, const double *edpl) {
    if (K < 1 || K > RK_EDPL_MAX_KEEP) return fail(RK_ERR_INVALID, "%s: keep_at_most=%u outside 1..16", who, K);
    if (n_reads >= (1ull << 32)) return fail(RK_ERR_INVALID, "%s: n_reads=%llu, at most 2^32 - 1 per call", who, (unsigned long long)n_reads);
    if (n_reads == 0) return RK_OK;
    if (!res || !res->n_rows || !res->branch || !res->lwr) return fail(RK_ERR_INVALID, "%s: null result array (n_rows, branch and lwr are read)", who);
    if (!edpl) return fail(RK_ERR_INVALID, "%s: null output", who);
    return RK_OK;
}

extern "C" int rk_edpl_device(const rk_tree *t, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_res, double *d_edpl, void *stream) {
    const char *who = "rk_edpl_device";
    if (!t) return fail(RK_ERR_INVALID, "%s: null tree", who);
    int rc = edpl_args(who, keep_at_most, n_reads, d_res, d_edpl);
    if (rc || n_reads == 0) return rc;
    HIP_TRY(hipSetDevice(t->device));
    // with the tables: one block a CU, of the waves whose stages fit behind them (at least four: the limit leaves room for them at
    // any K); without: blocks of four waves, a grid of as many a CU as their stages allow
    const bool lds = edpl_tables_in_lds(t);
    const uint64_t stage = edpl_stage_bytes(keep_at_most), tables = lds ? (uint64_t)t->lca_words * 8 : 0;
    const uint32_t waves = lds ? (uint32_t)std::min<uint64_t>((RK_EDPL_CU_LDS_BYTES - tables) / stage, EDPL_MAX_WAVES) : RK_EDPL_GLOBAL_WAVES;
    const uint64_t tiles = (n_reads + 64 * waves - 1) / (64 * waves);
    const uint64_t per_cu = lds ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(RK_EDPL_CU_LDS_BYTES / (waves * stage), RK_EDPL_GLOBAL_BLOCKS_PER_CU));
    const unsigned blocks = (unsigned)std::min<uint64_t>(tiles, (uint64_t)t->cu_count * per_cu);
    const size_t lds_bytes = (size_t)(tables + waves * stage);
    auto launch = [&](auto kernel) -> int {
        HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * waves), lds_bytes, (hipStream_t)stream, (u64)n_reads, keep_at_most, t->B, t->lca_words,
                           (const unsigned char *)d_res->n_rows, (const unsigned short *)d_res->branch, (const double *)d_res->lwr, t->node, t->lca, d_edpl);
        HIP_TRY(hipGetLastError());
        return RK_OK;
    };
    return lds ? launch(edpl_kernel<true>) : launch(edpl_kernel<false>);
}

extern "C" int rk_edpl_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res,
                            double *edpl, uint32_t n_threads) {
    const char *who = "rk_edpl_host";
    RK_GUARD_BEGIN
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, branch_len, true, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    int rc = edpl_args(who, keep_at_most, n_reads, res, edpl);
    if (rc || n_reads == 0) return rc;
    rk::TreeDist dist;
    rk::tree_dist_build(w, parent, branch_len, dist);
    const uint64_t T = host_threads(n_threads, (n_reads + 4095) / 4096);
    return masses_fan_out(who, T, 0, false, nullptr, [&](uint64_t th, uint64_t *) {
        rk::edpl_range(dist, keep_at_most, n_reads * th / T, n_reads * (th + 1) / T, res->n_rows, res->branch, res->lwr, edpl);
    });
    RK_GUARD_END(who)
}

extern "C" int rk_tree_distance_host(uint32_t n_branches, const int32_t *parent, const float *branch_len, uint32_t n_pairs, const uint16_t *a, const uint16_t *b,
                                     double *d) {
    const char *who = "rk_tree_distance_host";
    RK_GUARD_BEGIN
    rk::TreeWalk w;
    if (rk::tree_walk(who, n_branches, parent, branch_len, true, w, g_err, sizeof(g_err))) return RK_ERR_INVALID;
    if (n_pairs == 0) return RK_OK;
    if (!a || !b) return fail(RK_ERR_INVALID, "%s: null branch array", who);
    if (!d) return fail(RK_ERR_INVALID, "%s: null output", who);
    for (uint32_t i = 0; i < n_pairs; i++)
        if (a[i] >= n_branches || b[i] >= n_branches) return fail(RK_ERR_INVALID, "%s: pair %u is (%u, %u), the tree has %u branches", who, i, a[i], b[i], n_branches);
    rk::TreeDist dist;
    rk::tree_dist_build(w, parent, branch_len, dist);
    for (uint32_t i = 0; i < n_pairs; i++) d[i] = rk::tree_distance(dist.node[a[i]], dist.node[b[i]], dist.B, dist.dpar(), dist.depth(), dist.table());
    return RK_OK;
    RK_GUARD_END(who)
}

// The drivers' call: a result set on the host in, one double a read on the host out, in chunks through rk_edpl_device on db's device.
// Only n_rows, branch and lwr are uploaded; the buffers are allocated for the call and freed; it waits for the result.
extern "C" int rk_edpl_batch(rk_db *db, const rk_tree *t, uint32_t keep_at_most, uint64_t n_reads, const rk_result *res, double *edpl) {
    const char *who = "rk_edpl_batch";
    if (int rc = batch_handles(who, db, t)) return rc;
    int rc = edpl_args(who, keep_at_most, n_reads, res, edpl);
    if (rc || n_reads == 0) return rc;
    std::lock_guard<std::mutex> lock(db->host_mutex);
    hipStream_t s;
    if (int e = batch_stream(db, s)) return e;
    const uint64_t K = keep_at_most, chunk = std::min<uint64_t>(n_reads, RK_EDPL_CHUNK_READS);
    BatchBufs b;
    GrowBuf &d_in = b.in, &d_out = b.out;
    const uint64_t branch_at = up256(chunk), lwr_at = branch_at + up256(chunk * K * 2);  // n_rows | branch | lwr
    if (int e = d_in.reserve(lwr_at + chunk * K * 8)) return e;
    if (int e = d_out.reserve(chunk * 8)) return e;
    char *base = (char *)d_in.p;
    const rk_result d_res{(uint8_t *)base, (uint16_t *)(base + branch_at), nullptr, (double *)(base + lwr_at), nullptr};
    for (uint64_t r0 = 0; r0 < n_reads; r0 += chunk) {  // (one stream: a chunk's uploads wait for the kernel of the chunk before)
        const uint64_t n = std::min(chunk, n_reads - r0);
        HIP_TRY(hipMemcpyAsync(d_res.n_rows, res->n_rows + r0, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_res.branch, res->branch + r0 * K, n * K * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_res.lwr, res->lwr + r0 * K, n * K * 8, hipMemcpyHostToDevice, s));
        if (int e = rk_edpl_device(t, keep_at_most, n, &d_res, d_out.as<double>(), s)) return e;
        HIP_TRY(hipMemcpyAsync(edpl + r0, d_out.p, n * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return RK_OK;
}
