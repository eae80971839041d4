// rk_synth_impl.h -- the seeded synthetic phylo-kmer database of SURVEY.md section 8(d), generated straight into the
// HBM image (included at the end of rk_engine.hip), and rk_db_fetch_row (a row read back out of the image).
//
// Why it lives in the library: BASELINE config C5 is a ~200 GB database (3.3e10 entries).  It cannot pass through
// rk_db_create's host arrays (the image plus its CSR source would not fit next to each other anywhere), so the image is
// filled by a kernel from a counter-based generator: every quantity is a pure function of (seed, dense k-mer index,
// entry index), integer arithmetic except one float32 multiply, so that a checker can regenerate any row on the host
// (rappas_amd/synth.py: synth_rows) and hand it to the oracle.
//
//   mix(x)      splitmix64 finaliser
//   h0          mix(seed + (dense + 1) * 0x9E3779B97F4A7C15)
//   present     (h0 >> 32) < floor(key_fraction * 2^32)
//   len         1 + #{ j in [1, max_len) : surv[j] > (mix(h0 ^ 0xA0761D6478BD642F) >> 32) },  max_len = max(1, n_branches - 1),
//               surv[0] = 2^32, surv[j] = (surv[j-1] * q) >> 32, q = floor((1 - 1/mean_row_len) * 2^32)   (1 + geometric)
//   b0          1 + (((mix(h0 ^ 0xE7037ED1A0B428DB) >> 32) * max(1, n_branches - len)) >> 32)   (0 when n_branches == 1)
//   entry i     branch b0 + i,  score = T * ((mix(h0 + (i + 1) * 0xD6E8FEB86659FD93) >> 40) * 2^-24)   (float32, T <= v <= 0)
#pragma once

namespace rk {

struct SynthParams {
    u64 seed, key_thresh;
    const u64 *surv;  // [surv_n], non-increasing
    u32 surv_n;
    u32 n_branches, max_len;
    float T;
};

__host__ __device__ __forceinline__ u64 synth_mix(u64 x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
__host__ __device__ __forceinline__ u64 synth_h0(u64 seed, u64 dense) { return synth_mix(seed + (dense + 1) * 0x9E3779B97F4A7C15ull); }
__host__ __device__ __forceinline__ u32 synth_len(const SynthParams &sp, u64 h0) {
    const u64 r = synth_mix(h0 ^ 0xA0761D6478BD642Full) >> 32;
    // first j in [1, surv_n) with surv[j] <= r (surv is non-increasing); all j below it count
    u32 lo = 1, hi = sp.surv_n;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (sp.surv[mid] > r) lo = mid + 1; else hi = mid;
    }
    const u32 len = lo;  // 1 + (lo - 1)
    return len < sp.max_len ? len : sp.max_len;
}
__host__ __device__ __forceinline__ u32 synth_b0(const SynthParams &sp, u64 h0, u32 len) {
    if (sp.n_branches == 1) return 0;
    const u64 hi = sp.n_branches > len ? sp.n_branches - len : 1;
    return 1u + (u32)(((synth_mix(h0 ^ 0xE7037ED1A0B428DBull) >> 32) * hi) >> 32);
}
__host__ __device__ __forceinline__ float synth_score(const SynthParams &sp, u64 h0, u32 i) {
    const u64 hs = synth_mix(h0 + (u64)(i + 1) * 0xD6E8FEB86659FD93ull);
    const float u = (float)(u32)(hs >> 40) * 5.9604644775390625e-08f;  // 24 random bits * 2^-24: exact
    return sp.T * u;
}

// one workgroup per row (grid-stride): INDEXED = the large-tree image (index line | u16 branch[lenp] | f32 score[lenp]),
// else 128-byte units of {slot offset, score} entries
template <bool INDEXED>
__global__ void __launch_bounds__(256) synth_fill_kernel(SynthParams sp, u64 n_keys, const u64 *dense, const u64 *desc,
                                                         unsigned char *rows) {
    for (u64 r = blockIdx.x; r < n_keys; r += gridDim.x) {
        const u64 h0 = synth_h0(sp.seed, dense[r]);
        const u32 len = synth_len(sp, h0);
        const u32 b0 = synth_b0(sp, h0, len);
        const u64 d = desc[r];
        const u32 lenp = (u32)d & DESC_LEN_MASK;
        unsigned char *row = rows + ((d >> DESC_LEN_BITS) << 3);
        if (INDEXED) {
            unsigned short *bp = (unsigned short *)row;
            float *scp = (float *)(row + 2 * (size_t)lenp);
            if (threadIdx.x < 32) {
                const u32 i = threadIdx.x + 1;
                const u32 bound = index_bound(i, sp.n_branches);
                const u32 below = bound > b0 ? bound - b0 : 0u;  // entries with branch < bound
                ((unsigned short *)(row - 64))[threadIdx.x] = (unsigned short)(below < len ? below : len);
            }
            for (u32 i = threadIdx.x; i < lenp; i += blockDim.x) {
                bp[i] = i < len ? (unsigned short)(b0 + i) : RAW_PAD_BRANCH;
                scp[i] = i < len ? synth_score(sp, h0, i) : RAW_PAD_SCORE;
            }
        } else {
            Entry *ep = (Entry *)row;
            for (u32 i = threadIdx.x; i < lenp; i += blockDim.x) ep[i] = i < len ? Entry{slot_offset(b0 + i), synth_score(sp, h0, i)} : slot_padding();
        }
    }
}

// one wave: the row of `code` as the placement kernels would see it (table lookup + entry decode)
template <int BITS, int TM>
__global__ void __launch_bounds__(64) fetch_row_kernel(DbView db, u64 code, u32 cap, u32 *out_len, unsigned short *out_br, float *out_sc) {
    const u32 lane = threadIdx.x;
    const u64 desc = lookup_desc<BITS, TM>(db, code);
    const u32 lenp = (u32)desc & DESC_LEN_MASK;
    u32 mine = 0;
    for (u32 e = lane; e < lenp; e += 64) {
        u32 br;
        float sc;
        load_entry(db, desc, e, br, sc);
        if (br == 0xFFFFu) continue;  // padding (only ever trails the row)
        mine++;
        if (e < cap) { out_br[e] = (unsigned short)br; out_sc[e] = sc; }
    }
    if (mine) atomicAdd(out_len, mine);
}

}  // namespace rk

namespace {
struct DevBufS {
    void *p = nullptr;
    ~DevBufS() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" int rk_db_create_synth(const rk_synth_desc *d, rk_db **out) {
    RK_GUARD_BEGIN
    static const char *const who = "rk_db_create_synth";
    if (!d || !out) return fail(RK_ERR_INVALID, "rk_db_create_synth: null argument");
    *out = nullptr;
    if (int rc = image_error(rk_image::check_scalars(d->alphabet, d->k, d->n_branches, d->thr_log10, d->thr), who, d->alphabet, d->k, d->n_branches, d->table_mode)) return rc;
    if (!(d->key_fraction > 0.0 && d->key_fraction <= 1.0)) return fail(RK_ERR_INVALID, "rk_db_create_synth: key_fraction must be in (0, 1]");
    if (!(d->mean_row_len >= 1.0 && d->mean_row_len <= 65535.0)) return fail(RK_ERR_INVALID, "rk_db_create_synth: mean_row_len must be in [1, 65535]");
    const rk_image::TableMode tm = rk_image::resolve_table_mode(d->table_mode, d->alphabet, d->k, 1ull << 32);
    if (!tm.space_ok) return fail(RK_ERR_UNSUPPORTED, "rk_db_create_synth: sigma^k must be <= 2^32 (every code is visited once)");
    if (int rc = image_error(tm.status, who, d->alphabet, d->k, d->n_branches, tm.mode)) return rc;
    const uint64_t space = tm.space;
    ImageShape shape;
    shape.alphabet = d->alphabet; shape.convert_uo = d->convert_uo; shape.k = d->k; shape.n_branches = d->n_branches;
    shape.thr_log10 = d->thr_log10; shape.thr = d->thr;
    shape.bits = rk_image::bits_of(d->alphabet); shape.mode = tm.mode;
    shape.mono = d->thr_log10 <= 0.0f;  // (scores are T * u, 0 <= u < 1)

    // ---- generator tables ----
    SynthParams sp{};
    sp.seed = d->seed;
    sp.key_thresh = (uint64_t)(d->key_fraction * 4294967296.0);
    sp.n_branches = d->n_branches;
    sp.max_len = d->n_branches > 1 ? d->n_branches - 1 : 1;
    sp.T = d->thr_log10;
    std::vector<u64> surv;
    {
        const double p = 1.0 / d->mean_row_len;
        const uint64_t q = (uint64_t)((1.0 - p) * 4294967296.0);
        surv.push_back(1ull << 32);
        while (surv.size() < sp.max_len && surv.back() != 0) surv.push_back((surv.back() * q) >> 32);
    }
    sp.surv = surv.data();
    sp.surv_n = (uint32_t)surv.size();

    // The pass below writes a row's window span as it meets the row, so the window width is needed before a row is drawn: the plan is
    // asked with the spec's density here, and plan_kind below, given the same density, keeps or drops these very windows
    const rk_image::RowDensity density = rk_image::spec_density((double)sp.key_thresh / 4294967296.0, d->mean_row_len);
    WindowPlan wp;
    const bool may_window = rk_geom::window_plan(d->n_branches, shape.bits, density.units_per_code, density.units_per_row, geom_knobs(), wp);
    std::vector<unsigned char> winspec;  // [space] winspec_byte(first, last window) of every row (rows are branch runs)
    if (may_window) winspec.assign(space, 0);
    // ---- pass 1 (host): which codes carry a row and how long it is; rows are laid out in dense order ----
    std::vector<u64> dense, lens32;  // lens32: row length per present key (u64: they become the descriptors below)
    {
        unsigned hw = std::thread::hardware_concurrency();
        const unsigned T = space > (1u << 20) ? std::max(1u, std::min(hw ? hw : 1u, 16u)) : 1u;
        std::vector<std::vector<u64>> dpart(T), lpart(T);
        std::vector<std::thread> th;
        bool oom = false;
        for (unsigned t = 0; t < T; t++) {
            auto job = [&, t]() {
                try {
                    const uint64_t lo = space * t / T, hi = space * (t + 1) / T;
                    for (uint64_t c = lo; c < hi; c++) {
                        const uint64_t h0 = synth_h0(sp.seed, c);
                        if ((h0 >> 32) >= sp.key_thresh) continue;
                        const u32 len = synth_len(sp, h0);
                        dpart[t].push_back(c);
                        lpart[t].push_back(len);
                        if (may_window) {
                            const u32 b0 = synth_b0(sp, h0, len), f = b0 / wp.W, l = (b0 + len - 1) / wp.W;
                            winspec[c] = winspec_byte(f, l);
                        }
                    }
                } catch (const std::bad_alloc &) { oom = true; }
            };
            if (t + 1 < T) th.emplace_back(job); else job();
        }
        for (std::thread &x : th) x.join();
        if (oom) return fail(RK_ERR_NOMEM, "rk_db_create_synth: host OOM");
        for (unsigned t = 0; t < T; t++) {
            dense.insert(dense.end(), dpart[t].begin(), dpart[t].end());
            lens32.insert(lens32.end(), lpart[t].begin(), lpart[t].end());
            std::vector<u64>().swap(dpart[t]);
            std::vector<u64>().swap(lpart[t]);
        }
    }
    // ---- the plan: kind of image (no position keys in a generated image), row layout, table ----
    const uint64_t n_keys = dense.size();
    rk_image::RowStats rs;
    for (uint64_t i = 0; i < n_keys; i++) rs.add(lens32[i]);
    shape.n_keys = n_keys; shape.n_entries = rs.n_entries;
    const rk_image::KindPlan kind = rk_image::plan_kind(d->n_branches, shape.bits, tm, rs, density, false, geom_knobs());
    rk_image::RowLayout lay(kind.indexed);
    std::vector<u64> &desc = lens32;  // lengths become descriptors in place
    for (uint64_t i = 0; i < n_keys; i++) desc[i] = lay.add_row(lens32[i]);
    if (int rc = image_error(lay.finish(), who, d->alphabet, d->k, d->n_branches, tm.mode)) return rc;
    std::vector<uint64_t> table;
    rk_image::build_table(shape, space, lay, [&](uint64_t i) { return dense[i]; }, [&](uint64_t i) { return desc[i]; },
                          [&](uint64_t i) { return rk_image::code_of_dense(shape.bits, d->k, dense[i]); }, image_knobs(), table);
    rk_image::finish_shape(shape, lay, kind, table.size(), rs.longest, space);

    // ---- device: table and window spans uploaded, the rows filled by a kernel from the generator's tables ----
    const bool indexed = lay.indexed;
    DevBufS d_dense, d_desc, d_surv;  // (freed after install has synchronised)
    return install(shape, d->device, [&](const rk_db &db, int sec, void *dst, uint64_t bytes) -> int {
        if (sec != IMG_ROWS) {
            if (bytes) HIP_TRY(hipMemcpy(dst, sec == IMG_TABLE ? (const void *)table.data() : (const void *)winspec.data(), bytes, hipMemcpyHostToDevice));
            return RK_OK;
        }
        HIP_TRY(hipMemset(dst, indexed ? 0xFF : 0, lay.unit_bytes));  // unit 0: the reserved "skip" / scratch pattern
        if (!n_keys) return RK_OK;
        HIP_TRY(hipMalloc(&d_dense.p, n_keys * 8));
        HIP_TRY(hipMalloc(&d_desc.p, n_keys * 8));
        HIP_TRY(hipMalloc(&d_surv.p, surv.size() * 8));
        HIP_TRY(hipMemcpy(d_dense.p, dense.data(), n_keys * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_desc.p, desc.data(), n_keys * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_surv.p, surv.data(), surv.size() * 8, hipMemcpyHostToDevice));
        SynthParams dsp = sp;
        dsp.surv = (const u64 *)d_surv.p;
        uint64_t blocks = (uint64_t)db.cu_count * 16;
        if (blocks > n_keys) blocks = n_keys;
        if (indexed)
            hipLaunchKernelGGL(synth_fill_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, 0, dsp, (u64)n_keys, (const u64 *)d_dense.p,
                               (const u64 *)d_desc.p, (unsigned char *)dst);
        else
            hipLaunchKernelGGL(synth_fill_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, 0, dsp, (u64)n_keys, (const u64 *)d_dense.p,
                               (const u64 *)d_desc.p, (unsigned char *)dst);
        HIP_TRY(hipGetLastError());
        return RK_OK;
    }, out);
    RK_GUARD_END("rk_db_create_synth")
}

template <int BITS>
static void launch_fetch(const rk_db *db, u64 code, u32 cap, u32 *d_len, unsigned short *d_br, float *d_sc) {
    switch (db->info.table_mode) {
    case RK_TABLE_DIRECT: hipLaunchKernelGGL((fetch_row_kernel<BITS, TM_COMPACT>), dim3(1), dim3(64), 0, 0, db->view, code, cap, d_len, d_br, d_sc); break;
    case RK_TABLE_DIRECT8: hipLaunchKernelGGL((fetch_row_kernel<BITS, TM_DIRECT8>), dim3(1), dim3(64), 0, 0, db->view, code, cap, d_len, d_br, d_sc); break;
    default: hipLaunchKernelGGL((fetch_row_kernel<BITS, TM_HASH>), dim3(1), dim3(64), 0, 0, db->view, code, cap, d_len, d_br, d_sc); break;
    }
}

extern "C" int rk_db_fetch_row(rk_db *db, uint64_t code, uint32_t cap, uint32_t *len, uint16_t *branch_ids, float *scores) {
    if (!db || !len) return fail(RK_ERR_INVALID, "rk_db_fetch_row: null argument");
    if (cap && (!branch_ids || !scores)) return fail(RK_ERR_INVALID, "rk_db_fetch_row: null output arrays");
    const uint32_t bits = db->info.bits_per_symbol;
    uint64_t dense;
    if (!rk_image::code_in_space(bits, db->info.k, code)) return fail(RK_ERR_INVALID, "rk_db_fetch_row: code outside the k-mer space");
    if (bits == 5 && !rk_image::aa_dense_of_code(code, db->info.k, dense)) return fail(RK_ERR_INVALID, "rk_db_fetch_row: code has a digit >= 20");
    int prev = 0;
    (void)hipGetDevice(&prev);
    struct Restore { int p; ~Restore() { (void)hipSetDevice(p); } } restore{prev};
    HIP_TRY(hipSetDevice(db->info.device));
    DevBufS d_len, d_br, d_sc;
    HIP_TRY(hipMalloc(&d_len.p, 4));
    HIP_TRY(hipMalloc(&d_br.p, (size_t)(cap ? cap : 1) * 2));
    HIP_TRY(hipMalloc(&d_sc.p, (size_t)(cap ? cap : 1) * 4));
    HIP_TRY(hipMemset(d_len.p, 0, 4));
    if (bits == 2) launch_fetch<2>(db, code, cap, (u32 *)d_len.p, (unsigned short *)d_br.p, (float *)d_sc.p);
    else launch_fetch<5>(db, code, cap, (u32 *)d_len.p, (unsigned short *)d_br.p, (float *)d_sc.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(len, d_len.p, 4, hipMemcpyDeviceToHost));
    const uint32_t n = *len < cap ? *len : cap;
    if (n) {
        HIP_TRY(hipMemcpy(branch_ids, d_br.p, (size_t)n * 2, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(scores, d_sc.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return RK_OK;
}
