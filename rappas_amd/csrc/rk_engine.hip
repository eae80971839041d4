// rk_engine.hip -- host side of the placement engine: DB image construction (open-addressed / direct table
// + CSR row blob resident in HBM), launch geometry, and the C ABI of include/rappas_place.h.
// Product path: there is NO CPU fallback in this file; every compute entry point needs a HIP device.
#include "rk_kernels.hip"
#include "rk_internal.h"
#include "rk_pack_host.h"
#include "rk_translate_host.h"
#include "rk_plan.h"
#include "rk_geometry.h"
#include "rk_image_plan.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <cerrno>
#include <cstddef>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <atomic>
#include <mutex>
#include <tuple>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>
#include <fstream>
#include <pthread.h>
#include <sched.h>

using namespace rk;

#ifndef RK_WG_RING
#define RK_WG_RING 20  // the same for the large-tree kernel, whose waves stream long row slices from HBM: what counts there is bytes in flight
                       // (C5s: rings of 8 / 12 / 16 / 20 / 24 / 32 give 0.72 / 0.76 / 0.77 / 0.79 / 0.78 / 0.77 of the byte roofline;
                       // C5 at 200 GB 0.61 -> 0.65, C5m 0.60 -> 0.63; short-row trees beyond 32 000 branches lose 7 %)
#endif
#ifndef RK_WRING
#define RK_WRING RK_RING  // the same for the windowed kernel
#endif
#ifndef RK_HRING
#define RK_HRING 2  // ... and for the hash-accumulator kernel (place_hash64_kernel: steps of RK_HNPL entries per lane = 4 * RK_HNPL row units)
#endif
#ifndef RK_HNPL
#define RK_HNPL 4
#endif

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace rk {
int fail_msg(int code, const char *fmt, ...) {  // rk_internal.h: the same sink for the other translation units
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace rk

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? RK_ERR_NOMEM : RK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                     \
    } while (0)

extern "C" const char *rk_last_error(void) { return g_err; }

// The placement kernels are launched as persistent grids: one block per slot a CU really has, every block walking the batch with
// the grid's stride.  The slots are what the runtime says fit (registers, the LDS allocation granule), not LDS size / LDS
// per block: a grid one block per CU too large runs a second round and costs up to 2 x (seen: 23 360 B of LDS per block, seven
// by division, six resident; 32-lane geometry with 11 by division, 8 by registers).
struct Grid {
    int threads; size_t lds;        // per block: threads and dynamic LDS
    uint64_t want_per_cu, work;     // blocks a CU holds by LDS size; blocks the batch has work for
    bool whole_simds = false;       // optional clamp: nine to eleven resident blocks become eight (launch_variant)
};
// One launch of a persistent grid on `stream`: nothing is allocated and nothing synchronises (stream capture keeps working); an empty
// grid launches nothing and asks the runtime nothing.
template <typename K, typename... Args>
static int launch_grid(int cu_count, K kern, const Grid &g, hipStream_t stream, const Args &...args) {
    if (g.work == 0) return RK_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    int n = 0;
    {  // (asked once per kernel, block size, LDS size and device: the query is not free next to a small launch)
        static std::mutex mu;
        static std::map<std::tuple<const void *, int, size_t, int>, int> known;
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        const auto key = std::make_tuple((const void *)kern, g.threads, g.lds, dev);
        std::lock_guard<std::mutex> lock(mu);
        auto it = known.find(key);
        if (it != known.end()) {
            n = it->second;
        } else {
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)kern, g.threads, g.lds));
            known.emplace(key, n);
        }
    }
    if (n < 1) return fail(RK_ERR_UNSUPPORTED, "internal: kernel does not fit a CU (%d threads, %zu B of LDS per block)", g.threads, g.lds);
    uint64_t per_cu = rk_geom::resident_per_cu(g.want_per_cu, (uint64_t)n, g.lds);
    static const bool trace = rk_knob("RK_TRACE_GRID") != nullptr;  // developer knob
    if (trace) fprintf(stderr, "[rk] grid: %d threads, %zu B LDS per block -> %d resident per CU (by LDS size %llu)\n", g.threads, g.lds, n, (unsigned long long)g.want_per_cu);
    if (g.whole_simds && per_cu > 8 && per_cu < 12) per_cu = 8;
    const uint64_t blocks = rk_geom::grid_blocks(cu_count, per_cu, g.work);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)g.threads), g.lds, stream, args...);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}
extern "C" int rk_version(void) { return RK_VERSION; }

// Main_DBBUILD_3.java:165-166
extern "C" void rk_thresholds(float omega, uint32_t n_states, uint32_t k, float *thr, float *thr_log10) {
    float ratio = omega / (float)n_states;
    float p = (float)std::pow(0.0 + (double)ratio, (double)k);
    if (thr) *thr = p;
    if (thr_log10) *thr_log10 = (float)std::log10((double)p);
}

// ------------------------------------------------------------------------------------------------
// alphabets (host tables uploaded with the DB)
// DNA: src/core/DNAStatesShifted.java:45-96 (ambiguity sets), :182-209 (states).
// AA : src/core/AAStates.java:23-28, :68-123.
// ------------------------------------------------------------------------------------------------
struct Alphabet {
    unsigned char table[256];      // state | 0x80|class | 0xFF
    unsigned char alts[16 * 20];   // alternatives per class
    unsigned char alt_count[16];
};

static void build_alphabet(uint32_t alphabet, bool convert_uo, Alphabet &A) {
    memset(A.table, 0xFF, sizeof(A.table));
    memset(A.alts, 0, sizeof(A.alts));
    memset(A.alt_count, 0, sizeof(A.alt_count));
    auto both = [&](char up, unsigned char v) {
        A.table[(unsigned char)up] = v;
        A.table[(unsigned char)(up + 32)] = v;
    };
    if (alphabet == RK_ALPHABET_DNA) {
        both('A', 0); both('T', 1); both('U', 1); both('C', 2); both('G', 3);
        const unsigned char a = 0, t = 1, c = 2, g = 3;
        struct { char ch; int n; unsigned char s[4]; } cls[] = {
            {'R', 2, {a, g}}, {'Y', 2, {c, t}}, {'S', 2, {c, g}}, {'W', 2, {a, t}}, {'K', 2, {g, t}},
            {'M', 2, {a, c}}, {'B', 3, {c, g, t}}, {'D', 3, {a, g, t}}, {'H', 3, {a, c, t}},
            {'V', 3, {a, c, g}}, {'N', 4, {a, c, g, t}},
        };
        int ci = 0;
        for (auto &e : cls) {
            both(e.ch, (unsigned char)(0x80 | ci));
            A.alt_count[ci] = (unsigned char)e.n;
            for (int i = 0; i < e.n; i++) A.alts[ci * 20 + i] = e.s[i];
            ci++;
        }
        // '.' and '-' : four never-filled (zero) alternatives
        A.table[(unsigned char)'.'] = A.table[(unsigned char)'-'] = (unsigned char)(0x80 | ci);
        A.alt_count[ci] = 4;
    } else {
        const char *order = "RHKDESTNQCGPAILMFWYV";
        for (int i = 0; i < 20; i++) both(order[i], (unsigned char)i);
        if (convert_uo) { both('U', 9); both('O', 14); }
        // class 0: any
        for (char ch : {'-', '*', '!', 'X', 'x'}) A.table[(unsigned char)ch] = 0x80;
        A.alt_count[0] = 20;
        for (int i = 0; i < 20; i++) A.alts[i] = (unsigned char)i;
        both('B', 0x81); A.alt_count[1] = 2; A.alts[20 + 0] = 3;  A.alts[20 + 1] = 7;
        both('Z', 0x82); A.alt_count[2] = 2; A.alts[40 + 0] = 4;  A.alts[40 + 1] = 8;
        both('J', 0x83); A.alt_count[3] = 2; A.alts[60 + 0] = 13; A.alts[60 + 1] = 14;
    }
}

// ------------------------------------------------------------------------------------------------
// DB object
// ------------------------------------------------------------------------------------------------
#include "rk_hostbuf_impl.h"

using namespace rk_geom;  // (its types and constants; its functions are called by their full names: the engine's own are db_geometry, db_wg_geometry)
static_assert(rk_geom::ROW_ENTRIES == ROW_UNIT, "rk_geometry.h repeats this constant of the device code");
static int knob_int(const char *name, int unset) {
    const char *e = rk_knob(name);
    return e ? atoi(e) : unset;
}
static rk_geom::Knobs geom_knobs() {  // (developer knobs, read where the geometry is asked for: the product library reads none)
    return {(uint32_t)knob_int("RK_LIST_CAP", 0), (uint32_t)knob_int("RK_WAVES_PER_CU", 0), knob_int("RK_WG_PASSES", 1), (uint32_t)knob_int("RK_HASH_WAVES", -1),
            rk_knob("RK_WINDOW_ALWAYS") != nullptr, rk_knob("RK_WSTREAM_ALWAYS") != nullptr};
}

using rk_image::ImageShape;  // (rk_image_plan.h: what an image is, apart from its bytes)
using rk_image::ipow_fits;
static_assert(rk_image::ROW_ENTRIES == ROW_UNIT && rk_image::DESC_LEN_BITS == DESC_LEN_BITS && rk_image::COMPACT_KMERS == COMPACT_KMERS,
              "rk_image_plan.h repeats these constants of the device code");
static rk_image::Knobs image_knobs() { return {rk_knob("RK_COMPACT_BYTES") != nullptr, rk_knob("RK_COMPACT_NIBBLES") != nullptr}; }  // (developer knobs, as geom_knobs)

static void info_of(const ImageShape &s, int device, rk_db_info *info) {
    memset(info, 0, sizeof(*info));
    info->alphabet = s.alphabet; info->k = s.k; info->n_branches = s.n_branches; info->table_mode = s.mode;
    info->thr_log10 = s.thr_log10; info->thr = s.thr; info->n_keys = s.n_keys; info->n_entries = s.n_entries;
    info->table_slots = s.slots; info->table_bytes = s.table_bytes; info->rows_bytes = s.rows_bytes;
    info->bits_per_symbol = s.bits; info->max_row_len = s.max_len; info->device = device;
}

struct rk_db {
    ImageShape shape;                  // what install() was given; info and view below are derived from it in finish_db
    rk_db_info info{};
    DbView view{};
    void *d_table = nullptr;
    void *d_rows = nullptr;
    unsigned char *d_alpha = nullptr;  // table[256] | alts[320] | alt_count[16]
    unsigned char *d_winspec = nullptr;  // [sigma^k] window span or position key per k-mer (shape.windowed || shape.has_pos)
    void *d_dense_table = nullptr;     // dense view (rk_device.h, ROW_UNIT24) for place_packed16_kernel, or nullptr: build_dense_view
    void *d_dense_rows = nullptr;
    uint64_t dense_rows_bytes = 0;
    uint32_t lanes_per_read = 0;       // 0 = auto
    int cu_count = 256;
    size_t lds_per_cu = 160 * 1024;
    hipStream_t stream = nullptr;      // spare stream
    std::mutex host_mutex;             // rk_place_batch (host path) owns the workspaces below
    rk_workspace ws[4];                // device buffers + stream per in-flight chunk (grow-only)
    GrowBuf d_masses;                  // the masses sink of the host path: 2 * B + 4 words the four streams add into,
    PinBuf h_masses;                   // and where they arrive on the host (allocated at the first profile-only call)
    uint32_t masses_samples = 0;       // the samples whose buffers the last profile-only call left in d_masses (0: one whole-batch buffer, or none)
    std::string kernel_name;
    // Scratch of the launches themselves (the tile order's keys / histogram / permutation, the marks of the tiles one kernel hands to
    // the next): one grow-only block per stream a caller has launched on, owned by the handle -- the library allocates from no pool
    // the hosting process shares and changes no attribute of one (launch_scratch)
    struct LaunchScratch { hipStream_t s; void *p; size_t cap; uint64_t used; };
    mutable std::mutex scratch_mu;
    mutable std::vector<LaunchScratch> scratch;
    mutable uint64_t scratch_clock = 0;
};

extern "C" void rk_db_destroy(rk_db *db) {
    if (!db) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(db->info.device);
    if (db->d_table) (void)hipFree(db->d_table);
    if (db->d_rows) (void)hipFree(db->d_rows);
    if (db->d_dense_table) (void)hipFree(db->d_dense_table);
    if (db->d_dense_rows) (void)hipFree(db->d_dense_rows);
    if (db->d_alpha) (void)hipFree(db->d_alpha);
    if (db->d_winspec) (void)hipFree(db->d_winspec);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    for (rk_workspace &w : db->ws) w.release();
    db->d_masses.release();
    db->h_masses.release();
    for (rk_db::LaunchScratch &b : db->scratch)
        if (b.p) (void)hipFree(b.p);
    if (prev >= 0) (void)hipSetDevice(prev);
    delete db;
}

// device selection, properties, spare stream and the alphabet tables of a handle whose shape and device are set; install() owns the
// handle and restores the current device
static int open_db(rk_db *db) {
    const int device = db->info.device;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    db->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    db->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? (size_t)prop.maxSharedMemoryPerMultiProcessor : 64 * 1024;
    HIP_TRY(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc((void **)&db->d_alpha, 256 + 320 + 16));
    Alphabet A;
    build_alphabet(db->shape.alphabet, db->shape.convert_uo != 0, A);
    HIP_TRY(hipMemcpy(db->d_alpha, A.table, 256, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db->d_alpha + 256, A.alts, 320, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db->d_alpha + 576, A.alt_count, 16, hipMemcpyHostToDevice));
    return RK_OK;
}

// ---- the dense view of a small-tree image (rk_device.h, ROW_UNIT24): 24 entries per 128-byte unit instead of 16, so a read of C2
//      pulls 123 row lines from the Infinity Cache instead of 145.  Built on the device from the canonical image,
//      which stays as it is (save / load, clone, the ambiguity kernel, rk_db_fetch_row and every other kernel read that one) ----
__device__ __forceinline__ u32 compact_count(const unsigned char *blk, u32 j, bool nib) {
    return nib ? (blk[4 + j / 2] >> (4 * (j & 1))) & 15u : blk[4 + j];
}
// dense units of a canonical row of `units` units from unit cu: its entries end where the padding (slot 0) of its last unit starts;
// a row keeps at least one unit, so a k-mer has a row in the dense view exactly when it has one in the canonical image
__device__ __forceinline__ u32 dense_units_of(const Entry *rows, u32 cu, u32 units, u32 &n) {
    const Entry *last = rows + (u64)(cu + units - 1) * ROW_UNIT;
    u32 m = ROW_UNIT;
    while (m > 0 && last[m - 1].branch == 0) m--;
    n = (units - 1) * ROW_UNIT + m;
    const u32 du = (n + ROW_UNIT24 - 1) / ROW_UNIT24;
    return du ? du : 1u;
}

// pass 1, one thread per 16-byte table block: the dense unit counts of its k-mers (into the dense table, base left for pass 2) and their sum
__global__ void dense_count_kernel(const uint4 *ctab, uint4 *dtab, u64 n_blocks, u32 per, bool nib, const Entry *rows, u32 *sums) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (u64)gridDim.x * blockDim.x) {
        const uint4 cblk = ctab[b];
        const unsigned char *cb = (const unsigned char *)&cblk;
        u32 ow[4] = {0u, 0u, 0u, 0u};
        u32 cu = cblk.x, sum = 0, n;
        for (u32 j = 0; j < per; j++) {
            const u32 units = compact_count(cb, j, nib);
            if (!units) continue;
            const u32 du = dense_units_of(rows, cu, units, n);
            if (nib) ow[1 + j / 8] |= du << (4 * (j % 8));
            else ow[1 + j / 4] |= du << (8 * (j % 4));
            sum += du;
            cu += units;
        }
        dtab[b] = make_uint4(0u, ow[1], ow[2], ow[3]);
        sums[b] = sum;
    }
}

// pass 2, one thread per table block: its dense base (1 + the units of every block before it) and its rows in the dense layout
__global__ void dense_fill_kernel(const uint4 *ctab, uint4 *dtab, u64 n_blocks, u32 per, bool nib, const Entry *rows, const u32 *bases,
                                  float T, uint4 *drows) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (u64)gridDim.x * blockDim.x) {
        const uint4 cblk = ctab[b];
        const unsigned char *cb = (const unsigned char *)&cblk;
        u32 cu = cblk.x, du0 = bases[b], n;
        ((u32 *)dtab)[4 * b] = du0;
        for (u32 j = 0; j < per; j++) {
            const u32 units = compact_count(cb, j, nib);
            if (!units) continue;
            const u32 du = dense_units_of(rows, cu, units, n);
            const Entry *src = rows + (u64)cu * ROW_UNIT;
            for (u32 q = 0; q < du; q++) {
                u32 s[ROW_UNIT24], d[ROW_UNIT24];
#pragma unroll
                for (u32 t = 0; t < ROW_UNIT24; t++) {
                    const u32 e = q * ROW_UNIT24 + t;
                    const Entry x = e < n ? src[e] : Entry{0u, 0.0f};
                    s[t] = x.branch >> 2;  // byte offset of the branch's word -> word index (<= SLOT24_MAX: n_branches <= 1 023)
                    d[t] = s[t] ? __float_as_uint(x.score - T) : 0u;  // = apply_slot's fl(v - T), bit for bit
                }
                u32 w[32];
#pragma unroll
                for (u32 i = 0; i < 16; i++) w[2 * i] = d[i];
#pragma unroll
                for (u32 i = 0; i < 8; i++) {
                    w[2 * i + 1] = d[16 + i];
                    w[2 * (8 + i) + 1] = s[i] | s[i + 8] << SLOT24_BITS | s[16 + i] << (2 * SLOT24_BITS);
                }
                uint4 *dst = drows + (u64)(du0 + q) * 8;
#pragma unroll
                for (u32 i = 0; i < 8; i++) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
            }
            du0 += du;
            cu += units;
        }
    }
}

// Every small-tree image place_packed16_kernel serves gets the view (the canonical layout stays in use when it cannot be made: out of
// device memory, or the developer knob RK_NO_DENSE_UNITS, read per handle, for A/B runs and tests).  Needs the canonical image complete
// on the current device.
static void build_dense_view(rk_db *db) {
    if (db->info.table_mode != RK_TABLE_DIRECT || db->info.n_branches > SLOT24_MAX || db->shape.indexed || db->shape.windowed ||
        db->info.rows_bytes >= ROWS_FIT32_LIMIT || db->info.table_bytes < 16 || rk_knob("RK_NO_DENSE_UNITS"))
        return;
    // ... where rows stream (the nibble form's rule, build_table): a dense step costs more VALU and LDS work per unit, which only fewer row
    // lines pay back.  C4 (0.13 row units per k-mer code) placed 7.97e8 reads/s with the view against 8.26e8 without; C2 (1.03): 3.78e8
    // against 3.66e8
    if (2 * (db->info.rows_bytes / 128) < db->info.table_slots) return;
    const u64 n_blocks = db->info.table_bytes / 16;
    const u32 per = db->shape.nib ? 2 * COMPACT_KMERS : COMPACT_KMERS;
    const unsigned grid = (unsigned)std::min<u64>((n_blocks + 255) / 256, (u64)db->cu_count * 8);
    u32 *d_sums = nullptr;
    bool ok = false;
    do {
        std::vector<u32> sums(n_blocks);
        if (hipMalloc((void **)&d_sums, n_blocks * 4) != hipSuccess || hipMalloc(&db->d_dense_table, n_blocks * 16) != hipSuccess) break;
        hipLaunchKernelGGL(dense_count_kernel, dim3(grid), dim3(256), 0, db->stream, (const uint4 *)db->d_table, (uint4 *)db->d_dense_table,
                           (u64)n_blocks, per, db->shape.nib, (const Entry *)db->d_rows, d_sums);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(sums.data(), d_sums, n_blocks * 4, hipMemcpyDeviceToHost, db->stream) != hipSuccess ||
            hipStreamSynchronize(db->stream) != hipSuccess)
            break;
        u64 next = 1;  // unit 0: reserved, all zero
        for (u64 b = 0; b < n_blocks; b++) {
            const u64 c = sums[b];
            sums[b] = (u32)next;
            next += c;
        }
        const u64 bytes = next * 128;
        if (bytes > db->info.rows_bytes) break;  // (cannot happen: a dense row never has more units than its canonical one)
        if (hipMalloc(&db->d_dense_rows, bytes) != hipSuccess || hipMemsetAsync(db->d_dense_rows, 0, 128, db->stream) != hipSuccess ||
            hipMemcpyAsync(d_sums, sums.data(), n_blocks * 4, hipMemcpyHostToDevice, db->stream) != hipSuccess)
            break;
        hipLaunchKernelGGL(dense_fill_kernel, dim3(grid), dim3(256), 0, db->stream, (const uint4 *)db->d_table, (uint4 *)db->d_dense_table,
                           (u64)n_blocks, per, db->shape.nib, (const Entry *)db->d_rows, (const u32 *)d_sums, db->info.thr_log10,
                           (uint4 *)db->d_dense_rows);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(db->stream) != hipSuccess) break;
        db->dense_rows_bytes = bytes;
        ok = true;
    } while (false);
    if (d_sums) (void)hipFree(d_sums);
    if (!ok) {
        if (db->d_dense_table) (void)hipFree(db->d_dense_table);
        if (db->d_dense_rows) (void)hipFree(db->d_dense_rows);
        db->d_dense_table = db->d_dense_rows = nullptr;
        db->dense_rows_bytes = 0;
        (void)hipGetLastError();
    }
}

// info, device view and dense view from the shape, once d_table / d_rows / d_winspec hold the image: the one place they are derived
static void finish_db(rk_db *db) {
    const ImageShape &s = db->shape;
    info_of(s, db->info.device, &db->info);
    db->view.direct = s.mode == RK_TABLE_DIRECT8 ? (const u64 *)db->d_table : nullptr;
    db->view.compact = s.mode == RK_TABLE_DIRECT ? (const uint4 *)db->d_table : nullptr;
    db->view.compact_nib = s.nib ? 1u : 0u;
    db->view.slots = s.mode == RK_TABLE_HASH ? (const uint4 *)db->d_table : nullptr;
    db->view.hash_mask = s.hash_mask;
    db->view.rows = (const unsigned char *)db->d_rows;
    db->view.rows_bytes = s.rows_bytes;
    db->view.k = s.k; db->view.bits = s.bits; db->view.n_branches = s.n_branches; db->view.alphabet = s.alphabet;
    db->view.T = s.thr_log10; db->view.P = s.thr; db->view.convert_uo = s.convert_uo;
    db->view.soa = s.indexed ? 1u : 0u;
    db->view.mono = s.mono ? 1u : 0u;
    db->view.winspec = (s.windowed || s.has_pos) ? db->d_winspec : nullptr;
    db->view.win_w = s.windowed ? s.wp.W : 0u;
    db->view.n_win = s.windowed ? s.wp.n_win : 0u;
    build_dense_view(db);
}

static int check_launchable(const rk_db *db);

// The one way a handle is made: a handle of `shape` on `device`, its three sections allocated from the shape's sizes and filled by
// fill(db, section, dst, bytes) -> RK_* (IMG_TABLE, IMG_ROWS, then IMG_WINSPEC where the image has one; `device` is current).  What the
// four entry points differ in is their fill.  Any failure destroys the handle; the caller's current device is restored on every path.
enum { IMG_TABLE, IMG_ROWS, IMG_WINSPEC };
template <class Fill>
static int install(const ImageShape &shape, int device, Fill fill, rk_db **out) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    struct Restore { int p; ~Restore() { (void)hipSetDevice(p); } } restore{prev};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(RK_ERR_NO_DEVICE, "rk_db_create: no HIP device available (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return fail(RK_ERR_INVALID, "rk_db_create: device %d out of range (0..%d)", device, ndev - 1);
    std::unique_ptr<rk_db, void (*)(rk_db *)> db(new (std::nothrow) rk_db(), rk_db_destroy);
    if (!db) return fail(RK_ERR_NOMEM, "rk_db_create: host OOM");
    db->shape = shape;
    db->info.device = device;
    if (int rc = open_db(db.get())) return rc;
    HIP_TRY(hipMalloc(&db->d_table, shape.table_bytes ? shape.table_bytes : 8));
    HIP_TRY(hipMalloc(&db->d_rows, shape.rows_bytes));
    if (shape.windowed || shape.has_pos) HIP_TRY(hipMalloc((void **)&db->d_winspec, shape.winspec_bytes));
    if (int rc = fill(*db, IMG_TABLE, db->d_table, shape.table_bytes)) return rc;
    if (int rc = fill(*db, IMG_ROWS, db->d_rows, shape.rows_bytes)) return rc;
    if (db->d_winspec)
        if (int rc = fill(*db, IMG_WINSPEC, (void *)db->d_winspec, shape.winspec_bytes)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    finish_db(db.get());
    if (int rc = check_launchable(db.get())) return rc;  // a tree whose score vector no kernel geometry can hold is refused here, not at the first batch
    *out = db.release();
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// the HBM image from the caller's CSR arrays (the arithmetic: rk_image_plan.h)
// ------------------------------------------------------------------------------------------------
// What a plan refuses, as the error codes and texts of the C ABI; `who` is the entry point's name
static int image_error(rk_image::Status st, const char *who, uint32_t alphabet, uint32_t k, uint32_t n_branches, uint32_t table_mode) {
    switch (st) {
    case rk_image::IMAGE_OK: return RK_OK;
    case rk_image::BAD_ALPHABET: return fail(RK_ERR_INVALID, "%s: alphabet must be 4 (DNA) or 20 (AA), got %u", who, alphabet);
    case rk_image::K_OUT_OF_RANGE: return fail(RK_ERR_UNSUPPORTED, "%s: k=%u outside supported range 2..%u for this alphabet", who, k, rk_image::max_k(alphabet));
    case rk_image::BAD_BRANCHES: return fail(RK_ERR_INVALID, "%s: n_branches=%u must be in 1..65535 (branch ids are 16-bit)", who, n_branches);
    case rk_image::THRESHOLD_NOT_FINITE: return fail(RK_ERR_INVALID, "%s: thresholds must be finite", who);
    case rk_image::DIRECT_TOO_LARGE: return fail(RK_ERR_UNSUPPORTED, "%s: direct table needs sigma^k <= 2^31 slots", who);
    case rk_image::BAD_TABLE_MODE: return fail(RK_ERR_INVALID, "%s: bad table_mode %u", who, table_mode);
    default: return fail(RK_ERR_UNSUPPORTED, "%s: row blob exceeds 8 TiB", who);
    }
}

// Validation + host-side construction of the image (no HIP call in here: rk_db_validate runs it without a device): check, order keys,
// plan layout, fill rows, table, finish.  An allocation that fails leaves through the entry point's guard (RK_ERR_NOMEM).
struct DbImage {
    ImageShape shape;
    std::vector<uint64_t> table;
    std::vector<Entry> blob;
    std::vector<unsigned char> winspec;  // [sigma^k], or empty
};
using KeyOrder = std::vector<std::pair<uint64_t, uint64_t>>;  // (dense index, key number), ascending
static const char *const CREATE = "rk_db_create";  // (rk_db_validate and rk_db_save_desc report under this name too)

// check: the scalars and arrays of the description, the table mode (AUTO resolved); fills the shape's scalars
static int check_desc(const rk_db_desc *d, ImageShape &shape, rk_image::TableMode &tm) {
    if (!d) return fail(RK_ERR_INVALID, "rk_db_create: null argument");
    if (int rc = image_error(rk_image::check_scalars(d->alphabet, d->k, d->n_branches, d->thr_log10, d->thr), CREATE, d->alphabet, d->k, d->n_branches, d->table_mode)) return rc;
    if (d->n_keys && (!d->key_codes || !d->row_offsets)) return fail(RK_ERR_INVALID, "rk_db_create: null key arrays");
    const uint64_t n_entries = d->n_keys ? d->row_offsets[d->n_keys] : 0;
    if (n_entries && (!d->branch_ids || !d->scores)) return fail(RK_ERR_INVALID, "rk_db_create: null entry arrays");
    if (d->n_keys && d->row_offsets[0] != 0) return fail(RK_ERR_INVALID, "rk_db_create: row_offsets[0] must be 0");
    shape.alphabet = d->alphabet; shape.convert_uo = d->convert_uo; shape.k = d->k; shape.n_branches = d->n_branches;
    shape.thr_log10 = d->thr_log10; shape.thr = d->thr;
    shape.bits = rk_image::bits_of(d->alphabet); shape.n_keys = d->n_keys; shape.n_entries = n_entries;
    tm = rk_image::resolve_table_mode(d->table_mode, d->alphabet, d->k, 1ull << 40);
    shape.mode = tm.mode;
    return image_error(tm.status, CREATE, d->alphabet, d->k, d->n_branches, tm.mode);
}

// order keys: every code a k-mer, none twice; rows are laid out in dense-index order of their k-mer
static int order_keys(const rk_db_desc *d, uint32_t bits, KeyOrder &order) {
    order.resize(d->n_keys);
    for (uint64_t r = 0; r < d->n_keys; r++) {
        uint64_t dense;
        if (!rk_image::dense_of_code(bits, d->k, d->key_codes[r], dense)) return fail(RK_ERR_INVALID, "rk_db_create: key %llu has an invalid k-mer code", (unsigned long long)r);
        order[r] = {dense, r};
    }
    std::sort(order.begin(), order.end());
    for (uint64_t i = 1; i < d->n_keys; i++)
        if (order[i].first == order[i - 1].first)
            return fail(RK_ERR_INVALID, "rk_db_create: duplicate k-mer code at key %llu", (unsigned long long)order[i].second);
    return RK_OK;
}

// plan layout: the kind of image from the row lengths (the window plan sees the measured density, the image carries position keys),
// then a descriptor per key number, rows in dense order
static int plan_layout(const rk_db_desc *d, const KeyOrder &order, uint32_t bits, const rk_image::TableMode &tm, rk_image::KindPlan &kind,
                       rk_image::RowLayout &lay, std::vector<uint64_t> &desc, uint32_t &max_len) {
    rk_image::RowStats rs;
    for (uint64_t r = 0; r < d->n_keys; r++) rs.add(d->row_offsets[r + 1] - d->row_offsets[r]);  // (the offsets themselves are tested below)
    kind = rk_image::plan_kind(d->n_branches, bits, tm, rs, rk_image::measured_density(rs, tm.space), true, geom_knobs());
    lay = rk_image::RowLayout(kind.indexed);
    desc.resize(d->n_keys);
    max_len = 0;
    for (uint64_t i = 0; i < d->n_keys; i++) {
        const uint64_t r = order[i].second, b = d->row_offsets[r], e = d->row_offsets[r + 1];
        if (e < b) return fail(RK_ERR_INVALID, "rk_db_create: row_offsets not monotone at key %llu", (unsigned long long)r);
        const uint64_t len = e - b;
        if (len == 0) return fail(RK_ERR_INVALID, "rk_db_create: key %llu has an empty row", (unsigned long long)r);
        if (len > d->n_branches)
            return fail(RK_ERR_INVALID, "rk_db_create: row %llu has %llu entries (> n_branches)", (unsigned long long)r, (unsigned long long)len);
        if (len > max_len) max_len = (uint32_t)len;
        desc[r] = lay.add_row(len);
    }
    return image_error(lay.finish(), CREATE, d->alphabet, d->k, d->n_branches, tm.mode);
}

// fill rows, one thread's share: the rows of keys r_lo .. r_hi validated and written where their descriptors point; with_keys: their
// winspec bytes too (windows or 64ths of the tree, key_w branches each).  Stops at the first bad row.
struct RowErr { int kind = 0; uint64_t r = ~0ull; uint32_t x = 0; };  // 1: branch id out of range, 2: repeated in the row, 3: score not finite
static void fill_row_range(const rk_db_desc *d, bool indexed, const std::vector<uint64_t> &desc, uint64_t r_lo, uint64_t r_hi, Entry *blob,
                           unsigned char *ws_by_key, uint32_t key_w, RowErr &err, bool &mono) {
    std::vector<uint32_t> stamp(d->n_branches, 0xFFFFFFFFu);
    std::vector<Entry> tmp;
    for (uint64_t r = r_lo; r < r_hi; r++) {
        const uint64_t b = d->row_offsets[r], len = d->row_offsets[r + 1] - b;
        Entry *ep = blob + (desc[r] >> DESC_LEN_BITS);
        if (indexed) { tmp.resize(len); ep = tmp.data(); }
        uint32_t xmin = 0xFFFFu, xmax = 0;
        for (uint64_t i = 0; i < len; i++) {
            const uint16_t x = d->branch_ids[b + i];
            xmin = x < xmin ? x : xmin;
            xmax = x > xmax ? x : xmax;
            const float v = d->scores[b + i];
            if (x >= d->n_branches) { err = {1, r, x}; return; }
            if (stamp[x] == (uint32_t)r) { err = {2, r, x}; return; }
            stamp[x] = (uint32_t)r;
            if (!std::isfinite(v)) { err = {3, r, x}; return; }
            if (!(v >= d->thr_log10)) mono = false;
            ep[i].branch = indexed ? (uint32_t)x : slot_offset(x);  // raw id (sorted, SoA below) | slot byte offset
            ep[i].score = v;
        }
        if (ws_by_key) ws_by_key[r] = winspec_byte(xmin / key_w, xmax / key_w);
        if (!indexed) continue;
        std::sort(ep, ep + len, [](const Entry &p, const Entry &q) { return p.branch < q.branch; });
        unsigned char *row = (unsigned char *)(blob + (desc[r] >> DESC_LEN_BITS));
        const uint64_t lenp = (uint32_t)desc[r] & DESC_LEN_MASK;
        uint16_t *split = (uint16_t *)(row - 64);  // the 64-byte line in front of the row
        uint16_t *bp = (uint16_t *)row;
        float *sp = (float *)(row + 2 * lenp);
        uint64_t e = 0;
        for (uint32_t i = 1; i <= 32; i++) {
            const uint32_t bound = index_bound(i, d->n_branches);
            while (e < len && ep[e].branch < bound) e++;
            split[i - 1] = (uint16_t)e;
        }
        for (uint64_t i = 0; i < lenp; i++) {
            bp[i] = i < len ? (uint16_t)ep[i].branch : RAW_PAD_BRANCH;
            sp[i] = i < len ? ep[i].score : RAW_PAD_SCORE;
        }
    }
}

// fill rows: rows are independent, so a few host threads take contiguous key ranges of (roughly) equal entry counts (6e8 entries took
// 14 s on one); the error reported is that of the first bad row by key number
static int fill_rows(const rk_db_desc *d, const rk_image::KindPlan &kind, const rk_image::RowLayout &lay, const std::vector<uint64_t> &desc,
                     std::vector<Entry> &blob, std::vector<unsigned char> &ws_by_key, bool &mono) {
    const uint64_t n_keys = d->n_keys, n_entries = n_keys ? d->row_offsets[n_keys] : 0;
    // padding / reserved line 0: raw-id images (large trees) skip on 0xFFFF, slot-offset images update scratch slot 0
    blob.assign(lay.blob_bytes / 8, lay.indexed ? Entry{0xFFFFFFFFu, RAW_PAD_SCORE} : slot_padding());
    if (kind.want_windows || kind.want_pos) ws_by_key.assign(n_keys, 0);
    unsigned hw = std::thread::hardware_concurrency();
    const unsigned T = n_entries > (1u << 22) ? std::max(1u, std::min(hw ? hw : 1u, 16u)) : 1u;
    std::vector<RowErr> errs(T);
    std::vector<char> monos(T, 1);
    std::vector<std::thread> th;
    std::vector<uint64_t> cut(T + 1, n_keys);
    cut[0] = 0;
    for (unsigned t = 1; t < T; t++)
        cut[t] = (uint64_t)(std::lower_bound(d->row_offsets, d->row_offsets + n_keys, n_entries * t / T) - d->row_offsets);
    for (unsigned t = 0; t < T; t++) {
        auto job = [&, t]() {
            bool m = true;
            fill_row_range(d, lay.indexed, desc, cut[t], cut[t + 1], blob.data(), ws_by_key.empty() ? nullptr : ws_by_key.data(), kind.key_w, errs[t], m);
            monos[t] = m ? 1 : 0;
        };
        if (t + 1 < T) th.emplace_back(job); else job();
    }
    for (std::thread &x : th) x.join();
    const RowErr *first = nullptr;
    for (const RowErr &e : errs)
        if (e.kind && (!first || e.r < first->r)) first = &e;
    if (first) {
        if (first->kind == 1) return fail(RK_ERR_INVALID, "rk_db_create: branch id %u >= n_branches in row %llu", first->x, (unsigned long long)first->r);
        if (first->kind == 2) return fail(RK_ERR_INVALID, "rk_db_create: branch id %u repeated inside row %llu", first->x, (unsigned long long)first->r);
        return fail(RK_ERR_INVALID, "rk_db_create: non-finite score in row %llu", (unsigned long long)first->r);
    }
    mono = std::find(monos.begin(), monos.end(), 0) == monos.end();
    return RK_OK;
}

static int build_image(const rk_db_desc *d, DbImage &img) {
    ImageShape &shape = img.shape;
    rk_image::TableMode tm{};
    if (int rc = check_desc(d, shape, tm)) return rc;
    KeyOrder order;
    if (int rc = order_keys(d, shape.bits, order)) return rc;
    rk_image::KindPlan kind;
    rk_image::RowLayout lay(false);
    std::vector<uint64_t> desc;  // by key number
    uint32_t max_len = 0;
    if (int rc = plan_layout(d, order, shape.bits, tm, kind, lay, desc, max_len)) return rc;
    std::vector<unsigned char> ws_by_key;  // winspec_byte(first window, last window) of every row, or empty
    if (int rc = fill_rows(d, kind, lay, desc, img.blob, ws_by_key, shape.mono)) return rc;
    rk_image::build_table(shape, tm.space, lay, [&](uint64_t i) { return order[i].first; }, [&](uint64_t i) { return desc[order[i].second]; },
                          [&](uint64_t i) { return d->key_codes[order[i].second]; }, image_knobs(), img.table);
    rk_image::finish_shape(shape, lay, kind, img.table.size(), max_len, tm.space);
    if (shape.winspec_bytes) {
        img.winspec.assign(tm.space, 0);
        for (uint64_t i = 0; i < shape.n_keys; i++) img.winspec[order[i].first] = ws_by_key[order[i].second];
    }
    return RK_OK;
}

extern "C" int rk_db_validate(const rk_db_desc *d, rk_db_info *info) {
    RK_GUARD_BEGIN
    DbImage img;
    int rc = build_image(d, img);
    if (rc) return rc;
    if (info) info_of(img.shape, -1, info);
    return RK_OK;
    RK_GUARD_END("rk_db_validate")
}

extern "C" int rk_db_create(const rk_db_desc *d, rk_db **out) {
    RK_GUARD_BEGIN
    if (!d || !out) return fail(RK_ERR_INVALID, "rk_db_create: null argument");
    *out = nullptr;
    DbImage img;
    if (int rc = build_image(d, img)) return rc;  // argument errors are reported before the device is looked at
    const void *from[3] = {img.table.data(), img.blob.data(), img.winspec.data()};
    return install(img.shape, d->device, [&](const rk_db &, int sec, void *dst, uint64_t bytes) -> int {
        if (bytes) HIP_TRY(hipMemcpy(dst, from[sec], bytes, hipMemcpyHostToDevice));
        return RK_OK;
    }, out);
    RK_GUARD_END("rk_db_create")
}

// A second handle of the same database on another (or the same) device, copied device to device: the image is not rebuilt and
// nothing goes back through the host (a C5-class image is 200 GB; xGMI moves it in seconds, the host could not even hold it).
extern "C" int rk_db_clone(const rk_db *src, int32_t device, rk_db **out) {
    RK_GUARD_BEGIN
    if (!src || !out) return fail(RK_ERR_INVALID, "rk_db_clone: null argument");
    *out = nullptr;
    const void *from[3] = {src->d_table, src->d_rows, src->d_winspec};
    const int sdev = src->info.device;
    int rc = install(src->shape, device, [&](const rk_db &, int sec, void *dst, uint64_t bytes) -> int {
        if (!bytes) return RK_OK;
        if (device == sdev) HIP_TRY(hipMemcpy(dst, from[sec], bytes, hipMemcpyDeviceToDevice));
        else HIP_TRY(hipMemcpyPeer(dst, device, from[sec], sdev, bytes));
        return RK_OK;
    }, out);
    if (rc == RK_OK) (*out)->lanes_per_read = src->lanes_per_read;
    return rc;
    RK_GUARD_END("rk_db_clone")
}

extern "C" int rk_db_get_info(const rk_db *db, rk_db_info *info) {
    if (!db || !info) return fail(RK_ERR_INVALID, "rk_db_get_info: null argument");
    *info = db->info;
    return RK_OK;
}

extern "C" void *rk_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)fail(e == hipErrorOutOfMemory ? RK_ERR_NOMEM : RK_ERR_HIP, "rk_host_alloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

extern "C" void rk_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

extern "C" uint32_t rk_packed_words(const rk_db *db, uint32_t max_len) {
    if (!db) return 0;
    uint64_t bits = (uint64_t)max_len * db->info.bits_per_symbol;
    uint32_t w = (uint32_t)((bits + 31) / 32);
    return w ? w : 1;
}

extern "C" int rk_set_lanes_per_read(rk_db *db, uint32_t lanes) {
    if (!db) return fail(RK_ERR_INVALID, "rk_set_lanes_per_read: null db");
    if (lanes != 0 && lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64)
        return fail(RK_ERR_INVALID, "rk_set_lanes_per_read: lanes must be 0 (auto), 8, 16, 32 or 64");
    if (lanes != 0 && db->shape.indexed)
        return fail(RK_ERR_UNSUPPORTED, "rk_set_lanes_per_read: this database uses the large-tree image (n_branches > %u, long rows): always the workgroup-per-read kernel", RK_WG_MIN_BRANCHES);
    db->lanes_per_read = lanes;
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// launch geometry
// ------------------------------------------------------------------------------------------------
// (the arithmetic: rk_geometry.h)  What a geometry refuses, as the error codes and texts of the C ABI
static int geometry_error(rk_geom::Status st, const rk_db *db, uint32_t keep_at_most = 0, size_t lds_per_read = 0) {
    switch (st) {
    case rk_geom::GEOM_OK: return RK_OK;
    case rk_geom::KEEP_NEEDS_LANES: return fail(RK_ERR_INVALID, "keep_at_most=%u needs lanes_per_read >= %u", keep_at_most, keep_at_most);
    case rk_geom::READ_EXCEEDS_LDS: return fail(RK_ERR_UNSUPPORTED, "n_branches=%u needs %zu B of LDS per read, more than one CU has (%zu B)", db->info.n_branches, lds_per_read, db->lds_per_cu);
    case rk_geom::NO_WG_WINDOW: return fail(RK_ERR_UNSUPPORTED, "n_branches=%u: no score-vector window fits one CU's LDS (%zu B)", db->info.n_branches, db->lds_per_cu);
    case rk_geom::WINDOWED_NO_FIT: return fail(RK_ERR_UNSUPPORTED, "internal: windowed geometry does not fit the LDS");
    default: return fail(RK_ERR_INVALID, "internal: ambiguity kernel launched without a score-vector geometry");
    }
}
static int db_geometry(const rk_db *db, uint32_t keep_at_most, Geometry &g) {
    const rk_geom::Status st = rk_geom::choose_geometry(db->info.n_branches, db->info.bits_per_symbol, db->lds_per_cu, db->lanes_per_read, keep_at_most, geom_knobs(), g);
    return geometry_error(st, db, keep_at_most, st == rk_geom::READ_EXCEEDS_LDS ? g.lds_per_wave : 0);
}
static int db_wg_geometry(const rk_db *db, WgGeometry &g, uint32_t keep_at_most = 16) {
    return geometry_error(rk_geom::choose_wg_geometry(db->info.n_branches, db->lds_per_cu, keep_at_most, geom_knobs(), g), db);
}

// 16 lanes per read, direct table, 32-bit row offsets, packed record of <= 16 words: the tile-pipelined kernel
static bool use_pipelined16(const rk_db *db, const Geometry &g, const PlaceArgs &args) {
    static const bool off = rk_knob("RK_NO_PIPE") != nullptr;  // developer knob: A/B against place_packed_kernel
    return !off && g.G == 16 && db->info.table_mode != RK_TABLE_HASH && db->info.rows_bytes < ROWS_FIT32_LIMIT && args.words_per_read <= 16;
}

template <int G, int BITS, int TM, bool WIDE>
static int launch_variant(const rk_db *db, const Geometry &g, const PlaceArgs &args, hipStream_t stream) {
    constexpr int PU = rk_geom::probe_unroll(G, BITS);
    constexpr int U = G == 64 ? RK_RING64 : RK_RING;
    auto kern = place_packed_kernel<G, BITS, TM, WIDE, U, PU>;
    decltype(kern) clade_kern = nullptr;
    PlaceArgs la = args;
    bool whole_simds = false;
    if constexpr (G == 16 && !WIDE && TM != TM_HASH) {
        if (use_pipelined16(db, g, args)) {
            // The waves of this kernel take their tiles at a fixed stride, so each does the same share of the batch and a CU's four
            // SIMDs finish together only if they hold the same number of waves.  C4: 14 592 B of LDS a wave allow ten waves a CU; at
            // 201 VGPRs the registers held it to eight, at 163 (round 8) ten were resident, three on two SIMDs and two on the others,
            // and the batch took 1.45 ms instead of 1.14 -- the 0.25 / 0.30 of the uneven split.  Nine to eleven resident waves of a
            // compact-table instance go back to the eight (two a SIMD) that every such instance had before; nothing else changes.
            whole_simds = TM == TM_COMPACT;
            constexpr bool D24 = TM == TM_COMPACT;  // (the other tables have no dense view: k24 is k16 there)
            constexpr int U24 = D24 ? RK_RING_DENSE : U;  // the dense instances' own ring (DESIGN.md 4.1a "Round 11")
            auto k16 = place_packed16_kernel<BITS, TM, U, PU>;
            auto k24 = place_packed16_kernel<BITS, TM, U24, PU, D24>;
            if constexpr (BITS == 5) {
                // every read of the batch has the same, known length and at most 96 k-mers (C4: 100 residues, k = 5): six rounds
                if (!args.lens && args.fixed_len >= db->info.k && args.fixed_len - db->info.k + 1 <= 96u) {
                    k16 = place_packed16_kernel<BITS, TM, U, 6>;
                    k24 = place_packed16_kernel<BITS, TM, U24, 6, D24>;
                }
            }
            kern = k16;
            if (TM == TM_COMPACT && db->d_dense_rows) {  // the dense view: its own table and row blob, for this kernel only
                kern = k24;
                la.db.compact = (const uint4 *)db->d_dense_table;
                la.db.rows = (const unsigned char *)db->d_dense_rows;
                la.db.rows_bytes = db->dense_rows_bytes;
                // Reads of a clade find most of their row lines in the L2 already, so the lines the view saves do not pay for its longer
                // step (C2's clade line: 3.14e8 reads/s with the view against 3.27e8 without).  Where the re-tiling pre-pass judged the
                // batch on the device, both kernels are launched and the one the batch is not for returns at once (PlaceArgs::only_if).
                if (args.perm) {
                    clade_kern = k16;
                    la.only_if = 3u;  // bits 0, 1: uniform reads (batch_is_mine)
                }
            }
        }
    }
    const Grid grid{64, g.lds_per_wave, g.waves_per_cu, (args.n_reads + g.NG - 1) / g.NG, whole_simds};
    if (int rc = launch_grid(db->cu_count, kern, grid, stream, la)) return rc;
    if (!clade_kern) return RK_OK;
    PlaceArgs ca = args;
    ca.only_if = 4u;  // bit 2: reads of a clade
    return launch_grid(db->cu_count, clade_kern, grid, stream, ca);
}

template <int G, int BITS>
static int launch_t(const rk_db *db, const Geometry &g, const PlaceArgs &a, hipStream_t s) {
    const bool wide = db->info.rows_bytes >= ROWS_FIT32_LIMIT;  // 32-bit row offsets whenever the row blob is < 4 GiB
    switch (db->info.table_mode) {
    case RK_TABLE_DIRECT: return wide ? launch_variant<G, BITS, TM_COMPACT, true>(db, g, a, s) : launch_variant<G, BITS, TM_COMPACT, false>(db, g, a, s);
    case RK_TABLE_DIRECT8: return wide ? launch_variant<G, BITS, TM_DIRECT8, true>(db, g, a, s) : launch_variant<G, BITS, TM_DIRECT8, false>(db, g, a, s);
    default: return wide ? launch_variant<G, BITS, TM_HASH, true>(db, g, a, s) : launch_variant<G, BITS, TM_HASH, false>(db, g, a, s);
    }
}
// mid-size trees: the windowed kernel whenever the image carries window spans, nobody forced a lane-group width, the K best
// of the tree fit one 16-lane row (keep_at_most <= 16) and the packed record fits one word per lane
static bool use_windowed(const rk_db *db, uint32_t keep_at_most, uint32_t words_per_read) {
    static const bool off = rk_knob("RK_NO_WINDOW") != nullptr;  // developer knob: A/B against the dense kernels
    // (scripts/keep_at_most_sweep.py, windowed against dense, Mreads/s: 3 999 branches K = 9 / 12 / 16: 156 / 141 / 105 against 91 / 84 / 76)
    // Records of more than 16 words (the kernel then reads its k-mers from memory, and a long read is emitted in several window
    // ranges): ahead of the dense kernels while a read has fewer symbols than about a ninth of the tree's branches
    // (scripts/read_length_sweep.py, G k-mers/s windowed against dense: 3 999 branches 300 / 450 / 600 bp: 25.6 / 19.8 / 16.4 against
    // 18.3 / 20.6 / 22.0; 7 999: 450 / 600 / 1000 bp: 17.5 / 15.2 / 10.8 against 11.8 / 12.7 / 14.4; 15 999: 1000 bp 9.7 against 6.8)
    const uint64_t max_symbols = (uint64_t)words_per_read * 32 / db->info.bits_per_symbol;
    const bool fits = words_per_read <= 16 || max_symbols * 9 <= db->info.n_branches || db->info.n_branches > 16000;  // (25 001 branches: 10.2 against 3.3 at 1000 bp)
    return !off && db->shape.windowed && db->lanes_per_read == 0 && keep_at_most <= 16 && fits;
}

// ---- scratch of a launch: owned by the handle, one grow-only block per stream a caller launches on.  Nothing is taken from (and no
//      attribute is set on) the device's default memory pool, which the hosting process -- a JVM, PyTorch -- shares.  Returns nullptr
//      when the block would have to grow and cannot right now (the stream is being captured into a graph, the device is out of
//      memory): the callers then do without it (batch order kept, place_packed16w_kernel alone).  Calls on ONE stream must not
//      overlap in time (include/rappas_place.h): growing the block waits for the stream's work and frees the old one ----
static void *launch_scratch(const rk_db *db, hipStream_t s, size_t bytes) {
    std::lock_guard<std::mutex> lock(db->scratch_mu);
    rk_db::LaunchScratch *b = nullptr;
    for (auto &x : db->scratch)
        if (x.s == s) { b = &x; break; }
    if (!b) {
        if (db->scratch.size() >= 16) {  // a caller that makes a stream per call: the least recently used block goes (its stream may be gone, so the whole device is waited for)
            auto lru = std::min_element(db->scratch.begin(), db->scratch.end(), [](const rk_db::LaunchScratch &x, const rk_db::LaunchScratch &y) { return x.used < y.used; });
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone || hipDeviceSynchronize() != hipSuccess) {
                (void)hipGetLastError();
                return nullptr;
            }
            if (lru->p) (void)hipFree(lru->p);
            db->scratch.erase(lru);
        }
        db->scratch.push_back({s, nullptr, 0, 0});
        b = &db->scratch.back();
    }
    b->used = ++db->scratch_clock;
    if (b->cap < bytes) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (b->p) {
            if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            (void)hipFree(b->p);
            b->p = nullptr;
            b->cap = 0;
        }
        const size_t want = ((bytes + bytes / 4) + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        if (hipMalloc(&b->p, want) != hipSuccess || !b->p) {
            (void)hipGetLastError();
            b->p = nullptr;
            return nullptr;
        }
        b->cap = want;
    }
    return b->p;
}

// ---- tiles of reads that sit in the same part of the tree (rk_kernels.hip: retile_*): keys, counting sort, the order the kernels take
//      their tiles in (PlaceArgs::perm); and the marks of the tiles a first kernel hands to place_packed16w_kernel
//      (PlaceArgs::tile_marks, one byte per tile of four reads).  Without scratch, or below 32 768 reads (the pre-pass's launches
//      cost more than they can win), the batch keeps its order ----
struct TileOrder {
    unsigned char *marks = nullptr;  // zeroed by prepare() when asked for
    int prepare(const rk_db *db, PlaceArgs &a, hipStream_t s, bool want_marks) {
        a.perm = nullptr;
        a.keep_order = nullptr;
        a.tile_marks = nullptr;
        uint64_t retile_min = 32768;
        if (const char *e = rk_knob("RK_RETILE_MIN_READS")) retile_min = (uint64_t)atoll(e);  // developer / test knob (0 = always)
        // (images without a position byte per k-mer -- hashed tables, the large-tree image -- keep their order)
        const bool retile = db->view.winspec && a.n_reads >= retile_min && a.n_reads < (1ull << 32) && !rk_knob("RK_NO_RETILE");
        if (!retile && !want_marks) return RK_OK;
        const size_t n_tiles = (size_t)((a.n_reads + 3) / 4);
        const size_t marks_off = 1024, perm_off = marks_off + (want_marks ? ((n_tiles + 255) & ~(size_t)255) : 0);
        const size_t keys_off = perm_off + (retile ? (((size_t)a.n_reads * 4 + 255) & ~(size_t)255) : 0);
        // (the marked tiles as a list + the queue's two counters, in front of the marks: place_packed16w_kernel as the second launch)
        const bool want_list = want_marks && n_tiles < (1ull << 32);
        const size_t list_off = (keys_off + (retile ? a.n_reads : 0) + 255) & ~(size_t)255, total = list_off + (want_list ? n_tiles * 4 : 0);
        unsigned char *base = (unsigned char *)launch_scratch(db, s, total);
        if (!base) return RK_OK;
        if (want_marks) {
            marks = base + marks_off;
            HIP_TRY(hipMemsetAsync(marks - 8, 0, n_tiles + 8, s));
            a.tile_marks = marks;
            if (want_list) {
                a.marked_ctl = (uint32_t *)(marks - 8);
                a.marked_list = (uint32_t *)(base + list_off);
            }
        }
        if (!retile) return RK_OK;
        uint32_t *hist = (uint32_t *)base, *cursor = hist + 128, *perm = (uint32_t *)(base + perm_off);
        unsigned char *keys = base + keys_off;
        HIP_TRY(hipMemsetAsync(base, 0, marks_off - 8, s));  // (the last 8 bytes: the hand-over queue's counters, zeroed with the marks)
        const unsigned nblk = (unsigned)std::min<uint64_t>((a.n_reads + 255) / 256, 2048);  // (grid-stride: a batch that keeps its order ends 2 048 blocks, not a million threads)
        const unsigned sblk = (unsigned)((a.n_reads / 64 + 255) / 256 + 1);
        if (db->info.bits_per_symbol == 2) hipLaunchKernelGGL(retile_sample_kernel<2>, dim3(sblk), dim3(256), 0, s, a, hist);
        else hipLaunchKernelGGL(retile_sample_kernel<5>, dim3(sblk), dim3(256), 0, s, a, hist);
        // (a batch is "sparse" when its sampled k-mers have a row at most 1.3 times as often as a random read's: the share of the alphabet's
        //  k-mer codes that carry one)
        double space = 1.0;
        for (uint32_t i = 0; i < db->info.k; i++) space *= (double)db->info.alphabet;
        const double share = std::min(1.0, 1.3 * (double)db->info.n_keys / space);
        hipLaunchKernelGGL(retile_decide_kernel, dim3(1), dim3(64), 0, s, hist, (uint32_t)(share * 65536.0));
        if (db->info.bits_per_symbol == 2) hipLaunchKernelGGL(retile_key_kernel<2>, dim3(nblk), dim3(256), 0, s, a, keys, hist);
        else hipLaunchKernelGGL(retile_key_kernel<5>, dim3(nblk), dim3(256), 0, s, a, keys, hist);
        hipLaunchKernelGGL(retile_scan_kernel, dim3(1), dim3(64), 0, s, hist, cursor);
        hipLaunchKernelGGL(retile_scatter_kernel, dim3(nblk), dim3(256), 0, s, a.n_reads, (const unsigned char *)keys, (const uint32_t *)hist, cursor, perm);
        HIP_TRY(hipGetLastError());
        a.perm = perm;
        a.keep_order = hist + 65;  // (RETILE_BINS + 1)
        return RK_OK;
    }
};

using rk_plan::F_NONE;
using rk_plan::F_SORTED;
using rk_plan::F_HASH_BIG;
using rk_plan::F_HASH_SMALL;
static rk_plan::Knobs plan_knobs() {  // (developer knobs: the product library reads none)
    rk_plan::Knobs kn;
    kn.hash_always = rk_knob("RK_HASH_ALWAYS") != nullptr;
    kn.hash_big_table = rk_knob("RK_HASH_BIG_TABLE") != nullptr;
    kn.hash_small_table = rk_knob("RK_HASH_SMALL_TABLE") != nullptr;
    kn.hash_clade_small = rk_knob("RK_HASH_CLADE_SMALL") != nullptr;
    kn.wstream_always = rk_knob("RK_WSTREAM_ALWAYS") != nullptr;
    kn.no_wstream = rk_knob("RK_NO_WSTREAM") != nullptr;
    kn.key_slack = (uint32_t)knob_int("RK_HASH_KEY_SLACK", (int)kn.key_slack);
    return kn;
}
static uint32_t hash_key_limit(uint32_t log_slots) { return rk_plan::hash_key_limit(plan_knobs(), log_slots); }
static bool hash_capable(const rk_db *db) {  // images whose tiles can go to place_hash64_kernel first
    if (rk_knob("RK_NO_HASH") || rk_knob("RK_NO_WSTREAM") || db->info.rows_bytes >= ROWS_FIT32_LIMIT) return false;
    return rk_knob("RK_HASH_ALWAYS") || db->shape.wp.stream;
}
// the plan's inputs for reads of this shape on this image (the launch's own: verdict, first_ok, marked_list, left false)
static rk_plan::In plan_in(const rk_db *db, const rk_plan::ReadShape &rs, uint32_t words_per_read) {
    rk_plan::In in;
    in.n_branches = db->info.n_branches;
    in.est_units = rs.est_units;
    in.full_hit_entries = rk_plan::full_hit_entries(rs.max_syms, db->info.k, db->info.n_keys, db->info.n_entries);
    in.hash_capable = hash_capable(db);
    in.words_per_read = words_per_read;
    in.one_batch = rs.one_batch;
    in.stream = db->shape.wp.stream;
    in.knobs = plan_knobs();
    return in;
}

static int launch_windowed(const rk_db *db, PlaceArgs a, hipStream_t stream) {
    const WindowPlan &wp = db->shape.wp;
    const uint64_t n_tiles = (a.n_reads + 3) / 4;
    if (!n_tiles) return RK_OK;
    // (the reads of this batch may be longer than the 150 symbols the image was judged for: rk_plan::read_shape)
    const rk_plan::ReadShape rs = rk_plan::read_shape(db->info.bits_per_symbol, db->info.k, a.words_per_read, a.lens != nullptr, a.fixed_len, wp.units_per_code);
    rk_plan::In in = plan_in(db, rs, a.words_per_read);
    TileOrder order;
    if (int rc = order.prepare(db, a, stream, rk_plan::plan_fit(in).want_marks())) return rc;
    in.first_ok = a.tile_marks != nullptr;  // (no scratch to be had for the marks: place_packed16w_kernel alone)
    in.marked_list = a.marked_list != nullptr;
    // Which kernel goes first for each class of batch (rk_plan.h); when the batch went through the re-tiling pre-pass (a.perm) its
    // verdicts are on the device: the kernels that differ between the classes are launched side by side and return at once when the batch
    // is not theirs (PlaceArgs::only_if), and place_packed16w_kernel takes every tile of a batch whose class has no first kernel
    // (PlaceArgs::marked_if).  Without the verdicts (small batches) one rule serves all.
    in.verdict = a.perm != nullptr;
    const rk_plan::Plan plan = rk_plan::launch_plan(in);
    const bool dna = db->info.bits_per_symbol == 2;
    auto go = [&](auto kern, const WaveGeometry &w, PlaceArgs b) {  // one kernel on the batch's tiles, with its LDS layout
        b.s_stride = w.s_stride; b.main_cap = w.main_cap; b.work_cap = w.work_cap; b.list_cap = w.list_cap;
        return launch_grid(db->cu_count, kern, Grid{64, w.lds_wave, w.waves_cu, n_tiles}, stream, b);
    };
    auto launch_hash = [&](uint32_t log_slots, uint32_t only_if, uint32_t only_marked) -> int {
        const WaveGeometry w = rk_geom::hash_geometry(log_slots, hash_key_limit(log_slots), db->lds_per_cu, geom_knobs());
        PlaceArgs b = a;
        b.only_if = only_if; b.only_marked = only_marked;
        if (log_slots != RK_HASH_LOG_SLOTS) return dna ? go(place_hash64_kernel<2, RK_HRING, RK_HNPL, 3, RK_HASH_LOG_SLOTS - 1>, w, b) : go(place_hash64_kernel<5, RK_HRING, RK_HNPL, 2, RK_HASH_LOG_SLOTS - 1>, w, b);
        return dna ? go(place_hash64_kernel<2, RK_HRING, RK_HNPL, 3, RK_HASH_LOG_SLOTS>, w, b) : go(place_hash64_kernel<5, RK_HRING, RK_HNPL, 2, RK_HASH_LOG_SLOTS>, w, b);
    };
    auto compact_marks = [&]() -> int {  // the marked tiles as a list + the queue's counters, for the next launch
        if (!a.marked_list) return RK_OK;
        HIP_TRY(hipMemsetAsync(a.marked_ctl, 0, 8, stream));
        const unsigned nblk = (unsigned)std::min<uint64_t>((n_tiles + 255) / 256, 1024);
        hipLaunchKernelGGL(compact_marks_kernel, dim3(nblk), dim3(256), 0, stream, (const unsigned char *)a.tile_marks, n_tiles, a.marked_list, a.marked_ctl);
        HIP_TRY(hipGetLastError());
        return RK_OK;
    };
    if (plan.hash_small.run)
        if (int rc = launch_hash(RK_HASH_LOG_SLOTS - 1, plan.hash_small.only_if, 0u)) return rc;
    if (plan.hash_big.run)
        if (int rc = launch_hash(RK_HASH_LOG_SLOTS, plan.hash_big.only_if, 0u)) return rc;
    if (plan.hash_behind.run) {  // the tiles the small table handed over: the large one next, then place_packed16w_kernel for what is left
        if (int rc = compact_marks()) return rc;
        if (int rc = launch_hash(RK_HASH_LOG_SLOTS, plan.hash_behind.only_if, 1u)) return rc;
    }
    if (plan.sorted.run) {  // place_packed16s_kernel
        WaveGeometry w;
        if (int rc = geometry_error(rk_geom::sorted_geometry(wp, db->lds_per_cu, w), db)) return rc;
        PlaceArgs b = a;
        b.only_if = plan.sorted.only_if; b.only_marked = 0;  // (only_if: when another kernel takes batches of the other shape)
        if (int rc = dna ? (w.wide ? go(place_packed16s_kernel<2, 8, 9, true>, w, b) : go(place_packed16s_kernel<2, 8, 9, false>, w, b))
                         : (w.wide ? go(place_packed16s_kernel<5, 8, 7, true>, w, b) : go(place_packed16s_kernel<5, 8, 7, false>, w, b)))  // (<= 102 residues in 16 words)
            return rc;
    }
    // ---- place_packed16w_kernel: every tile (records of more than 16 words), or the tiles the first kernel handed over ----
    a.only_marked = plan.only_marked ? 1u : 0u;
    a.marked_if = plan.marked_if;
    if (a.only_marked)
        if (int rc = compact_marks()) return rc;
    WaveGeometry w;
    if (int rc = geometry_error(rk_geom::windowed_geometry(wp, a.keep_at_most, a.words_per_read, db->lds_per_cu, w), db)) return rc;
    return dna ? go(place_packed16w_kernel<2, RK_WRING, 9>, w, a) : go(place_packed16w_kernel<5, RK_WRING, 9>, w, a);
}

static int launch_place(const rk_db *db, const Geometry &g, PlaceArgs a, hipStream_t s) {
    // (reads of one clade read the same rows: taken together they find them in the L2 -- scripts/clade_sorted_probe.py)
    TileOrder order;
    if (int rc = order.prepare(db, a, s, false)) return rc;
    const bool dna = db->info.bits_per_symbol == 2;
    switch (g.G) {
    case 8: return dna ? launch_t<8, 2>(db, g, a, s) : launch_t<8, 5>(db, g, a, s);
    case 16: return dna ? launch_t<16, 2>(db, g, a, s) : launch_t<16, 5>(db, g, a, s);
    case 32: return dna ? launch_t<32, 2>(db, g, a, s) : launch_t<32, 5>(db, g, a, s);
    default: return dna ? launch_t<64, 2>(db, g, a, s) : launch_t<64, 5>(db, g, a, s);
    }
}

static int check_launchable(const rk_db *db) {
    if (db->shape.windowed) return RK_OK;  // (the windowed and the ambiguity kernel hold windows of any tree; a forced dense geometry is checked at launch)
    if (db->shape.indexed) {
        WgGeometry wg;
        return db_wg_geometry(db, wg);
    }
    Geometry g;
    return db_geometry(db, 7, g);
}

// ---- large trees: one workgroup per read ----
static int launch_wg(const rk_db *db, const WgGeometry &g, PlaceArgs a, hipStream_t stream) {
    a.s_stride = g.s_stride; a.list_cap = g.list_cap; a.n_pass = g.n_pass;
    auto go = [&](auto kern) { return launch_grid(db->cu_count, kern, Grid{64 * (int)g.nw, g.lds, g.wgs_per_cu, a.n_reads}, stream, a); };
    const bool dna = db->info.bits_per_symbol == 2, wide = db->info.rows_bytes >= ROWS_FIT32_LIMIT;
    if (db->info.table_mode == RK_TABLE_HASH) {
        if (dna) return wide ? go(place_wg_kernel<2, TM_HASH, true, RK_WG_RING>) : go(place_wg_kernel<2, TM_HASH, false, RK_WG_RING>);
        return wide ? go(place_wg_kernel<5, TM_HASH, true, RK_WG_RING>) : go(place_wg_kernel<5, TM_HASH, false, RK_WG_RING>);
    }
    if (dna) return wide ? go(place_wg_kernel<2, TM_DIRECT8, true, RK_WG_RING>) : go(place_wg_kernel<2, TM_DIRECT8, false, RK_WG_RING>);
    return wide ? go(place_wg_kernel<5, TM_DIRECT8, true, RK_WG_RING>) : go(place_wg_kernel<5, TM_DIRECT8, false, RK_WG_RING>);
}

// ---- the ambiguity kernel: the score vector, or a window of it, and the Samb / Camb windows (rk_geom::amb_geometry) ----
template <int BITS>
static int launch_ascii_v(const rk_db *db, PlaceArgs args, AmbArgs m, hipStream_t stream) {
    AmbGeometry g;
    if (int rc = geometry_error(rk_geom::amb_geometry(db->info.n_branches, db->lds_per_cu, db->shape.indexed, (size_t)ASCII_LIST_CAP * 8 + ASCII_TABLE_BYTES, geom_knobs(), g), db)) return rc;
    args.s_stride = g.s_stride; m.amb_chunk = g.amb_chunk; m.s_win = g.s_win;
    auto go = [&](auto kern) { return launch_grid(db->cu_count, kern, Grid{64, g.lds, g.waves_cu, (args.n_reads + 63) / 64}, stream, args, m); };
    switch (db->info.table_mode) {
    case RK_TABLE_DIRECT: return db->shape.indexed ? go(place_ascii_kernel<BITS, TM_COMPACT, true>) : go(place_ascii_kernel<BITS, TM_COMPACT, false>);
    case RK_TABLE_DIRECT8: return db->shape.indexed ? go(place_ascii_kernel<BITS, TM_DIRECT8, true>) : go(place_ascii_kernel<BITS, TM_DIRECT8, false>);
    default: return db->shape.indexed ? go(place_ascii_kernel<BITS, TM_HASH, true>) : go(place_ascii_kernel<BITS, TM_HASH, false>);
    }
}
static int launch_ascii(const rk_db *db, const PlaceArgs &a, const AmbArgs &m, hipStream_t s) {
    return db->info.bits_per_symbol == 2 ? launch_ascii_v<2>(db, a, m, s) : launch_ascii_v<5>(db, a, m, s);
}

static int check_params(const rk_params *p) {
    if (!p) return fail(RK_ERR_INVALID, "null rk_params");
    if (p->keep_at_most < 1 || p->keep_at_most > 16) return fail(RK_ERR_INVALID, "keep_at_most=%u outside 1..16", p->keep_at_most);
    if (p->amb_mode > RK_AMB_MAX) return fail(RK_ERR_INVALID, "amb_mode=%u invalid", p->amb_mode);
    if (std::isnan(p->keep_factor) || std::isnan(p->ns_bound)) return fail(RK_ERR_INVALID, "NaN in rk_params");
    return RK_OK;
}
// without a length array every record holds fixed_len symbols of `bits` bits: they must be there
static int check_fixed_len(const char *who, const void *lens, uint32_t fixed_len, uint32_t bits, uint32_t words) {
    if (!lens && (uint64_t)fixed_len * bits > (uint64_t)words * 32) return fail(RK_ERR_INVALID, "%s: fixed_len=%u does not fit %u words", who, fixed_len, words);
    return RK_OK;
}
static bool result_complete(const rk_result *r) { return r && r->n_rows && r->branch && r->score && r->lwr && r->flags; }

extern "C" const char *rk_kernel_name(const rk_db *db) {
    if (!db) return "";
    Geometry g;
    char buf[800];
    auto named = [&]() { return (const_cast<rk_db *>(db)->kernel_name = buf).c_str(); };
    if (db->shape.indexed && db->lanes_per_read == 0) {
        WgGeometry wg;
        if (db_wg_geometry(db, wg, 7) != RK_OK) return "";
        snprintf(buf, sizeof(buf), "place_wg_kernel<BITS=%u,%s,%s,U=%d> waves/WG=%u lds/WG=%zuB rows/batch=%u WGs/CU=%u passes=%u",
                 db->info.bits_per_symbol, db->info.table_mode == RK_TABLE_HASH ? "HASH" : "DIRECT8",
                 db->info.rows_bytes < ROWS_FIT32_LIMIT ? "OFF32" : "OFF64", RK_WG_RING, wg.nw, wg.lds, wg.list_cap, wg.wgs_per_cu, wg.n_pass);
        return named();
    }
    if (use_windowed(db, 7, 16)) {
        // (for the reads of BASELINE's configs -- 150 bases / 100 residues -- and a batch large enough for the pre-pass's verdicts)
        const uint32_t syms_name = db->info.bits_per_symbol == 5 ? 100u : 150u;
        const uint32_t wpr_name = (syms_name * db->info.bits_per_symbol + 31) / 32;
        rk_plan::ReadShape rs = rk_plan::read_shape(db->info.bits_per_symbol, db->info.k, wpr_name, false, syms_name, db->shape.wp.units_per_code);
        rs.one_batch = true;  // (reads of these lengths in records of their own length: the probe batch is the record's)
        rk_plan::In in = plan_in(db, rs, wpr_name);
        in.verdict = true;
        const rk_plan::FirstPlan pl = rk_plan::first_kernel_plan(in, rk_plan::plan_fit(in));
        auto what = [](rk_plan::First f) { return f == F_HASH_SMALL ? "place_hash64_kernel with 1 024 slots (the 2 048-slot one behind it)" : f == F_HASH_BIG ? "place_hash64_kernel" : f == F_SORTED ? "place_packed16s_kernel" : "place_packed16w_kernel"; };
        const rk_plan::First shown = pl.for_uniform == F_HASH_BIG || pl.for_uniform == F_HASH_SMALL ? pl.for_uniform : (pl.for_sparse == F_HASH_SMALL || pl.for_clade == F_HASH_SMALL || pl.for_clade == F_HASH_BIG) && pl.for_uniform == F_NONE ? pl.for_clade : pl.for_uniform;
        const bool hash_shown = shown == F_HASH_BIG || shown == F_HASH_SMALL, sparse_too = !hash_shown || pl.for_sparse != pl.for_uniform;
        char other[360] = "";  // the classes of batch that get another first kernel
        if (pl.for_clade != pl.for_uniform || pl.for_sparse != pl.for_uniform)
            snprintf(other, sizeof(other), "; batches of 32 768 reads or more, judged on the device: clade-shaped -> %s%s%s", what(pl.for_clade),
                     sparse_too ? ", uniform and sparse-hit -> " : "", sparse_too ? what(pl.for_sparse) : "");
        if (hash_shown) {
            const uint32_t ls = shown == F_HASH_SMALL ? RK_HASH_LOG_SLOTS - 1 : RK_HASH_LOG_SLOTS;
            const WaveGeometry hw = rk_geom::hash_geometry(ls, hash_key_limit(ls), db->lds_per_cu, geom_knobs());
            snprintf(buf, sizeof(buf), "place_hash64_kernel<BITS=%u,U=%d,NPL=%d,PU=%d,LOGS=%u> %u slots, <= %u keys a read%s (+ place_packed16w_kernel for the tiles it hands over; windows=%u x %u branches)",
                     db->info.bits_per_symbol, RK_HRING, RK_HNPL, db->info.bits_per_symbol == 5 ? 2 : 3, ls, hw.s_stride, hw.work_cap, other, db->shape.wp.n_win, db->shape.wp.W);
        } else if (pl.for_uniform == F_SORTED) {
            snprintf(buf, sizeof(buf), "place_packed16s_kernel<BITS=%u,U=8,PU=%d,WIDE=%d> windows=%u x %u branches%s (+ place_packed16w_kernel for the tiles it hands over)",
                     db->info.bits_per_symbol, db->info.bits_per_symbol == 5 ? 7 : 9, rk_geom::sorted_wide(db->shape.wp) ? 1 : 0, db->shape.wp.n_win, db->shape.wp.W, other);
        } else {  // (the image's plan: a launch re-balances its two lists, rk_geom::windowed_geometry)
            snprintf(buf, sizeof(buf), "place_packed16w_kernel<BITS=%u,U=%d,PU=9> windows=%u x %u branches lds/wave=%zuB main=%u work=%u", db->info.bits_per_symbol, RK_WRING,
                     db->shape.wp.n_win, db->shape.wp.W, rk_geom::lds_of_four_reads(db->shape.wp.s_stride, db->shape.wp.main_cap, db->shape.wp.work_cap), db->shape.wp.main_cap, db->shape.wp.work_cap);
        }
        return named();
    }
    if (db_geometry(db, 7, g) != RK_OK) return "";
    PlaceArgs probe{};
    probe.words_per_read = 16;
    // (the tile-pipelined variant serves packed records of <= 16 words, i.e. reads of <= 256 bases / 102 residues; longer
    // records take place_packed_kernel with the same geometry)
    const bool pipe = use_pipelined16(db, g, probe);
    // (U: the ring the geometry counts with, RK_RING; the ROW24 instances run their own, RK_RING_DENSE, on the same list)
    snprintf(buf, sizeof(buf), "%s<G=%u,BITS=%u,%s,%s%s,U=%d,PU=%u> lds/wave=%zuB cap=%u waves/CU<=%u (LDS; registers may allow fewer)%s",
             pipe ? "place_packed16_kernel" : "place_packed_kernel", g.G, db->info.bits_per_symbol, db->info.table_mode == RK_TABLE_DIRECT ? (db->shape.nib ? "DIRECT4" : "DIRECT") : (db->info.table_mode == RK_TABLE_DIRECT8 ? "DIRECT8" : "HASH"),
             pipe && db->d_dense_rows ? "ROW24," : "", db->info.rows_bytes < ROWS_FIT32_LIMIT ? "ITEM32" : "ITEM64", g.G == 64 ? RK_RING64 : RK_RING, g.pu, g.lds_per_wave, g.list_cap, g.waves_per_cu,
             pipe && db->d_dense_rows && db->view.winspec ? "; batches of 32 768 reads or more that the device judges clade-shaped: 16-entry units" : "");
    return named();
}

// ------------------------------------------------------------------------------------------------
// device entry points
// ------------------------------------------------------------------------------------------------
extern "C" int rk_pack_reads_device(rk_db *db, uint64_t n_reads, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off,
                                    uint32_t words_per_read, uint32_t *d_packed, uint32_t *d_lens, uint32_t *d_flags,
                                    void *stream) {
    if (!db || !d_seq_ascii || !d_seq_off || !d_packed || !d_lens || !d_flags || words_per_read == 0)
        return fail(RK_ERR_INVALID, "rk_pack_reads_device: null/zero argument");
    if (n_reads == 0) return RK_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(db->info.device));
    HIP_TRY(hipMemsetAsync(d_flags, 0, n_reads * sizeof(uint32_t), s));
    const uint64_t total = n_reads * words_per_read;
    uint64_t blocks = (total + 255) / 256;
    const uint64_t maxb = (uint64_t)db->cu_count * 16;
    if (blocks > maxb) blocks = maxb;
    if (db->info.bits_per_symbol == 2)
        hipLaunchKernelGGL(pack_reads_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, d_seq_ascii, (const u64 *)d_seq_off, (u64)n_reads,
                           words_per_read, (const unsigned char *)db->d_alpha, db->info.k, d_packed, d_lens, d_flags);
    else
        hipLaunchKernelGGL(pack_reads_kernel<5>, dim3((unsigned)blocks), dim3(256), 0, s, d_seq_ascii, (const u64 *)d_seq_off, (u64)n_reads,
                           words_per_read, (const unsigned char *)db->d_alpha, db->info.k, d_packed, d_lens, d_flags);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_place_packed_device(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *d_packed,
                                      uint32_t words_per_read, const uint32_t *d_lens, uint32_t fixed_len,
                                      const uint32_t *d_flags_in, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off,
                                      const rk_result *d_out, void *stream) {
    if (!db || !d_out) return fail(RK_ERR_INVALID, "rk_place_packed_device: null argument");
    int rc = check_params(p);
    if (rc) return rc;
    if (n_reads == 0) return RK_OK;
    if (!d_packed || words_per_read == 0) return fail(RK_ERR_INVALID, "rk_place_packed_device: null packed reads");
    if (!result_complete(d_out)) return fail(RK_ERR_INVALID, "rk_place_packed_device: null result array");
    rc = check_fixed_len("rk_place_packed_device", d_lens, fixed_len, db->info.bits_per_symbol, words_per_read);
    if (rc) return rc;
    const bool use_wg = db->shape.indexed && db->lanes_per_read == 0;  // an explicit lanes_per_read forces the single-wave kernel
    const bool use_win = !use_wg && use_windowed(db, p->keep_at_most, words_per_read);
    Geometry g{};
    WgGeometry wg{};
    rc = use_wg ? db_wg_geometry(db, wg, p->keep_at_most) : (use_win ? RK_OK : db_geometry(db, p->keep_at_most, g));  // (the windowed launch has its own plan)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(db->info.device));
    hipStream_t s = (hipStream_t)stream;
    PlaceArgs a{};
    a.db = db->view;
    a.n_reads = n_reads;
    a.packed = d_packed; a.words_per_read = words_per_read; a.lens = d_lens; a.fixed_len = fixed_len;
    a.flags_in = d_flags_in;
    const bool ascii = d_flags_in && d_seq_ascii && d_seq_off;
    a.has_ascii = ascii ? 1u : 0u;
    a.keep_at_most = p->keep_at_most; a.keep_factor = p->keep_factor; a.ns_bound = p->ns_bound;
    a.o_nrows = d_out->n_rows; a.o_branch = d_out->branch; a.o_score = d_out->score; a.o_lwr = d_out->lwr; a.o_flags = d_out->flags;
    a.s_stride = use_wg ? wg.s_stride : g.s_stride;
    a.list_cap = use_wg ? wg.list_cap : g.list_cap;
    if (use_wg) rc = launch_wg(db, wg, a, s);
    else if (use_win) rc = launch_windowed(db, a, s);
    else rc = launch_place(db, g, a, s);
    if (rc) return rc;
    if (ascii) {
        AmbArgs m{};
        m.ascii = d_seq_ascii; m.seq_off = (const u64 *)d_seq_off;
        m.char_table = db->d_alpha; m.alt_table = db->d_alpha + 256; m.alt_count = db->d_alpha + 576;
        m.amb_mode = p->amb_mode;
        m.max_amb = (uint32_t)std::floor(std::pow((double)db->info.k, 1.0 / (double)db->info.alphabet));  // AmbigSequenceKnife.java:95
        rc = launch_ascii(db, a, m, s);
        if (rc) return rc;
    }
    return RK_OK;
}

// ------------------------------------------------------------------------------------------------
// DNA reads on either strand: the reverse complement of packed records / characters on the device, the per-read
// merge of two result sets, and rk_place_packed_device composed over them.  Two placement passes; nothing here touches a placement
// kernel or the launch plan.
// ------------------------------------------------------------------------------------------------
static int strands_handle(const rk_db *db, const char *who) {
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    if (db->info.alphabet != RK_ALPHABET_DNA) return fail(RK_ERR_UNSUPPORTED, "%s: reverse complement is defined for DNA databases only (this one holds amino acids)", who);
    return RK_OK;
}

static unsigned strand_blocks(const rk_db *db, uint64_t threads) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((threads + 255) / 256, (uint64_t)db->cu_count * 16));
}

extern "C" int rk_revcomp_packed_device(rk_db *db, uint64_t n_reads, const uint32_t *d_packed, uint32_t words_per_read, const uint32_t *d_lens,
                                        uint32_t fixed_len, uint32_t *d_packed_out, void *stream) {
    int rc = strands_handle(db, "rk_revcomp_packed_device");
    if (rc) return rc;
    if (n_reads == 0) return RK_OK;
    if (!d_packed || !d_packed_out || words_per_read == 0) return fail(RK_ERR_INVALID, "rk_revcomp_packed_device: null/zero argument");
    if (d_packed == d_packed_out) return fail(RK_ERR_INVALID, "rk_revcomp_packed_device: the output must not alias the input");
    rc = check_fixed_len("rk_revcomp_packed_device", d_lens, fixed_len, 2, words_per_read);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(db->info.device));
    hipLaunchKernelGGL(revcomp_packed_kernel, dim3(strand_blocks(db, n_reads * words_per_read)), dim3(256), 0, (hipStream_t)stream, d_packed, (u64)n_reads,
                       words_per_read, d_lens, fixed_len, d_packed_out);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

// only_flags / out_cap: the composed call reverses the reads the ambiguity kernel takes, into the room its workspace has
static int launch_revcomp_ascii(rk_db *db, uint64_t n_reads, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off, const uint32_t *only_flags,
                                uint8_t *d_out, uint64_t out_cap, hipStream_t s) {
    hipLaunchKernelGGL(revcomp_ascii_kernel, dim3(strand_blocks(db, n_reads * 64)), dim3(256), 0, s, d_seq_ascii, (const u64 *)d_seq_off, (u64)n_reads,
                       only_flags, d_out, (u64)out_cap);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_revcomp_ascii_device(rk_db *db, uint64_t n_reads, const uint8_t *d_seq_ascii, const uint64_t *d_seq_off, uint8_t *d_out_ascii,
                                       void *stream) {
    int rc = strands_handle(db, "rk_revcomp_ascii_device");
    if (rc) return rc;
    if (n_reads == 0) return RK_OK;
    if (!d_seq_ascii || !d_seq_off || !d_out_ascii) return fail(RK_ERR_INVALID, "rk_revcomp_ascii_device: null argument");
    if (d_seq_ascii == d_out_ascii) return fail(RK_ERR_INVALID, "rk_revcomp_ascii_device: the output must not alias the input");
    HIP_TRY(hipSetDevice(db->info.device));
    return launch_revcomp_ascii(db, n_reads, d_seq_ascii, d_seq_off, nullptr, d_out_ascii, ~0ull, (hipStream_t)stream);
}

// merge_results_kernel: `cand` replaces `best` read by read where it is the better one
static int launch_merge(rk_db *db, uint32_t K, uint64_t n_reads, const rk_result *best, uint8_t *best_frame, const rk_result *cand, uint32_t mark,
                        uint32_t frame_id, hipStream_t s) {
    hipLaunchKernelGGL(merge_results_kernel, dim3(strand_blocks(db, n_reads)), dim3(256), 0, s, (u64)n_reads, K, best->n_rows, best->branch, best->score,
                       best->lwr, best->flags, best_frame, (const unsigned char *)cand->n_rows, (const unsigned short *)cand->branch,
                       (const float *)cand->score, (const double *)cand->lwr, (const uint32_t *)cand->flags, mark, frame_id);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_merge_strands_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_fwd, const rk_result *d_rev,
                                       void *stream) {
    int rc = strands_handle(db, "rk_merge_strands_device");
    if (rc) return rc;
    if (keep_at_most < 1 || keep_at_most > 16) return fail(RK_ERR_INVALID, "keep_at_most=%u outside 1..16", keep_at_most);
    if (n_reads == 0) return RK_OK;
    if (!result_complete(d_fwd) || !result_complete(d_rev)) return fail(RK_ERR_INVALID, "rk_merge_strands_device: null result array");
    HIP_TRY(hipSetDevice(db->info.device));
    return launch_merge(db, keep_at_most, n_reads, d_fwd, nullptr, d_rev, RK_FLAG_REVERSE, 0, (hipStream_t)stream);
}

#include "rk_masses_impl.h"  // the edge-mass entry points

// A second result set in a workspace, from byte offset `at` on: n_rows | branch | score | lwr | flags, each on a 256-byte boundary of
// the block.  Returns the offset behind it and, given a block, the arrays at those offsets of it.
static uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }
static uint64_t work_result(char *base, uint64_t at, uint64_t n, uint32_t K, rk_result *out) {
    const uint64_t branch = at + up256(n), score = branch + up256(n * K * 2), lwr = score + up256(n * K * 4), flags = lwr + up256(n * K * 8);
    if (base && out) *out = rk_result{(uint8_t *)(base + at), (uint16_t *)(base + branch), (float *)(base + score), (double *)(base + lwr), (uint32_t *)(base + flags)};
    return flags + up256(n * 4);
}

// The workspace of rk_place_packed_device_strands: reverse records | second result set | reversed characters.  Returns the size of
// everything before the characters.
static uint64_t strand_work(uint64_t n, uint32_t wpr, uint32_t K, char *base = nullptr, rk_result *second = nullptr) {
    return work_result(base, up256(n * wpr * 4), n, K, second);
}

extern "C" uint64_t rk_strands_work_bytes(const rk_db *db, uint64_t n_reads, uint32_t words_per_read, uint32_t keep_at_most, uint64_t ascii_bytes) {
    if (strands_handle(db, "rk_strands_work_bytes")) return 0;
    if (words_per_read == 0 || keep_at_most < 1 || keep_at_most > 16) { (void)fail(RK_ERR_INVALID, "rk_strands_work_bytes: words_per_read=%u, keep_at_most=%u", words_per_read, keep_at_most); return 0; }
    if (n_reads >= (1ull << 40)) { (void)fail(RK_ERR_INVALID, "rk_strands_work_bytes: n_reads too large"); return 0; }
    return strand_work(n_reads, words_per_read, keep_at_most) + ascii_bytes;
}

extern "C" int rk_place_packed_device_strands(rk_db *db, const rk_params *p, uint32_t strand, uint64_t n_reads, const uint32_t *d_packed,
                                              uint32_t words_per_read, const uint32_t *d_lens, uint32_t fixed_len, const uint32_t *d_flags_in,
                                              const uint8_t *d_seq_ascii, const uint64_t *d_seq_off, const rk_result *d_out, void *d_work,
                                              uint64_t work_bytes, void *stream) {
    int rc = strands_handle(db, "rk_place_packed_device_strands");
    if (rc) return rc;
    if (strand > RK_STRAND_BOTH) return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: strand=%u (0 forward, 1 reverse, 2 both)", strand);
    if (strand == RK_STRAND_FORWARD)
        return rk_place_packed_device(db, p, n_reads, d_packed, words_per_read, d_lens, fixed_len, d_flags_in, d_seq_ascii, d_seq_off, d_out, stream);
    // every test the placement call would make, before the first launch: an error leaves the caller's arrays as they are
    if (!d_out) return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: null argument");
    rc = check_params(p);
    if (rc) return rc;
    if (n_reads == 0) return RK_OK;
    if (!d_packed || words_per_read == 0) return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: null packed reads");
    if (!result_complete(d_out)) return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: null result array");
    rc = check_fixed_len("rk_place_packed_device_strands", d_lens, fixed_len, 2, words_per_read);
    if (rc) return rc;
    if (n_reads >= (1ull << 40)) return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: n_reads too large");
    char *base = (char *)d_work;
    rk_result rres{};
    const uint64_t before_ascii = strand_work(n_reads, words_per_read, p->keep_at_most, base, &rres);
    if (!d_work || work_bytes < before_ascii)
        return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: workspace of %llu bytes, %llu needed (rk_strands_work_bytes)", (unsigned long long)(d_work ? work_bytes : 0),
                    (unsigned long long)before_ascii);
    const bool ascii = d_flags_in && d_seq_ascii && d_seq_off;
    if (ascii && work_bytes == before_ascii)
        return fail(RK_ERR_INVALID, "rk_place_packed_device_strands: the workspace has no room for the reversed characters (rk_strands_work_bytes with ascii_bytes)");
    HIP_TRY(hipSetDevice(db->info.device));
    hipStream_t s = (hipStream_t)stream;
    uint32_t *rev = (uint32_t *)base;
    uint8_t *rev_ascii = ascii ? (uint8_t *)(base + before_ascii) : nullptr;
    rc = rk_revcomp_packed_device(db, n_reads, d_packed, words_per_read, d_lens, fixed_len, rev, s);
    if (rc) return rc;
    if (ascii) {
        rc = launch_revcomp_ascii(db, n_reads, d_seq_ascii, d_seq_off, d_flags_in, rev_ascii, work_bytes - before_ascii, s);
        if (rc) return rc;
    }
    if (strand == RK_STRAND_REVERSE) {
        rc = rk_place_packed_device(db, p, n_reads, rev, words_per_read, d_lens, fixed_len, d_flags_in, rev_ascii, d_seq_off, d_out, s);
        if (rc) return rc;
        hipLaunchKernelGGL(mark_reverse_kernel, dim3(strand_blocks(db, n_reads)), dim3(256), 0, s, d_out->flags, (u64)n_reads);
        HIP_TRY(hipGetLastError());
        return RK_OK;
    }
    // the reverse strand first: d_flags_in may be the output flag array itself, which the forward pass then overwrites
    rc = rk_place_packed_device(db, p, n_reads, rev, words_per_read, d_lens, fixed_len, d_flags_in, rev_ascii, d_seq_off, &rres, s);
    if (rc) return rc;
    rc = rk_place_packed_device(db, p, n_reads, d_packed, words_per_read, d_lens, fixed_len, d_flags_in, d_seq_ascii, d_seq_off, d_out, s);
    if (rc) return rc;
    return rk_merge_strands_device(db, p->keep_at_most, n_reads, d_out, &rres, s);
}

// ------------------------------------------------------------------------------------------------
// DNA reads on an amino-acid database: one reading frame of packed DNA records translated on the device, the per-read
// merge of a frame's result set into the best so far, and rk_place_packed_device composed over the six frames.  Six placement passes,
// one after the other through one record set; nothing here touches a placement kernel or the launch plan.
// ------------------------------------------------------------------------------------------------
static int translated_handle(const rk_db *db, const char *who) {
    if (!db) return fail(RK_ERR_INVALID, "%s: null handle", who);
    if (db->info.alphabet != RK_ALPHABET_AA) return fail(RK_ERR_UNSUPPORTED, "%s: translated placement needs an amino-acid database (this one holds DNA)", who);
    return RK_OK;
}

// 32-bit words of the amino-acid record of a frame of `bases` bases (rk_packed_words of an amino-acid handle)
static uint32_t translated_words(uint64_t bases) {
    const uint64_t w = (bases / 3 * 5 + 31) / 32;
    return w ? (uint32_t)w : 1u;
}

// the argument tests the device and the host translation share; 0x7FFFFFFF / 16 words: 16 * dna_words must not wrap
static int translate_args(const char *who, uint32_t frame, const void *dna, uint32_t dna_words, const void *dna_lens, uint32_t fixed_len, const void *aa,
                          uint32_t aa_words, const void *aa_lens) {
    if (frame > 5) return fail(RK_ERR_INVALID, "%s: frame=%u (0..2 as given, 3..5 the reverse complement)", who, frame);
    if (!dna || !aa || !aa_lens || dna_words == 0 || dna_words > 0x7FFFFFFu) return fail(RK_ERR_INVALID, "%s: null/zero argument", who);
    if (check_fixed_len(who, dna_lens, fixed_len, 2, dna_words)) return RK_ERR_INVALID;
    const uint32_t need = translated_words(dna_lens ? (uint64_t)dna_words * 16 : fixed_len);
    if (aa_words < need) return fail(RK_ERR_INVALID, "%s: aa_words=%u, %u needed for the longest frame of these records", who, aa_words, need);
    return RK_OK;
}

extern "C" int rk_translate_packed_device(rk_db *db, uint32_t frame, uint64_t n_reads, const uint32_t *d_dna, uint32_t dna_words,
                                          const uint32_t *d_dna_lens, uint32_t fixed_len, uint32_t *d_aa_out, uint32_t aa_words,
                                          uint32_t *d_aa_lens_out, void *stream) {
    int rc = translated_handle(db, "rk_translate_packed_device");
    if (rc) return rc;
    if (n_reads == 0) return frame > 5 ? fail(RK_ERR_INVALID, "rk_translate_packed_device: frame=%u", frame) : RK_OK;
    rc = translate_args("rk_translate_packed_device", frame, d_dna, dna_words, d_dna_lens, fixed_len, d_aa_out, aa_words, d_aa_lens_out);
    if (rc) return rc;
    if ((const void *)d_dna == (const void *)d_aa_out) return fail(RK_ERR_INVALID, "rk_translate_packed_device: the output must not alias the input");
    HIP_TRY(hipSetDevice(db->info.device));
    hipLaunchKernelGGL(translate_frame_kernel, dim3(strand_blocks(db, n_reads)), dim3(256), 0, (hipStream_t)stream, d_dna, (u64)n_reads, dna_words, d_dna_lens,
                       fixed_len, frame, d_aa_out, aa_words, d_aa_lens_out);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

extern "C" int rk_translate_packed_host(uint32_t frame, uint64_t n_reads, const uint32_t *dna, uint32_t dna_words, const uint32_t *dna_lens,
                                        uint32_t fixed_len, uint32_t *aa_out, uint32_t aa_words, uint32_t *aa_lens_out) {
    if (n_reads == 0) return frame > 5 ? fail(RK_ERR_INVALID, "rk_translate_packed_host: frame=%u", frame) : RK_OK;
    int rc = translate_args("rk_translate_packed_host", frame, dna, dna_words, dna_lens, fixed_len, aa_out, aa_words, aa_lens_out);
    if (rc) return rc;
    rk::translate_range(frame, dna, dna_words, dna_lens, fixed_len, 0, n_reads, aa_out, aa_words, aa_lens_out);
    return RK_OK;
}

extern "C" int rk_merge_frames_device(rk_db *db, uint32_t keep_at_most, uint64_t n_reads, const rk_result *d_best, uint8_t *d_best_frame,
                                      const rk_result *d_cand, uint32_t cand_frame, void *stream) {
    int rc = translated_handle(db, "rk_merge_frames_device");
    if (rc) return rc;
    if (keep_at_most < 1 || keep_at_most > 16) return fail(RK_ERR_INVALID, "keep_at_most=%u outside 1..16", keep_at_most);
    if (cand_frame > 5) return fail(RK_ERR_INVALID, "rk_merge_frames_device: cand_frame=%u outside 0..5", cand_frame);
    if (n_reads == 0) return RK_OK;
    if (!result_complete(d_best) || !result_complete(d_cand) || !d_best_frame) return fail(RK_ERR_INVALID, "rk_merge_frames_device: null result array");
    HIP_TRY(hipSetDevice(db->info.device));
    return launch_merge(db, keep_at_most, n_reads, d_best, d_best_frame, d_cand, cand_frame >= 3 ? RK_FLAG_REVERSE : 0u, cand_frame, (hipStream_t)stream);
}

// The workspace of rk_place_packed_device_translated: amino-acid records of one frame | their lengths | one result set; every part
// starts on a 256-byte boundary of the block.
struct TranslatedWork {
    uint32_t aa_words;
    uint64_t lens, total;  // byte offsets (the records are at 0)
    rk_result cand;        // with a block given: the result set in it
};
static TranslatedWork translated_work(uint64_t n, uint32_t dna_words, uint32_t K, char *base = nullptr) {
    TranslatedWork w{};
    w.aa_words = translated_words((uint64_t)dna_words * 16);
    w.lens = up256(n * w.aa_words * 4);
    w.total = work_result(base, w.lens + up256(n * 4), n, K, &w.cand);
    return w;
}

extern "C" uint64_t rk_translated_work_bytes(const rk_db *db, uint64_t n_reads, uint32_t dna_words, uint32_t keep_at_most) {
    if (translated_handle(db, "rk_translated_work_bytes")) return 0;
    if (dna_words == 0 || dna_words > 0x7FFFFFFu || keep_at_most < 1 || keep_at_most > 16) { (void)fail(RK_ERR_INVALID, "rk_translated_work_bytes: dna_words=%u, keep_at_most=%u", dna_words, keep_at_most); return 0; }
    if (n_reads >= (1ull << 32)) { (void)fail(RK_ERR_INVALID, "rk_translated_work_bytes: n_reads too large"); return 0; }
    return translated_work(n_reads, dna_words, keep_at_most).total;
}

extern "C" int rk_place_packed_device_translated(rk_db *db, const rk_params *p, uint64_t n_reads, const uint32_t *d_dna, uint32_t dna_words,
                                                 const uint32_t *d_dna_lens, uint32_t fixed_len, const uint32_t *d_dna_flags, const rk_result *d_out,
                                                 uint8_t *d_frame, void *d_work, uint64_t work_bytes, void *stream) {
    const char *who = "rk_place_packed_device_translated";
    int rc = translated_handle(db, who);
    if (rc) return rc;
    // every test the calls below would make, before the first launch: an error leaves the caller's arrays as they are
    if (!d_out) return fail(RK_ERR_INVALID, "%s: null argument", who);
    rc = check_params(p);
    if (rc) return rc;
    if (n_reads == 0) return RK_OK;
    if (!d_dna || dna_words == 0 || dna_words > 0x7FFFFFFu) return fail(RK_ERR_INVALID, "%s: null packed reads", who);
    if (!result_complete(d_out) || !d_frame) return fail(RK_ERR_INVALID, "%s: null result array", who);
    rc = check_fixed_len(who, d_dna_lens, fixed_len, 2, dna_words);
    if (rc) return rc;
    if (d_dna_flags && d_dna_flags == d_out->flags) return fail(RK_ERR_INVALID, "%s: d_dna_flags must not be the output flag array (every frame reads it)", who);
    if (n_reads >= (1ull << 32)) return fail(RK_ERR_INVALID, "%s: n_reads too large", who);
    char *base = (char *)d_work;
    const TranslatedWork L = translated_work(n_reads, dna_words, p->keep_at_most, base);
    if (!d_work || work_bytes < L.total)
        return fail(RK_ERR_INVALID, "%s: workspace of %llu bytes, %llu needed (rk_translated_work_bytes)", who, (unsigned long long)(d_work ? work_bytes : 0),
                    (unsigned long long)L.total);
    HIP_TRY(hipSetDevice(db->info.device));
    hipStream_t s = (hipStream_t)stream;
    uint32_t *aa = (uint32_t *)base, *aa_lens = (uint32_t *)(base + L.lens);
    for (uint32_t f = 0; f < 6; f++) {
        rc = rk_translate_packed_device(db, f, n_reads, d_dna, dna_words, d_dna_lens, fixed_len, aa, L.aa_words, aa_lens, s);
        if (rc) return rc;
        // (the placement kernels take BAD_CHAR / AMBIGUOUS / TOO_LONG from d_flags_in and nothing else: the DNA packer's TOO_SHORT,
        //  which speaks of bases, ends here; TOO_SHORT of the result is the frame's own, R < k residues)
        rc = rk_place_packed_device(db, p, n_reads, aa, L.aa_words, aa_lens, 0, d_dna_flags, nullptr, nullptr, f == 0 ? d_out : &L.cand, s);
        if (rc) return rc;
        if (f == 0) {
            hipLaunchKernelGGL(init_frame_kernel, dim3(strand_blocks(db, n_reads)), dim3(256), 0, s, (const unsigned char *)d_out->n_rows, d_frame, (u64)n_reads);
            HIP_TRY(hipGetLastError());
        } else {
            rc = rk_merge_frames_device(db, p->keep_at_most, n_reads, d_out, d_frame, &L.cand, f, s);
            if (rc) return rc;
        }
    }
    return RK_OK;
}

// rk_count_work_device: the work a batch asks of the database (count_work_kernel), for callers that want the reference's own
// diagnostics -- k-mers looked up, k-mers found, row entries walked -- next to the placements.  Opt-in and separate: the placement
// kernels carry no counters.
template <int BITS>
static void launch_count(const rk_db *db, const uint32_t *d_packed, uint32_t wpr, const uint32_t *d_lens, uint32_t fixed_len, const uint32_t *d_flags_in,
                         uint64_t n_reads, unsigned long long *d_out, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_reads + 3) / 4, (uint64_t)db->cu_count * 8);
    switch (db->info.table_mode) {
    case RK_TABLE_DIRECT: hipLaunchKernelGGL((count_work_kernel<BITS, TM_COMPACT>), dim3(blocks), dim3(256), 0, s, db->view, d_packed, wpr, d_lens, fixed_len, d_flags_in, n_reads, d_out); break;
    case RK_TABLE_DIRECT8: hipLaunchKernelGGL((count_work_kernel<BITS, TM_DIRECT8>), dim3(blocks), dim3(256), 0, s, db->view, d_packed, wpr, d_lens, fixed_len, d_flags_in, n_reads, d_out); break;
    default: hipLaunchKernelGGL((count_work_kernel<BITS, TM_HASH>), dim3(blocks), dim3(256), 0, s, db->view, d_packed, wpr, d_lens, fixed_len, d_flags_in, n_reads, d_out); break;
    }
}
extern "C" int rk_count_work_device(rk_db *db, uint64_t n_reads, const uint32_t *d_packed, uint32_t words_per_read, const uint32_t *d_lens,
                                    uint32_t fixed_len, const uint32_t *d_flags_in, rk_work *d_out, void *stream) {
    if (!db || !d_out) return fail(RK_ERR_INVALID, "rk_count_work_device: null argument");
    HIP_TRY(hipSetDevice(db->info.device));
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(rk_work) == 3 * sizeof(unsigned long long), "rk_work is three 64-bit counters");
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(rk_work), s));
    if (n_reads == 0) return RK_OK;
    if (!d_packed || words_per_read == 0) return fail(RK_ERR_INVALID, "rk_count_work_device: null packed reads");
    if (check_fixed_len("rk_count_work_device", d_lens, fixed_len, db->info.bits_per_symbol, words_per_read)) return RK_ERR_INVALID;
    if (db->info.bits_per_symbol == 2) launch_count<2>(db, d_packed, words_per_read, d_lens, fixed_len, d_flags_in, n_reads, (unsigned long long *)d_out, s);
    else launch_count<5>(db, d_packed, words_per_read, d_lens, fixed_len, d_flags_in, n_reads, (unsigned long long *)d_out, s);
    HIP_TRY(hipGetLastError());
    return RK_OK;
}

static rk::PackSpec pack_spec(const Alphabet &A, uint32_t alphabet, uint32_t bits, uint32_t k, uint32_t words_per_read) {
    rk::PackSpec P;
    P.table = A.table; P.bits = bits; P.k = k; P.words_per_read = words_per_read;
    P.pad_char = alphabet == RK_ALPHABET_DNA ? 'A' : 'R';  // state 0 of either alphabet
    P.force_scalar = rk_knob("RK_PACK_SCALAR") != nullptr;  // developer / test knob
    return P;
}

#include "rk_hostpath_impl.h"
#include "rk_samples_impl.h"  // the tree handle, clade sums and KR distances

// AmbigSequenceKnife.initTables' char -> state part (AmbigSequenceKnife.java:103-130) on the host, for callers that would rather
// ship 2 / 5 bits per symbol over PCIe than 8: the same records, lengths and flags pack_reads_kernel produces (rk_pack_host.cpp:
// AVX2 + BMI2 blocks of 32 symbols where the machine has them, the table-driven loop otherwise).
static int pack_reads_threads(const rk::PackSpec &P, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off, uint32_t *packed,
                              uint32_t *lens, uint32_t *flags, uint32_t n_threads) {
    ForkJoin pool(host_threads(n_reads, n_threads) - 1);
    pool.run([&](unsigned part, unsigned parts) {
        rk::pack_reads_range(P, seq_ascii, seq_off, n_reads * part / parts, n_reads * (part + 1) / parts, 0, packed, lens, flags);
    });
    return RK_OK;
}

extern "C" int rk_pack_reads_host(const rk_db *db, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off, uint32_t words_per_read,
                                  uint32_t *packed, uint32_t *lens, uint32_t *flags, uint32_t n_threads) {
    if (!db || !seq_off || !packed || !lens || !flags || words_per_read == 0) return fail(RK_ERR_INVALID, "rk_pack_reads_host: null/zero argument");
    if (n_reads && !seq_ascii && seq_off[n_reads]) return fail(RK_ERR_INVALID, "rk_pack_reads_host: null reads");
    RK_GUARD_BEGIN
    Alphabet A;
    build_alphabet(db->info.alphabet, db->shape.convert_uo != 0, A);
    return pack_reads_threads(pack_spec(A, db->info.alphabet, db->info.bits_per_symbol, db->info.k, words_per_read), n_reads, seq_ascii, seq_off,
                              packed, lens, flags, n_threads);
    RK_GUARD_END("rk_pack_reads_host")
}

// The same without a database handle (and without a GPU): alphabet, --convertUO switch and k are all the packer needs.
extern "C" int rk_pack_reads(uint32_t alphabet, int convert_uo, uint32_t k, uint64_t n_reads, const uint8_t *seq_ascii, const uint64_t *seq_off,
                             uint32_t words_per_read, uint32_t *packed, uint32_t *lens, uint32_t *flags, uint32_t n_threads) {
    if (alphabet != RK_ALPHABET_DNA && alphabet != RK_ALPHABET_AA) return fail(RK_ERR_INVALID, "rk_pack_reads: alphabet must be 4 (DNA) or 20 (amino acids)");
    if (!seq_off || !packed || !lens || !flags || words_per_read == 0 || k == 0) return fail(RK_ERR_INVALID, "rk_pack_reads: null/zero argument");
    if (n_reads && !seq_ascii && seq_off[n_reads]) return fail(RK_ERR_INVALID, "rk_pack_reads: null reads");
    RK_GUARD_BEGIN
    Alphabet A;
    build_alphabet(alphabet, convert_uo != 0, A);
    return pack_reads_threads(pack_spec(A, alphabet, alphabet == RK_ALPHABET_DNA ? 2u : 5u, k, words_per_read), n_reads, seq_ascii, seq_off, packed,
                              lens, flags, n_threads);
    RK_GUARD_END("rk_pack_reads")
}

#include "rk_synth_impl.h"
#include "rk_image_impl.h"

#ifdef RK_STAMPS
// diagnostic builds only (scripts/stamps.py)
extern "C" int rk_debug_read_stamps(unsigned long long *out, int n_waves) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(rk::rk_stamp_buf), (size_t)n_waves * 16 * sizeof(unsigned long long)));  // (n_waves = 8192 reads both halves)
    return RK_OK;
}
#endif
