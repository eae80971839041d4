// rk_hostbuf_impl.h -- #included by rk_engine.hip ahead of rk_db: the grow-only buffers of a handle's host path (device memory and
// page-locked host memory next to the GPU), a result set made of them, and the workspace of one chunk in flight.  The pipeline that
// fills them is rk_hostpath_impl.h.  Not a header for anyone else: it uses the engine's fail().
#pragma once

namespace {
struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return RK_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RK_ERR_NOMEM : RK_ERR_HIP, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        cap = want;
        return RK_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() { return (T *)p; }
};

// The host CPUs next to a GPU (its PCI device's NUMA node, from sysfs), cut to what this process may run on: the staging threads of
// the host path and the page-locked buffers they fill are kept there (round 3 measured 2.0 - 2.6e8 reads/s for the same call
// depending on where the scheduler had put them).  `ok` false = unknown / one node / nothing left after the cut: nothing is pinned.
struct NodeCpus {
    cpu_set_t set;
    bool ok = false;
    int node = -1;
};
const NodeCpus &gpu_node_cpus(int device) {
    static std::mutex mu;
    static std::map<int, NodeCpus> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    NodeCpus nc;
    CPU_ZERO(&nc.set);
    char bus[64] = "";
    if (rk_knob("RK_NO_NUMA")) return known.emplace(device, nc).first->second;  // developer knob (A/B)
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) == hipSuccess && bus[0]) {
        for (char *c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);
        int node = -1;
        { std::ifstream f(std::string("/sys/bus/pci/devices/") + bus + "/numa_node"); if (f) f >> node; }
        std::string list;
        if (node >= 0) { std::ifstream f("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist"); if (f) std::getline(f, list); }
        cpu_set_t allowed;
        CPU_ZERO(&allowed);
        if (!list.empty() && sched_getaffinity(0, sizeof(allowed), &allowed) == 0) {
            int n_set = 0;
            const char *q = list.c_str();
            while (*q) {  // "0-23,96-119"
                char *e;
                long a = strtol(q, &e, 10), b = a;
                if (e == q) break;
                if (*e == '-') { q = e + 1; b = strtol(q, &e, 10); }
                for (long c = a; c <= b && c < CPU_SETSIZE; c++)
                    if (CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &nc.set); n_set++; }
                q = (*e == ',') ? e + 1 : e;
                if (*e != ',' ) break;
            }
            nc.ok = n_set >= 4 && n_set < CPU_COUNT(&allowed);  // (all of the allowed CPUs on that node: nothing to choose)
            nc.node = node;
        }
    } else {
        (void)hipGetLastError();
    }
    return known.emplace(device, nc).first->second;
}
void pin_this_thread(const NodeCpus *nc) {
    if (nc && nc->ok) (void)pthread_setaffinity_np(pthread_self(), sizeof(nc->set), &nc->set);
}

struct PinBuf {  // page-locked host staging, grow-only
    void *p = nullptr;
    size_t cap = 0;
    // (node: allocated by a short-lived thread that runs next to the GPU, so that the pages -- pinned as they are allocated -- come
    //  from that node's memory; the caller's own thread is never moved)
    int reserve(size_t n, const NodeCpus *node = nullptr, int device = 0) {
        if (n <= cap) return RK_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 4 + 256;
        hipError_t e = hipSuccess;
        bool done = false;
        if (node && node->ok) {
            try {
                std::thread t([&]() {
                    pin_this_thread(node);
                    (void)hipSetDevice(device);
                    e = hipHostMalloc(&p, want, hipHostMallocDefault);
                });
                t.join();
                done = true;
            } catch (...) {  // no thread to be had: allocate here
            }
        }
        if (!done) e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RK_ERR_NOMEM : RK_ERR_HIP, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        cap = want;
        return RK_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() { return (T *)p; }
};

// The arrays of a result set -- n_rows | branch | score | lwr | flags, and the frame bytes of the translated path -- each in a buffer
// of its own: ResultBufs<GrowBuf> on the device, ResultBufs<PinBuf> page-locked on the host.  This and work_result() (rk_engine.hip:
// a result set inside a caller's block) are the two places that write the five arrays out.
template <class Buf>
struct ResultBufs {
    Buf nrows, branch, score, lwr, flags, frames;
    template <class... Where>  // (PinBuf: node, device)
    int reserve(uint64_t n, uint32_t K, bool with_frames, Where... where) {
        int rc;
        if ((rc = nrows.reserve(n, where...)) || (rc = branch.reserve(n * K * 2, where...)) || (rc = score.reserve(n * K * 4, where...)) ||
            (rc = lwr.reserve(n * K * 8, where...)) || (rc = flags.reserve(n * 4, where...)))
            return rc;
        return with_frames ? frames.reserve(n, where...) : RK_OK;
    }
    void release() { for (Buf *b : {&nrows, &branch, &score, &lwr, &flags, &frames}) b->release(); }
    rk_result view() { return rk_result{nrows.template as<uint8_t>(), branch.template as<uint16_t>(), score.template as<float>(), lwr.template as<double>(), flags.template as<uint32_t>()}; }
    uint8_t *frame() { return frames.template as<uint8_t>(); }
    // rows [0, n) of this set -> rows [r0, r0 + n) of dst, asynchronously on the stream (dst_frame null: no frame bytes)
    hipError_t download(hipStream_t s, const rk_result &dst, uint8_t *dst_frame, uint64_t r0, uint64_t n, uint32_t K) {
        for (const Field &f : fields(dst, dst_frame, K)) {
            if (!f.dst) continue;
            const hipError_t e = hipMemcpyAsync(f.dst + r0 * f.per_read, f.src, n * f.per_read, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // rows [lo, lo + c) of this (host) set -> rows [r0 + lo, r0 + lo + c) of dst
    void copy_range(const rk_result &dst, uint8_t *dst_frame, uint64_t r0, uint64_t lo, uint64_t c, uint32_t K) {
        for (const Field &f : fields(dst, dst_frame, K))
            if (f.dst) memcpy(f.dst + (r0 + lo) * f.per_read, f.src + lo * f.per_read, c * f.per_read);
    }

  private:
    struct Field { const char *src; char *dst; size_t per_read; };
    std::array<Field, 6> fields(const rk_result &dst, uint8_t *dst_frame, uint32_t K) {
        return {{{(const char *)nrows.p, (char *)dst.n_rows, 1}, {(const char *)branch.p, (char *)dst.branch, (size_t)K * 2},
                 {(const char *)score.p, (char *)dst.score, (size_t)K * 4}, {(const char *)lwr.p, (char *)dst.lwr, (size_t)K * 8},
                 {(const char *)flags.p, (char *)dst.flags, 4}, {(const char *)frames.p, (char *)dst_frame, 1}}};
    }
};
}  // namespace

// the result set of reads r0 .. of a result set of K rows a read
static rk_result result_slice(const rk_result &r, uint64_t r0, uint32_t K) {
    return rk_result{r.n_rows + r0, r.branch + r0 * K, r.score + r0 * K, r.lwr + r0 * K, r.flags + r0};
}

// One chunk of the host path in flight: its input and its result set on the device, page-locked staging for callers that hand over
// pageable memory (a JVM heap array, a numpy array: copies to / from it run on a few host threads, the DMA itself is then
// asynchronous and overlaps the other workspaces' chunks), and the stream all of it runs on.  Grow-only, kept in the rk_db.
struct rk_workspace {
    GrowBuf ascii, off, packed, lens, flags;
    GrowBuf weights;              // the chunk's weights (masses sink)
    GrowBuf members;              // the chunk's membership entries (masses sink, per-sample form): sample | read - lo | weight
    ResultBufs<GrowBuf> res;      // (with the frame bytes: rk_place_batch_translated)
    GrowBuf strands, translated;  // the workspaces of rk_place_packed_device_strands / _translated for a chunk
    PinBuf h_ascii, h_off, h_packed, h_members;
    ResultBufs<PinBuf> h_res;
    bool pending = false;         // results of the last chunk are still in the staging buffers
    uint64_t pend_r0 = 0, pend_n = 0;
    hipStream_t stream = nullptr;
    void release() {
        for (GrowBuf *b : {&ascii, &off, &packed, &lens, &flags, &weights, &members, &strands, &translated}) b->release();
        for (PinBuf *b : {&h_ascii, &h_off, &h_packed, &h_members}) b->release();
        res.release();
        h_res.release();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};
