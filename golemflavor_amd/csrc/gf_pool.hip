// gf_pool.hip -- the per-device pools behind every model, sampler and read-back: the device's identity, idle streams, copy streams
// and constant blocks, and the unitarity workspace that belongs to a stream.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "gf_devcache.h"                // large device allocations are cached, not handed back to the driver
#include "gf_host.h"
#include "gf_pool.h"

namespace {

// Per-device cache of what a model needs from the runtime: the device's identity, a non-blocking stream and
// one small block of device memory for its constant tables.  A grid scan creates and destroys hundreds of
// models (one per grid point); hipStreamCreate / hipMalloc / hipFree / hipGetDeviceProperties cost ~1 ms each
// and hipFree synchronises the device, so destroyed models hand their stream and block back to this pool.
constexpr size_t POOL_MAX_ITEMS = 1024;
constexpr size_t WORK_CACHE_MAX_BYTES = (size_t)8 << 30;     // idle unitarity workspaces kept per device (of 288 GB)

// What the unitarity verdict of a batch needs besides the caller's arrays (gf_bsm.hip, gf_unitarity.hip): the arbitration
// queue, the walker queue and side buffer of the deferred tier 2, and one pinned word through which the arbitration kernel
// tells the host how long its queue was.  It belongs to the STREAM, not to the model: launches on one stream run in order,
// so every model that launches there can use the same workspace -- the 64 per-grid-point models of a texture scan, which
// propagate their chains one after the other on the sampler's stream, share one instead of allocating (and, worse,
// freeing: hipFree ~0.25 ms and a device synchronisation each) three buffers apiece -- and it stays with the stream when
// the stream goes back to the pool.
struct UniWork {
    std::mutex mu;                 // held from sizing the workspace to the last launch that uses it
    GfArbQueue* d_uq = nullptr;    // [uq_cap] walkers with their undecided bins
    GfUniQueue* d_wq = nullptr;    // [wq_cap] walkers
    double* d_t2sn = nullptr;      // [wq_cap][18]
    unsigned int* h_seen = nullptr;
    int64_t uq_cap = 0, wq_cap = 0;
    size_t bytes() const
    {
        return (d_uq ? sizeof(GfArbItem) * (size_t)uq_cap : 0) + (d_wq ? sizeof(unsigned long long) * (size_t)wq_cap : 0) +
               (d_t2sn ? sizeof(double) * 18 * (size_t)wq_cap : 0);
    }
    void release()
    {
        if (d_uq) (void)gf_cached_free(d_uq);
        if (d_wq) (void)gf_cached_free(d_wq);
        if (d_t2sn) (void)gf_cached_free(d_t2sn);
        d_uq = nullptr; d_wq = nullptr; d_t2sn = nullptr; uq_cap = wq_cap = 0;
    }
    // the pinned words the arbitration kernel and the host share, allocated on first use
    hipError_t ensure_seen()
    {
        if (h_seen) return hipSuccess;
        const hipError_t e = hipHostMalloc((void**)&h_seen, 64, hipHostMallocDefault);
        if (e != hipSuccess) { h_seen = nullptr; return e; }
        h_seen[0] = 0xffffffffu;           // nothing seen yet: the first launch takes the full grid
        h_seen[1] = 0;                     // host-only flag: full grids on request (gf_internal_full_arbitration_grids)
        h_seen[2] = 0;                     // written by k_uni_resolve: a queue overflowed (check_queue_overflow)
        h_seen[3] = h_seen[4] = 0;         // running totals: pairs arbitrated, arbitration launches (gf_internal_uni_stats)
        return hipSuccess;
    }
};

struct DevicePool {
    int state = 0;                 // 0 unknown, 1 gfx950, -1 something else
    int cus = 256;
    std::vector<hipStream_t> streams;
    std::vector<hipStream_t> copy_streams;               // high-priority streams for the large read-backs (pool_copy_stream)
    std::vector<void*> blocks;
    std::unordered_map<hipStream_t, UniWork*> work;      // never erased while the stream lives
};
std::mutex g_pool_mu;
DevicePool g_pool[POOL_MAX_DEVICES];

// the last idle item of one of the device's pools, or a new one from `create`
template <typename T, typename Create>
hipError_t pool_take(std::vector<T> DevicePool::*idle, int device, T* out, Create create)
{
    *out = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        std::vector<T>& v = g_pool[device].*idle;
        if (!v.empty()) { *out = v.back(); v.pop_back(); }
    }
    return *out ? hipSuccess : create(out);
}

// A stream for a read-back that is to run BESIDE kernels of another stream.  The runtime multiplexes its streams onto a handful of
// hardware queues, round-robin, and a copy stream that shares the compute stream's queue has its barrier packets queued behind the
// kernels enqueued there.  Streams of another PRIORITY get hardware queues of their own, so the copy streams are created with the
// greatest priority and kept in a pool of their own.  (Built while hunting the read-backs that ran at half speed; the cause turned out
// to be the driver wiping freed memory -- gf_devcache.h -- and the priority made no measurable difference: kept, it is the safer
// arrangement.  GF_COPY_STREAM_PLAIN=1: a stream like any other.)
hipError_t pool_copy_stream(int device, hipStream_t* stream)
{
    return pool_take(&DevicePool::copy_streams, device, stream, [](hipStream_t* st) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        static const bool plain = gf_internal_env("GF_COPY_STREAM_PLAIN", 0) != nullptr;            // A/B: a stream like any other
        return (plain || least == greatest) ? hipStreamCreateWithFlags(st, hipStreamNonBlocking)
                                            : hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest);
    });
}

// the stream's workspace, created if it has none yet (NULL: out of memory)
UniWork* work_for(int device, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    UniWork*& w = g_pool[device].work[stream];
    if (!w) w = new (std::nothrow) UniWork();
    return w;
}

// the stream's workspace if it has one
UniWork* work_of(int device, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool[device].work.find(stream);
    return it != g_pool[device].work.end() ? it->second : nullptr;
}

// The arbitration queue must hold every walker of one piece of the batch (gf_launch_bsm cuts AoS batches into pieces of
// uq_cap walkers; SoA batches go in one piece).  Items are walkers since round 3 (16 B each: index + mask of undecided bins),
// not (walker, bin) pairs: a queue for the 8.4 M walkers of a piece is 128 MiB where round 2's was 1 GiB for 6.7 M.
constexpr int64_t UQ_MAX_ITEMS = 1 << 23;
// from this batch size on (one lane per walker in the evaluation kernel) tier 2 runs as its own compact kernel
constexpr int64_t GF_TIER2_SPLIT_MIN = 65536;
constexpr int64_t WQ_MAX_WALKERS = 1 << 23;    // per piece: 8.4 M walkers, 1.2 GB of side buffer

// `items_limit` (out): how many items of the queue a piece of this batch may use (its capacity, or GF_UQ_MAX_ITEMS if smaller)
int ensure_uq(UniWork* w, hipStream_t st, int layout, int64_t n, int64_t* items_limit)
{
    int64_t need = n;                         // one item per walker
    int64_t max_items = UQ_MAX_ITEMS;
    if (const char* e = gf_internal_env("GF_UQ_MAX_ITEMS", 0)) {     // tests: a small queue, so that a modest batch is cut into pieces
        const long long v = std::atoll(e);
        if (v >= 4096 && v < UQ_MAX_ITEMS) max_items = v;
    }
    if (layout == GF_LAYOUT_AOS && need > max_items) need = max_items;
    *items_limit = layout == GF_LAYOUT_AOS ? max_items : (int64_t)0x7fffffffffffLL;
    if (need > 0xffffffffLL)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "a structure-of-arrays batch of %lld walkers with a status array exceeds the arbitration queue", (long long)n);
    GF_HIP(w->ensure_seen());
    int64_t cap = w->uq_cap ? w->uq_cap : 4096;
    while (cap < need) cap *= 2;
    // the walker queue (and the side buffer, 144 B per walker) of the deferred tier 2: one piece of the batch -- gf_launch_bsm
    // cuts an AoS batch into pieces that fit both queues
    const bool defer = n >= GF_TIER2_SPLIT_MIN;
    int64_t need_w = defer ? n : 0;
    if (layout == GF_LAYOUT_AOS && need_w > WQ_MAX_WALKERS) need_w = WQ_MAX_WALKERS;
    if (need_w > w->wq_cap) {                 // grow at least geometrically
        const int64_t twice = 2 * w->wq_cap < WQ_MAX_WALKERS ? 2 * w->wq_cap : WQ_MAX_WALKERS;
        if (layout == GF_LAYOUT_AOS && twice > need_w) need_w = twice;
    }
    if (cap == w->uq_cap && need_w <= w->wq_cap) return GF_OK;
    GF_HIP(hipStreamSynchronize(st));          // earlier launches may still use the old buffers
    GfUniQueue hdr = {0, 0, 0, 0, {0}};
    if (cap != w->uq_cap) {
        if (w->d_uq) (void)gf_cached_free(w->d_uq);
        w->d_uq = nullptr; w->uq_cap = 0;
        GF_HIP(gf_cached_malloc((void**)&w->d_uq, sizeof(GfArbQueue) + sizeof(GfArbItem) * (size_t)cap));
        GfArbQueue ah;
        std::memset(&ah, 0, sizeof(ah));
        ah.cap = (unsigned int)cap;
        GF_HIP(hipMemcpyAsync(w->d_uq, &ah, offsetof(GfArbQueue, items), hipMemcpyHostToDevice, st));
        GF_HIP(hipStreamSynchronize(st));
        w->uq_cap = cap;
    }
    if (need_w > w->wq_cap) {
        if (w->d_wq) (void)gf_cached_free(w->d_wq);
        if (w->d_t2sn) (void)gf_cached_free(w->d_t2sn);
        w->d_wq = nullptr; w->d_t2sn = nullptr; w->wq_cap = 0;
        GF_HIP(gf_cached_malloc((void**)&w->d_wq, sizeof(GfUniQueue) + sizeof(unsigned long long) * (size_t)need_w));
        GF_HIP(gf_cached_malloc((void**)&w->d_t2sn, sizeof(double) * 18 * (size_t)need_w));
        hdr.cap = (unsigned int)need_w;
        GF_HIP(hipMemcpyAsync(w->d_wq, &hdr, offsetof(GfUniQueue, items), hipMemcpyHostToDevice, st));
        GF_HIP(hipStreamSynchronize(st));
        w->wq_cap = need_w;
    }
    return GF_OK;
}

bool pool_has(int device) { return device >= 0 && device < POOL_MAX_DEVICES; }

// a stream of one of the device's pools for a caller outside this file
int borrow(int device, void** stream, hipError_t (*take)(int, hipStream_t*), const char* what)
{
    if (!pool_has(device) || !stream) return GF_ERR_INVALID_ARG;
    hipStream_t st = nullptr;
    const hipError_t e = take(device, &st);
    if (e != hipSuccess) return gf_hip_fail(e, what);
    *stream = (void*)st;
    return GF_OK;
}

}  // namespace

int pool_device(int device, int* cus)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1 || device < 0 || device >= count || device >= POOL_MAX_DEVICES) {
        (void)hipGetLastError();
        return gf_fail_msg(GF_ERR_NO_DEVICE, "no HIP device %d (found %d)", device, count);
    }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    DevicePool& dp = g_pool[device];
    if (dp.state == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); dp.state = -1; }
        else {
            dp.state = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : -1;
            dp.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
    }
    if (dp.state != 1) return gf_fail_msg(GF_ERR_NO_DEVICE, "device %d is not gfx950", device);
    *cus = dp.cus;
    return GF_OK;
}

hipError_t pool_stream(int device, hipStream_t* stream)
{
    return pool_take(&DevicePool::streams, device, stream, [](hipStream_t* st) { return hipStreamCreateWithFlags(st, hipStreamNonBlocking); });
}

hipError_t pool_block(int device, void** block)
{
    return pool_take(&DevicePool::blocks, device, block, [](void** b) { return gf_cached_malloc(b, CONST_BLOCK_BYTES); });
}

void pool_release(int device, hipStream_t stream, void* block)
{
    UniWork* drop = nullptr;
    bool trim = false;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        DevicePool& dp = g_pool[device];
        if (stream) {
            // the stream's workspace goes back to the pool with it, unless the idle workspaces of this device already hold
            // WORK_CACHE_MAX_BYTES: then its buffers are released (the small bookkeeping object stays)
            auto it = dp.work.find(stream);
            if (it != dp.work.end() && it->second) {
                size_t total = 0;
                for (auto& kv : dp.work) if (kv.second) total += kv.second->bytes();
                if (dp.streams.size() >= POOL_MAX_ITEMS) { drop = it->second; dp.work.erase(it); }
                else if (total > WORK_CACHE_MAX_BYTES) { drop = it->second; trim = true; }
            }
        }
        if (stream && dp.streams.size() < POOL_MAX_ITEMS) { dp.streams.push_back(stream); stream = nullptr; }
        if (block && dp.blocks.size() < POOL_MAX_ITEMS) { dp.blocks.push_back(block); block = nullptr; }
    }
    if (drop) {
        std::lock_guard<std::mutex> lk(drop->mu);
        drop->release();
        if (!trim) { if (drop->h_seen) (void)hipHostFree(drop->h_seen); }
    }
    if (drop && !trim) delete drop;
    if (stream) (void)hipStreamDestroy(stream);
    if (block) (void)gf_cached_free(block);
}

int check_queue_overflow(int device, hipStream_t st)
{
    UniWork* w = work_of(device, st);
    if (!w || !w->h_seen) return GF_OK;
    if (__atomic_exchange_n(&w->h_seen[2], 0u, __ATOMIC_RELAXED) == 0u) return GF_OK;
    return gf_fail_msg(GF_ERR_QUEUE_OVERFLOW, "a unitarity queue overflowed: (walker, bin) pairs were dropped and the status array of that batch is "
                                              "incomplete (the host cuts batches to fit the queues: this is a library bug)");
}

int pool_lease_workspace(int device, hipStream_t st, int layout, int64_t n, GfUniLease* lease)
{
    UniWork* w = work_for(device, st);
    if (!w) return GF_ERR_ALLOC;
    const int ro = check_queue_overflow(device, st);            // of an earlier asynchronous launch on this stream
    if (ro != GF_OK) return ro;
    lease->lock = std::unique_lock<std::mutex>(w->mu);
    int64_t limit = 0;
    const int rq = ensure_uq(w, st, layout, n, &limit);
    if (rq != GF_OK) return rq;
    lease->d_uq = w->d_uq;
    lease->uq_items = w->uq_cap < limit ? w->uq_cap : limit;
    lease->d_wq = n >= GF_TIER2_SPLIT_MIN ? w->d_wq : nullptr;
    lease->wq_cap = w->wq_cap;
    lease->d_t2sn = w->d_t2sn;
    lease->h_seen = w->h_seen;
    return GF_OK;
}

extern "C" {

// internal: a second stream from the device's pool (gf_sampler_host.hip: copies that overlap the sampler stream's kernels)
int gf_internal_borrow_stream(int device, void** stream) { return borrow(device, stream, pool_stream, "pool_stream"); }
// internal: a stream for a large read-back that overlaps another stream's kernels (pool_copy_stream: hardware queues of its own)
int gf_internal_borrow_copy_stream(int device, void** stream) { return borrow(device, stream, pool_copy_stream, "pool_copy_stream"); }

// idle (synchronised) streams only.  A stream goes back with its workspace and under the pool's cap (pool_release); a copy stream has
// no workspace, and its pool has never had a cap (POOL_MAX_ITEMS does not apply to it)
void gf_internal_return_stream(int device, void* stream)
{
    if (pool_has(device) && stream) pool_release(device, (hipStream_t)stream, nullptr);
}
void gf_internal_return_copy_stream(int device, void* stream)
{
    if (!pool_has(device) || !stream) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool[device].copy_streams.push_back((hipStream_t)stream);
}

// internal: while `on`, every arbitration launch on `stream` takes the full grid whatever the previous one found
// (gf_launch_uni_resolve); a workspace is created if the stream has none yet
void gf_internal_full_arbitration_grids(int device, void* stream, int on)
{
    if (!pool_has(device)) return;
    UniWork* w = work_for(device, (hipStream_t)stream);
    if (!w) return;
    std::lock_guard<std::mutex> lk(w->mu);
    if (w->ensure_seen() != hipSuccess) { (void)hipGetLastError(); return; }
    w->h_seen[1] = on ? 1u : 0u;
}

// internal (gf_sampler_host.hip): the overflow report for launches the sampler put on `stream` and has just synchronised
int gf_internal_check_overflow(int device, void* stream)
{
    if (!pool_has(device)) return GF_ERR_INVALID_ARG;
    return check_queue_overflow(device, (hipStream_t)stream);
}

// internal, diagnostics (tools/): {pairs in the last arbitration launch, pairs arbitrated so far, launches so far} of the
// model's stream (wrapping 32-bit counters); synchronise first
int gf_internal_uni_stats(gf_model* m, unsigned int out[3])
{
    if (!m || !out) return GF_ERR_INVALID_ARG;
    out[0] = out[1] = out[2] = 0;
    int device = 0;
    void* stream = nullptr;
    gf_model_peek_stream(m, &device, &stream);
    if (!stream) return GF_OK;
    UniWork* w = work_of(device, (hipStream_t)stream);
    if (w && w->h_seen) { out[0] = w->h_seen[0]; out[1] = w->h_seen[3]; out[2] = w->h_seen[4]; }
    return GF_OK;
}

// internal, diagnostics (tools/arb_probe.py): the items of the last arbitration launch on the model's stream, still in the
// queue's memory after the kernel re-armed it: items_out[min(count, max)][2] = (walker, mask of undecided bins)
int gf_internal_uni_dump(gf_model* m, unsigned long long* items_out, unsigned int max, unsigned int* count)
{
    if (!m || !items_out || !count) return GF_ERR_INVALID_ARG;
    int device = 0;
    void* stream = nullptr;
    gf_model_peek_stream(m, &device, &stream);
    if (!stream) return GF_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    UniWork* w = work_of(device, st);
    if (!w || !w->h_seen || !w->d_uq) return GF_ERR_INVALID_ARG;
    GF_HIP(hipStreamSynchronize(st));
    unsigned int n = w->h_seen[0];
    *count = n;
    if (n > max) n = max;
    if (n > (unsigned int)w->uq_cap) n = (unsigned int)w->uq_cap;
    if (n) {
        GF_HIP(hipMemcpyAsync(items_out, w->d_uq->items, sizeof(GfArbItem) * n, hipMemcpyDeviceToHost, st));
        GF_HIP(hipStreamSynchronize(st));
    }
    return GF_OK;
}

// Release what the library keeps cached on `device` between uses: the unitarity workspaces (arbitration queue, walker queue,
// side buffer: up to 8 GiB in all) of pooled, idle streams, and the pooled constant blocks.  Streams in use keep theirs.
// *released_bytes (may be NULL): device memory handed back.  For long-lived processes that ran one large scan and go on
// with small work.
int gf_device_trim(int device, size_t* released_bytes)
{
    int cus = 0;
    const int rc = pool_device(device, &cus);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(device));
    // the idle streams leave the pool while their workspaces are released (nobody can pick one up half-way) and return after
    std::vector<hipStream_t> streams;
    std::vector<UniWork*> idle;
    std::vector<void*> blocks;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        DevicePool& dp = g_pool[device];
        streams.swap(dp.streams);
        for (hipStream_t st : streams) {
            auto it = dp.work.find(st);
            if (it != dp.work.end() && it->second) idle.push_back(it->second);
        }
        blocks.swap(dp.blocks);
    }
    size_t total = gf_devcache_trim(device);            // the cached large buffers (gf_devcache.h) go back to the driver too
    for (UniWork* w : idle) {
        std::lock_guard<std::mutex> lk(w->mu);
        total += w->bytes();
        w->release();
    }
    for (void* b : blocks) { (void)gf_cached_free(b); total += CONST_BLOCK_BYTES; }
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        DevicePool& dp = g_pool[device];
        for (hipStream_t st : streams) dp.streams.push_back(st);
    }
    // the pinned staging slots of large device-to-host reads (host memory: not part of released_bytes, which counts device
    // memory); a read in progress keeps them
    gf_internal_d2h_ring_trim(device);
    if (released_bytes) *released_bytes = total;
    return GF_OK;
}

}  // extern "C"
