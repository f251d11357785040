// gf_readback.hip -- device memory into host memory: the ring of pinned slots with the host threads that empty it, the direct copy
// into registered memory, and the helpers that make a destination ready (page mapping, registration).  Host code and one copy kernel;
// no gf_model here: every entry point takes a device and a stream.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <sys/mman.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "gf_devcache.h"                // gf_internal_pinned_d2h_rate's device buffer; the pinned slots are hipHostMalloc'ed and stay outside the cache
#include "gf_host.h"

// ---- large device-to-host copies: a ring of pinned slots + host threads ----------------------------------------------------
// hipMemcpy into pageable memory is at the mercy of the runtime's own choice between pinning the destination in place and
// staging: measured on one box, in one process, five 1.9 GB read-backs into fresh arrays ran at 42, 52, 10, 51 and 15 GB/s
// (tools/numa_probe.py; not a NUMA effect: the same with the threads bound to either node).  So reads of 16 MiB and more bring
// their own staging: eight pinned 16 MiB slots per device (allocated on first use, kept until gf_device_trim), the DMA engine fills
// slot c while host threads copy slot c - 1 (and c - 2 ...) into the destination -- which also touches the destination's pages for
// the first time, from several threads, so no separate page-mapping pass is needed.  PCIe runs at its pinned-memory rate whatever
// the destination is.
namespace {
constexpr size_t D2H_SLOT = (size_t)16 << 20;
constexpr int D2H_SLOTS = 8;
constexpr size_t D2H_RING_MIN = (size_t)16 << 20;     // the synchronous copies take the ring from this size on
constexpr size_t D2H_DIRECT_PIECE = (size_t)64 << 20; // a gated copy into registered memory: the gate is asked once per piece
struct D2HRing {
    std::mutex mu;                                   // one large read-back at a time per device
    void* slot[D2H_SLOTS] = {};
    hipEvent_t ev[D2H_SLOTS] = {};
};
D2HRing g_d2h[POOL_MAX_DEVICES];

// GF_NO_D2H_PIPELINE=1: the synchronous copies leave everything to the runtime (diagnostics / A-B)
bool ring_off()
{
    static const bool off = gf_internal_env("GF_NO_D2H_PIPELINE", 0) != nullptr;
    return off;
}

// The host threads that empty the slots: a pool created on first use and kept (starting seven threads per 16 MiB slot cost
// 0.15-0.2 ms against the 0.33 ms the copy itself takes).  A job is a packed source of nrows x width bytes going to rows
// `dpitch` apart; it is cut into 1 MiB pieces that the workers and the calling thread take from a shared counter, so the
// pieces balance themselves whatever the row length.  Leaked on purpose at exit (the workers sleep on the condition
// variable); a forked child starts without a pool.
struct CopyPool {
    std::mutex mu;
    std::condition_variable wake, done;
    std::vector<std::thread> workers;
    char* dst = nullptr; const char* src = nullptr;
    size_t dpitch = 0, width = 0, total = 0, piece = 0, ntasks = 0;
    std::atomic<size_t> next{0};
    unsigned generation = 0, busy = 0;

    static void piece_copy(char* dst, size_t dpitch, const char* src, size_t width, size_t lo, size_t hi)
    {
        while (lo < hi) {                                          // [lo, hi) of the packed source, row by row
            const size_t r = lo / width, off = lo - r * width;
            const size_t n = (width - off) < (hi - lo) ? (width - off) : (hi - lo);
            std::memcpy(dst + r * dpitch + off, src + lo, n);
            lo += n;
        }
    }
    void take()
    {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= ntasks) return;
            const size_t lo = i * piece, hi = lo + piece < total ? lo + piece : total;
            piece_copy(dst, dpitch, src, width, lo, hi);
        }
    }
    void worker()
    {
        unsigned seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                wake.wait(lk, [&] { return generation != seen; });
                seen = generation;
            }
            take();
            std::lock_guard<std::mutex> lk(mu);
            if (--busy == 0) done.notify_one();
        }
    }
    void run(char* d, size_t dp, const char* s, size_t w, size_t nrows)
    {
        const size_t bytes = w * nrows;
        if (workers.empty() || bytes < ((size_t)2 << 20)) { piece_copy(d, dp, s, w, 0, bytes); return; }
        {
            std::lock_guard<std::mutex> lk(mu);
            dst = d; dpitch = dp; src = s; width = w; total = bytes;
            piece = (size_t)1 << 20;
            ntasks = (bytes + piece - 1) / piece;
            next.store(0, std::memory_order_relaxed);
            busy = (unsigned)workers.size();
            ++generation;
        }
        wake.notify_all();
        take();
        std::unique_lock<std::mutex> lk(mu);
        done.wait(lk, [&] { return busy == 0; });
    }
};
CopyPool* g_copy_pool = nullptr;
std::mutex g_copy_pool_mu;                        // one job at a time (the rings of two devices may drain concurrently)

void copy_rows(char* dst, size_t dpitch, const char* src, size_t width, size_t nrows)
{
    std::lock_guard<std::mutex> lk(g_copy_pool_mu);
    if (!g_copy_pool) {
        size_t nt = 0;
        if (const char* v = gf_internal_env("GF_D2H_THREADS", 0)) { const long k = std::atol(v); if (k >= 1 && k <= 64) nt = (size_t)k; }
        if (!nt) { const unsigned hw = std::thread::hardware_concurrency(); nt = hw >= 32 ? 8 : (hw >= 8 ? 4 : 1); }
        g_copy_pool = new CopyPool();
        for (size_t k = 1; k < nt; ++k) {
            g_copy_pool->workers.emplace_back([p = g_copy_pool] { p->worker(); });
            g_copy_pool->workers.back().detach();
        }
        static bool hooked = false;
        if (!hooked) { hooked = true; pthread_atfork(nullptr, nullptr, [] { g_copy_pool = nullptr; new (&g_copy_pool_mu) std::mutex(); }); }
    }
    g_copy_pool->run(dst, dpitch, src, width, nrows);
}

// Is the host range [p, p + span) REGISTERED memory (gf_host_register) or hipHostMalloc'ed -- memory the device can write itself?
// Asked once per read-back call (two attribute queries: the first byte and the last); GF_NO_DIRECT_D2H=1: always "no" (A/B).
// *alias: the device's address of p.
bool host_range_is_pinned(const void* p, size_t span, void** alias = nullptr)
{
    if (!p || span == 0) return false;
    static const bool off = gf_internal_env("GF_NO_DIRECT_D2H", 0) != nullptr;
    if (off) return false;
    const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + span - 1};
    for (const char* q : ends) {
        hipPointerAttribute_t a;
        std::memset(&a, 0, sizeof(a));
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain pageable memory: an error on some runtimes
        if (a.type != hipMemoryTypeHost) return false;                                                 // ... hipMemoryTypeUnregistered on others
    }
    if (alias) {
        *alias = nullptr;
        if (hipHostGetDevicePointer(alias, const_cast<void*>(p), 0) != hipSuccess || !*alias) { (void)hipGetLastError(); return false; }
    }
    return true;
}

// Rows of device memory into registered host memory by a KERNEL that stores through the host memory's device alias: 55-56 GB/s from 32
// workgroups (tools/experiments/d2h_kernel_probe.hip), and unaffected by what halves the runtime's DMA for ~0.6 s after a large hipFree
// (the driver wiping the freed memory with the DMA engine: tools/vram_realloc_probe4.py, profiles/r04/host_register.txt).  NOT the
// default (enqueue_d2h_rows): beside other kernels it costs them a dispatch each, and the device cache keeps the wipe from happening.
// A tile is 256 lanes x 16 elements of one row; few workgroups on purpose: the link is the bound.
template <typename T>
__global__ __launch_bounds__(256) void k_d2h_rows(T* __restrict__ dst, size_t dpitch_e, const T* __restrict__ src, size_t spitch_e,
                                                  size_t width_e, size_t height)
{
    constexpr size_t TILE = 256 * 16;
    const size_t tiles_per_row = (width_e + TILE - 1) / TILE, ntiles = tiles_per_row * height;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t r = t / tiles_per_row, c0 = (t - r * tiles_per_row) * TILE;
        const T* s = src + r * spitch_e + c0;
        T* d = dst + r * dpitch_e + c0;
        const size_t n = width_e - c0 < TILE ? width_e - c0 : TILE;
#pragma unroll 4
        for (size_t i = threadIdx.x; i < n; i += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(s + i), d + i);
    }
}
typedef double gf_v2d __attribute__((ext_vector_type(2)));

// enqueue on `st`: `height` rows of `width` bytes, `spitch` apart on the device, to the registered host rows `dpitch` apart behind
// `dst_alias` (their device address).
hipError_t enqueue_d2h_rows(hipStream_t st, void* dst_host, void* dst_alias, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height)
{
    // The runtime's DMA by default: it needs no compute unit, so it runs beside the sampler's and the post-processing kernels without
    // costing them a dispatch (the copy kernel beside them: C5 89 -> 177 us per half-step, C4's rows 33 GB/s).  The kernel is the
    // faster of the two only while the driver wipes freed memory with the DMA engine -- which the device cache (gf_devcache.h) now
    // keeps from happening.  GF_D2H_KERNEL=1: the kernel (A/B).
    static const bool dma = gf_internal_env("GF_D2H_KERNEL", 0) == nullptr;
    const bool words = ((width | dpitch | spitch | (size_t)(uintptr_t)dst_alias | (size_t)(uintptr_t)src) & 7u) == 0;
    if (dma || !words || !dst_alias)
        return height == 1 ? hipMemcpyAsync(dst_host, src, width, hipMemcpyDeviceToHost, st)
                           : hipMemcpy2DAsync(dst_host, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, st);
    static const int blocks = [] { const char* v = gf_internal_env("GF_D2H_KERNEL_BLOCKS", 0); const int k = v ? std::atoi(v) : 0; return k >= 1 && k <= 4096 ? k : 32; }();
    const bool wide = ((width | dpitch | spitch | (size_t)(uintptr_t)dst_alias | (size_t)(uintptr_t)src) & 15u) == 0;
    if (wide)
        hipLaunchKernelGGL(k_d2h_rows<gf_v2d>, dim3(blocks), dim3(256), 0, st, static_cast<gf_v2d*>(dst_alias), dpitch / 16,
                           static_cast<const gf_v2d*>(src), spitch / 16, width / 16, height);
    else
        hipLaunchKernelGGL(k_d2h_rows<double>, dim3(blocks), dim3(256), 0, st, static_cast<double*>(dst_alias), dpitch / 8,
                           static_cast<const double*>(src), spitch / 8, width / 8, height);
    return hipGetLastError();
}
}  // namespace

// ---- the ring pipeline ------------------------------------------------------------------------------------------------------------
// The calling thread issues chunk after chunk -- the DMA of a chunk into the next slot, then the slot's event -- and ONE consumer
// thread waits for each event and empties the slot into the destination (copy_rows).  A slot is reused once the consumer is done with
// it, so the DMA of chunk c runs while the host threads empty chunk c - 1.  Error text is only ever set by the calling thread (it is
// thread-local); the consumer reports through `failed`.
//
// A pipe may stay open over MANY blocks (gf_sampler_run_to_host): a chain that leaves the device block of steps by block of steps
// while it is sampled (62 blocks of 201 MB for the C5 scan at the reference's length) paid thread start, ring fill and ring drain 62
// times with a pipeline per block and reached 31 GB/s where the link gives 48 (profiles/r04/readback_overlap.txt).  _pipe_rows returns
// as soon as the block's chunks have been ISSUED, the next block's chunks follow without a gap, and only _close drains.
struct gf_d2h_pipe {
    int device = 0;
    hipStream_t st = nullptr;
    D2HRing* ring = nullptr;                // locked from pipe_start to pipe_finish
    struct Chunk { char* dst; size_t dpitch, width, nrows; } desc[D2H_SLOTS] = {};
    std::atomic<size_t> issued{0}, drained{0};
    std::atomic<int> failed{0}, closing{0};
    std::thread consumer;
    bool direct_pending = false;            // blocks went straight into a registered destination: pipe_finish waits for the stream
};

namespace {
// the consumer thread: chunk after chunk as they are issued, until a failure, or until the pipe closes with nothing left to empty
void pipe_consume(gf_d2h_pipe* p)
{
    for (size_t c = 0;; ++c) {
        while (p->issued.load(std::memory_order_acquire) <= c && !p->failed.load() && !p->closing.load()) std::this_thread::yield();
        if (p->failed.load() || p->issued.load(std::memory_order_acquire) <= c) return;       // (closing is set after the last issue)
        const int k = (int)(c % D2H_SLOTS);
        if (hipEventSynchronize(p->ring->ev[k]) != hipSuccess) { p->failed.store(1); return; }
        const gf_d2h_pipe::Chunk& d = p->desc[k];
        copy_rows(d.dst, d.dpitch, static_cast<const char*>(p->ring->slot[k]), d.width, d.nrows);
        p->drained.store(c + 1, std::memory_order_release);
    }
}

// The ring and the consumer thread are set up when the first chunk needs them: a pipe whose blocks all go straight into a registered
// destination never touches either (and a run does not start with 128 MiB of hipHostMalloc, 30 ms when it is the process's first and
// now and then several times that).
int pipe_start(gf_d2h_pipe* p)
{
    if (p->ring) return GF_OK;
    D2HRing* ring = &g_d2h[p->device];
    ring->mu.lock();                                      // one large read-back at a time per device; released by pipe_finish
    hipError_t e = hipSuccess;
    for (int k = 0; k < D2H_SLOTS && e == hipSuccess; ++k) {
        if (!ring->slot[k]) e = hipHostMalloc(&ring->slot[k], D2H_SLOT, hipHostMallocDefault);
        if (e == hipSuccess && !ring->ev[k]) e = hipEventCreateWithFlags(&ring->ev[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) { ring->mu.unlock(); return gf_hip_fail(e, "gf_internal_d2h: ring"); }
    p->ring = ring;
    p->consumer = std::thread(pipe_consume, p);
    return GF_OK;
}

// one chunk -- `nrows` rows of `width` bytes, a slot's worth at most -- into the next slot, once the consumer has emptied that slot
hipError_t pipe_issue(gf_d2h_pipe* p, char* dst, size_t dpitch, const char* src, size_t spitch, size_t width, size_t nrows)
{
    const size_t c = p->issued.load(std::memory_order_relaxed);
    while (c >= p->drained.load(std::memory_order_acquire) + D2H_SLOTS && !p->failed.load()) std::this_thread::yield();
    if (p->failed.load()) return hipSuccess;              // the consumer's failure: the caller sees `failed`
    const int k = (int)(c % D2H_SLOTS);
    p->desc[k] = {dst, dpitch, width, nrows};
    hipError_t e = nrows == 1 ? hipMemcpyAsync(p->ring->slot[k], src, width, hipMemcpyDeviceToHost, p->st)
                              : hipMemcpy2DAsync(p->ring->slot[k], width, src, spitch, width, nrows, hipMemcpyDeviceToHost, p->st);
    if (e == hipSuccess) e = hipEventRecord(p->ring->ev[k], p->st);
    if (e == hipSuccess) p->issued.store(c + 1, std::memory_order_release);
    return e;
}

// A pitched block through the ring, cut into chunks: as many whole rows as a slot takes, or, where a row is wider than a slot, the row
// in slot-sized pieces (a 1-D copy is height == 1).  `gate` (may be NULL) is asked before each chunk with the end offset of that chunk
// in the source; non-zero: nothing more is issued, what has been issued still arrives.  Returns once every chunk is ISSUED.
int pipe_block(gf_d2h_pipe* p, char* dst, size_t dpitch, const char* src, size_t spitch, size_t width, size_t height,
               int (*gate)(void* ctx, size_t upto), void* gate_ctx)
{
    const int rc = pipe_start(p);
    if (rc != GF_OK) { p->failed.store(1); return rc; }
    const size_t rps = width > D2H_SLOT ? 1 : D2H_SLOT / width;             // rows per chunk
    for (size_t r = 0; r < height; r += rps) {
        const size_t nr = height - r < rps ? height - r : rps;
        for (size_t off = 0; off < width; off += D2H_SLOT) {                // one pass unless the row is wider than a slot
            const size_t len = width - off < D2H_SLOT ? width - off : D2H_SLOT;
            if (gate && gate(gate_ctx, (r + nr - 1) * spitch + off + len) != 0) return gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h: the source was not completed");
            const hipError_t e = pipe_issue(p, dst + r * dpitch + off, dpitch, src + r * spitch + off, spitch, len, nr);
            if (e != hipSuccess) { p->failed.store(1); return gf_hip_fail(e, "gf_internal_d2h: ring copy"); }
            if (p->failed.load()) return gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h: event wait failed");
        }
    }
    return GF_OK;
}

// drain: the consumer empties what was issued and ends, the stream is waited for if blocks went out directly, the ring is released.
// false: a copy or an event wait failed somewhere along the pipe
bool pipe_finish(gf_d2h_pipe* p)
{
    p->closing.store(1);
    if (p->consumer.joinable()) p->consumer.join();
    if (p->direct_pending && hipStreamSynchronize(p->st) != hipSuccess) p->failed.store(1);
    if (p->ring) p->ring->mu.unlock();
    return p->failed.load() == 0;
}

// a synchronous copy through the ring: a pipe for the length of the call
int ring_copy(int device, hipStream_t st, char* dst, size_t dpitch, const char* src, size_t spitch, size_t width, size_t height,
              int (*gate)(void* ctx, size_t upto), void* gate_ctx)
{
    gf_d2h_pipe p;
    p.device = device; p.st = st;
    const int rc = pipe_block(&p, dst, dpitch, src, spitch, width, height, gate, gate_ctx);
    const bool ok = pipe_finish(&p);
    if (rc != GF_OK) return rc;
    return ok ? GF_OK : gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h: event wait failed");
}
}  // namespace

extern "C" {

// Synchronous copy of `bytes` from device memory to any host memory, in order on `stream`.  `gate` (may be NULL): called before a
// piece is issued with the end offset of that piece; returns once the source bytes [0, upto) are final (gf_sampler_postprocess_rows:
// the event of the group of chains they belong to), non-zero to abandon the copy -- so ONE pipeline runs over a source that is still
// being produced.
int gf_internal_d2h_gated(int device, void* stream, void* dst_host, const void* src_dev, size_t bytes,
                          int (*gate)(void* ctx, size_t upto), void* gate_ctx)
{
    if (device < 0 || device >= POOL_MAX_DEVICES || !dst_host || !src_dev) return GF_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* dst = static_cast<char*>(dst_host);
    const char* src = static_cast<const char*>(src_dev);
    void* alias = nullptr;
    if (bytes >= D2H_RING_MIN && host_range_is_pinned(dst_host, bytes, &alias)) {
        // a registered destination (gf_host_register): written directly (enqueue_d2h_rows), piece by piece as the source is completed
        for (size_t off = 0; off < bytes; off += D2H_DIRECT_PIECE) {
            const size_t len = bytes - off < D2H_DIRECT_PIECE ? bytes - off : D2H_DIRECT_PIECE;
            if (gate && gate(gate_ctx, off + len) != 0) {
                (void)hipStreamSynchronize(st);
                return gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h: the source was not completed");
            }
            GF_HIP(enqueue_d2h_rows(st, dst + off, static_cast<char*>(alias) + off, len, src + off, len, len, 1));
        }
        GF_HIP(hipStreamSynchronize(st));
        return GF_OK;
    }
    if (bytes < D2H_RING_MIN || ring_off()) {
        if (gate && gate(gate_ctx, bytes) != 0) return gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h: the source was not completed");
        GF_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
        GF_HIP(hipStreamSynchronize(st));
        return GF_OK;
    }
    return ring_copy(device, st, dst, bytes, src, bytes, bytes, 1, gate, gate_ctx);
}
int gf_internal_d2h(int device, void* stream, void* dst_host, const void* src_dev, size_t bytes)
{
    return gf_internal_d2h_gated(device, stream, dst_host, src_dev, bytes, nullptr, nullptr);
}

// The same for a pitched block -- `height` rows of `width` bytes, `spitch` apart on the device and `dpitch` apart on the host (the
// stored prefix of every chain of a sampler: row = chain).
int gf_internal_d2h_2d(int device, void* stream, void* dst_host, size_t dpitch, const void* src_dev, size_t spitch, size_t width,
                       size_t height)
{
    if (device < 0 || device >= POOL_MAX_DEVICES || !dst_host || !src_dev) return GF_ERR_INVALID_ARG;
    if (width == 0 || height == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    char* dst = static_cast<char*>(dst_host);
    const char* src = static_cast<const char*>(src_dev);
    if (width == dpitch && width == spitch) return gf_internal_d2h_gated(device, stream, dst_host, src_dev, width * height, nullptr, nullptr);
    void* alias = nullptr;
    if (width * height >= D2H_RING_MIN && host_range_is_pinned(dst, (height - 1) * dpitch + width, &alias)) {
        GF_HIP(enqueue_d2h_rows(st, dst, alias, dpitch, src, spitch, width, height));
        GF_HIP(hipStreamSynchronize(st));
        return GF_OK;
    }
    if (width * height < D2H_RING_MIN || ring_off()) {
        GF_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, st));
        GF_HIP(hipStreamSynchronize(st));
        return GF_OK;
    }
    return ring_copy(device, st, dst, dpitch, src, spitch, width, height, nullptr, nullptr);
}

int gf_internal_d2h_pipe_open(int device, void* stream, gf_d2h_pipe** out)
{
    if (device < 0 || device >= POOL_MAX_DEVICES || !out) return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_d2h_pipe* p = new (std::nothrow) gf_d2h_pipe();
    if (!p) return GF_ERR_ALLOC;
    p->device = device; p->st = (hipStream_t)stream;
    *out = p;
    return GF_OK;
}

// `height` rows of `width` bytes, `spitch` apart on the device, to rows `dpitch` apart on the host; returns once every chunk is issued.
// Whatever the size: a registered destination is written directly, anything else goes through the ring.
int gf_internal_d2h_pipe_rows(gf_d2h_pipe* p, void* dst_host, size_t dpitch, const void* src_dev, size_t spitch, size_t width, size_t height)
{
    if (!p || !dst_host || !src_dev) return GF_ERR_INVALID_ARG;
    if (width == 0 || height == 0) return GF_OK;
    char* dst = static_cast<char*>(dst_host);
    const char* src = static_cast<const char*>(src_dev);
    void* alias = nullptr;
    if (host_range_is_pinned(dst, (height - 1) * dpitch + width, &alias)) {
        // the block goes straight to where its rows belong (enqueue_d2h_rows) -- no slot, no host thread
        const hipError_t e = enqueue_d2h_rows(p->st, dst, alias, dpitch, src, spitch, width, height);
        if (e != hipSuccess) { p->failed.store(1); return gf_hip_fail(e, "gf_internal_d2h_pipe_rows"); }
        p->direct_pending = true;
        return GF_OK;
    }
    return pipe_block(p, dst, dpitch, src, spitch, width, height, nullptr, nullptr);
}

int gf_internal_d2h_pipe_close(gf_d2h_pipe* p)
{
    if (!p) return GF_OK;
    const bool ok = pipe_finish(p);
    delete p;
    return ok ? GF_OK : gf_fail_msg(GF_ERR_HIP, "gf_internal_d2h_pipe: a copy or an event wait failed");
}

// (gf_capi.hip's gf_device_trim) the pinned slots of `device`'s ring go back to the system; a read in progress keeps them
void gf_internal_d2h_ring_trim(int device)
{
    if (device < 0 || device >= POOL_MAX_DEVICES) return;
    D2HRing& R = g_d2h[device];
    std::unique_lock<std::mutex> lk(R.mu, std::try_to_lock);
    if (!lk.owns_lock()) return;
    for (int k = 0; k < D2H_SLOTS; ++k) {
        if (R.slot[k]) { (void)hipHostFree(R.slot[k]); R.slot[k] = nullptr; }
        if (R.ev[k]) { (void)hipEventDestroy(R.ev[k]); R.ev[k] = nullptr; }
    }
}

// (gf_capi.hip's host-batch pipeline) the host copy pool: `nrows` packed rows of `width` bytes to rows `dpitch` apart
void gf_internal_copy_rows(char* dst, size_t dpitch, const char* src, size_t width, size_t nrows) { copy_rows(dst, dpitch, src, width, nrows); }

// diagnostics (tools/readback_ab.py, not part of the ABI): what the link delivers in this process -- `bytes` of device memory copied into
// PINNED host memory in 64 MiB pieces, no host copy behind them; GB/s
int gf_internal_pinned_d2h_rate(int device, size_t bytes, double* gbps)
{
    if (!gbps || bytes < ((size_t)64 << 20)) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(device));
    const size_t piece = (size_t)64 << 20;
    void *h = nullptr, *d = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipHostMalloc(&h, 2 * piece, hipHostMallocDefault);
    if (e == hipSuccess) e = gf_cached_malloc(&d, piece);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, piece, hipMemcpyDeviceToHost, st);          // warm-up
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    const auto t0 = std::chrono::steady_clock::now();
    size_t done = 0;
    for (int k = 0; e == hipSuccess && done < bytes; ++k, done += piece)
        e = hipMemcpyAsync(static_cast<char*>(h) + (k & 1) * piece, d, piece, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st) (void)hipStreamDestroy(st);
    if (d) (void)gf_cached_free(d);
    if (h) (void)hipHostFree(h);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_internal_pinned_d2h_rate");
    *gbps = (double)done / dt / 1e9;
    return GF_OK;
}

// ---- the destination side ----------------------------------------------------------------------------------------------------------------------
// Make a freshly allocated host buffer ready to receive a large device-to-host copy at PCIe speed: its pages are
// touched (one byte per page is WRITTEN: the content is clobbered) from several threads.  Measured on the MI355X box
// (tools/pcie_probe.*): a D2H into untouched malloc / np.empty memory runs at 11-20 GB/s (page faults inside the copy),
// into touched pageable memory at 48-56 GB/s -- the rate of pinned memory, whose allocation itself costs 4.7 GB/s;
// touching 2 GiB takes 17 ms with 8 threads.
int gf_host_prepare(void* buf, size_t bytes) { return gf_host_prepare_n(buf, bytes, 0); }

// threads <= 0: up to 16 (as many as finish 2 GiB in ~15 ms); a caller that lets the mapping run BESIDE its own work asks for
// few: sixteen threads taking page faults hold up the main thread's launches and allocations (they share the address space's
// lock), two do not and still stay ahead of a PCIe copy (profiles/r03/readback.txt)
int gf_host_prepare_n(void* buf, size_t bytes, int threads)
{
    if (!buf && bytes) return GF_ERR_INVALID_ARG;
    const size_t page = 4096;
    const size_t min_per_thread = 16u << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? hw / 2 : 4;
    if (nt > 16) nt = 16;
    if (nt < 1) nt = 1;
    if (threads > 0) nt = (size_t)(threads > 64 ? 64 : threads);
    if (const char* e = gf_internal_env("GF_PREPARE_THREADS", 0)) { const long k = std::atol(e); if (k >= 1 && k <= 64) nt = (size_t)k; }   // A/B
    if (bytes / min_per_thread < nt) nt = bytes / min_per_thread ? bytes / min_per_thread : 1;
    // Mapping WITHOUT touching the content, so that a buffer may be prepared while a copy fills it: madvise(MADV_POPULATE_WRITE)
    // (Linux 5.14+: the kernel faults the range in writable, in one call per thread's share), and where that is refused a locked
    // OR of zero into one byte per page -- written in assembly: the compiler turns an __atomic_fetch_or(p, 0) into a LOAD, and a
    // load of an untouched anonymous page maps the shared zero page, i.e. nothing (measured: "12.6 GB in 1 ms").
    auto touch = [=](size_t lo, size_t hi) {
        char* p = static_cast<char*>(buf);
        const uintptr_t a = reinterpret_cast<uintptr_t>(p + lo), b = reinterpret_cast<uintptr_t>(p + hi);
        const uintptr_t pa = (a + page - 1) & ~(uintptr_t)(page - 1), pb = b & ~(uintptr_t)(page - 1);
        bool populated = false;
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23          /* linux/mman.h, Linux 5.14+; older headers lack the name, older kernels answer EINVAL */
#endif
        static const bool force_poke = gf_internal_env("GF_PREPARE_FORCE_POKE", 0) != nullptr;       // tests: the path taken where madvise is refused
        if (pb > pa && !force_poke) populated = madvise(reinterpret_cast<void*>(pa), pb - pa, MADV_POPULATE_WRITE) == 0;
        // (x86-64: a locked OR written in assembly -- the compiler turns __atomic_fetch_or(p, 0) into a LOAD there; elsewhere a
        // compare-and-swap of the byte with itself, which no compiler may drop: it is a write whenever it succeeds)
#if defined(__x86_64__)
        auto poke = [](char* q) { __asm__ __volatile__("lock; orb $0, (%0)" : : "r"(q) : "memory", "cc"); };
#else
        auto poke = [](char* q) {
            char v = __atomic_load_n(q, __ATOMIC_RELAXED);
            while (!__atomic_compare_exchange_n(q, &v, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
        };
#endif
        if (!populated)
            for (size_t o = lo; o < hi; o += page) poke(p + o);
        if (hi > lo) { poke(p + lo); poke(p + hi - 1); }                 // the partial pages at either end
    };
    if (nt == 1) { touch(0, bytes); return GF_OK; }
    std::vector<std::thread> th;
    const size_t per = ((bytes / nt) + page - 1) / page * page;
    for (size_t k = 0; k < nt; ++k) {
        const size_t lo = k * per, hi = (k + 1 == nt || (k + 1) * per > bytes) ? bytes : (k + 1) * per;
        if (lo >= bytes) break;
        th.emplace_back(touch, lo, hi);
    }
    for (auto& t : th) t.join();
    return GF_OK;
}

// ABI 5: a result arena -- host memory registered with the runtime, so that the read-backs' DMA writes it directly (host_range_is_pinned)
int gf_host_register(void* buf, size_t bytes)
{
    if (!buf || bytes == 0) return GF_ERR_INVALID_ARG;
    GF_HIP(hipHostRegister(buf, bytes, hipHostRegisterPortable));
    return GF_OK;
}
int gf_host_unregister(void* buf)
{
    if (!buf) return GF_ERR_INVALID_ARG;
    GF_HIP(hipHostUnregister(buf));
    return GF_OK;
}

}  // extern "C"
