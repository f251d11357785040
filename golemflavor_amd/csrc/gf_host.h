// Host pieces shared by the C ABI of the device samplers, of the cube runs, of chain post-processing and of read-back (every host
// file of the library but gf_devcache.hip): the library's internal functions (gf_internal.h), the error helpers that publish a
// message through gf_last_hip_error(), the two sources of device memory by name (GfMem), the holder of a call's scratch buffers with
// the way an entry point reports a refused request of its own (GfScratch::take), and the allocation of the arbitration queue the
// settle kernels share.  What the three sample sources share for their reductions is in gf_rowsets.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"
#include "gf_devcache.h"
#include "gf_internal.h"
#include "gf_launch.h"

// one definition each across the library's objects, and none of them exported from it
#pragma GCC visibility push(hidden)

// "what: <HIP's message>" as the last error; returns GF_ERR_HIP
inline int gf_hip_fail(hipError_t e, const char* what)
{
    char msg[512];
    std::snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
    gf_internal_set_error(msg);
    return GF_ERR_HIP;
}

// a printf-style message as the last error; returns rc
__attribute__((format(printf, 2, 3))) inline int gf_fail_msg(int rc, const char* fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    gf_internal_set_error(msg);
    return rc;
}

// The Gaussian constants of one mock measurement (bf [3], smearing sm) for the entry point `who`, whose messages call it realisation
// `label`: m [3] <- bf, *mh and *k by gf_internal_gauss_consts (gf_toys.hip, gf_ns_toys.hip)
inline int gf_gauss_realisation(const double* bf, double sm, size_t label, const char* who, double* m, double* mh, double* k)
{
    if (!(sm > 0.0) || !std::isfinite(sm) || !std::isfinite(bf[0]) || !std::isfinite(bf[1]) || !std::isfinite(bf[2]))
        return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: realisation %zu needs a finite measurement and a smearing > 0", who, label);
    double inv_smear, c0;
    for (int d = 0; d < 3; ++d) m[d] = bf[d];
    gf_internal_gauss_consts(sm, &inv_smear, &c0, mh, k);
    if (!std::isfinite(*mh) || !std::isfinite(*k))
        return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the smearing of realisation %zu is outside the range of the Gaussian's constants", who, label);
    return GF_OK;
}

// Where device memory comes from, named at every call that takes some: the library's cache of large blocks (gf_devcache.h) or the
// driver.  What one of them gave goes back through the same one.
enum GfMem { GF_MEM_CACHED, GF_MEM_DRIVER };
inline hipError_t gf_mem_alloc(GfMem mem, void** p, size_t bytes) { return mem == GF_MEM_CACHED ? gf_cached_malloc(p, bytes) : hipMalloc(p, bytes); }
inline hipError_t gf_mem_free(GfMem mem, void* p) { return mem == GF_MEM_CACHED ? gf_cached_free(p) : hipFree(p); }

// The device scratch buffers of one call, released together when the holder goes out of scope, in the order they were taken (the
// order decides which cached block a later request of the same size reuses).  Not for buffers an object owns across calls.
struct GfScratch {
    const GfMem mem;
    std::vector<void*> p;
    int failed = GF_OK;                 // the first refused take's code
    explicit GfScratch(GfMem mem_) : mem(mem_) {}
    template <typename T>
    hipError_t get(T** out, size_t bytes)
    {
        void* q = nullptr;
        const hipError_t e = gf_mem_alloc(mem, &q, bytes ? bytes : 8);
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<T*>(q);
        return e;
    }
    // get() for an entry point `who`.  A refused request clears HIP's last error (the next hipGetLastError() after a launch must not see
    // it), publishes the size and is GF_ERR_ALLOC; the takes after it do nothing and return the same, so a run of takes is checked once,
    // at its last one or through `failed`
    template <typename T>
    int take(T** out, size_t bytes, const char* who)
    {
        if (failed != GF_OK || get(out, bytes) == hipSuccess) return failed;
        (void)hipGetLastError();
        return failed = gf_fail_msg(GF_ERR_ALLOC, "%s: %zu bytes of device scratch were not granted", who, bytes);
    }
    ~GfScratch() { for (void* q : p) (void)gf_mem_free(mem, q); }
};

// BSM: the arbitration queue for `w` parked proposals, empty, with their rows [w][GF_PEND_STRIDE] and the settle kernel's
// per-proposal counters [w][2], zero, all three from `mem`; synchronous on return
inline hipError_t gf_alloc_arb_queue(GfMem mem, size_t w, hipStream_t st, GfArbQueue** pq, double** pend_rows, unsigned int** ctl)
{
    GfArbQueue qh;
    std::memset(&qh, 0, sizeof(qh));
    qh.cap = (unsigned int)w;
    hipError_t e = gf_mem_alloc(mem, (void**)pq, sizeof(GfArbQueue) + sizeof(GfArbItem) * w);
    if (e == hipSuccess) e = gf_mem_alloc(mem, (void**)pend_rows, sizeof(double) * w * GF_PEND_STRIDE);
    if (e == hipSuccess) e = gf_mem_alloc(mem, (void**)ctl, sizeof(unsigned int) * 2 * w);
    if (e == hipSuccess) e = hipMemcpyAsync(*pq, &qh, offsetof(GfArbQueue, items), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(*ctl, 0, sizeof(unsigned int) * 2 * w, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);             // qh goes out of scope
    return e;
}

#pragma GCC visibility pop

#define GF_HIP(call)                                        \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return gf_hip_fail(e_, #call); \
    } while (0)
