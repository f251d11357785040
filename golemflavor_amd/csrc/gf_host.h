// Host pieces shared by the C ABI of the device samplers (gf_sampler.hip, gf_nested.hip, gf_simplex.hip): the accessors
// gf_capi.hip implements (gf_model is private to it), the error helpers that publish a message through gf_last_hip_error(), and
// the allocation of the arbitration queue their settle kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"
#include "gf_launch.h"

extern "C" {
const char* gf_internal_env(const char* name, int affects_results);   // getenv with a record
int gf_model_internal(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, void** stream, int* device);
int gf_model_constants(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, int* device, int* cus,
                       int* nbins);
void gf_internal_set_error(const char* msg);
int gf_model_lnprob_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_lnprob,
                       double* d_fr, int32_t* d_status);
}

namespace {
// "what: <HIP's message>" as the last error; returns GF_ERR_HIP
inline int gf_hip_fail(hipError_t e, const char* what)
{
    char msg[256];
    std::snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
    gf_internal_set_error(msg);
    return GF_ERR_HIP;
}

// a printf-style message as the last error; returns rc
__attribute__((format(printf, 2, 3))) inline int gf_fail_msg(int rc, const char* fmt, ...)
{
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    gf_internal_set_error(msg);
    return rc;
}

// BSM: the arbitration queue for `w` parked proposals, empty, with their rows [w][GF_PEND_STRIDE] and the settle kernel's
// per-proposal counters [w][2], zero; synchronous on return.  hipMalloc is the including file's (gf_devcache.h's where that
// comes first).
inline hipError_t gf_alloc_arb_queue(size_t w, hipStream_t st, GfArbQueue** pq, double** pend_rows, unsigned int** ctl)
{
    GfArbQueue qh;
    std::memset(&qh, 0, sizeof(qh));
    qh.cap = (unsigned int)w;
    hipError_t e = hipMalloc((void**)pq, sizeof(GfArbQueue) + sizeof(GfArbItem) * w);
    if (e == hipSuccess) e = hipMalloc((void**)pend_rows, sizeof(double) * w * GF_PEND_STRIDE);
    if (e == hipSuccess) e = hipMalloc((void**)ctl, sizeof(unsigned int) * 2 * w);
    if (e == hipSuccess) e = hipMemcpyAsync(*pq, &qh, offsetof(GfArbQueue, items), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(*ctl, 0, sizeof(unsigned int) * 2 * w, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);             // qh goes out of scope
    return e;
}
}  // namespace

#define GF_HIP(call)                                        \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return gf_hip_fail(e_, #call); \
    } while (0)
