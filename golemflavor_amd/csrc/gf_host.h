// Host pieces shared by the C ABI of the device samplers (gf_sampler.hip, gf_nested.hip, gf_simplex.hip): the accessors
// gf_capi.hip implements (gf_model is private to it) and the error helpers that publish a message through gf_last_hip_error().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"

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
}  // namespace

#define GF_HIP(call)                                        \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return gf_hip_fail(e_, #call); \
    } while (0)
