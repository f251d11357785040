// Internal interface of gf_elements.hip (the element-space rows of include/golemflavor_hip.h) for the entry point that owns the rows
// it hands over: gf_sampler_element_marginals in gf_sampler.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"

// chain ch's rows [nrows][width_in] start at d_in + ch * in_stride (doubles) and go to d_out + ch * out_stride as [nrows][width_out],
// width_out = gf_element_plan_width(plan, width_in) >= 1 (checked by the caller); on `st` (current device), synchronous (the
// tiles' masks of rows for the exact pass live in a buffer of the library's cache for the call); `cus`: the device's compute units
hipError_t gf_element_run(hipStream_t st, const double* d_in, int64_t in_stride, int nchains, int64_t nrows, int width_in,
                             const gf_element_plan* plan, double* d_out, int64_t out_stride, int cus);
