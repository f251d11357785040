// Internal interface of gf_marginal.hip (the posterior marginals of include/golemflavor_hip.h) for the entry points that own the
// rows they hand over: gf_marginals* in gf_marginal.hip itself, gf_sampler_marginals in gf_sampler.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"

// the public argument checks of gf_marginals_device (everything except the rows): GF_OK, GF_ERR_INVALID_ARG or GF_ERR_UNSUPPORTED
int gf_marginal_check_args(int nchains, int64_t nrows, int width, const gf_marginal_spec* spec);
// d_rows: chain ch's rows [nrows][width] start at d_rows + ch * chain_stride (doubles); everything on `st` (current device);
// every output of *out may be NULL; synchronous
int gf_marginal_run(hipStream_t st, const double* d_rows, int64_t chain_stride, int nchains, int64_t nrows, int width,
                    const gf_marginal_spec* spec, const gf_marginal_out* out);
