// Internal interface of gf_diag.hip (the chain diagnostics of include/golemflavor_hip.h) for the entry point that sees a sampler's
// stored chain: gf_sampler_diagnostics in gf_postprocess.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"

// the argument rules of gf_chain_diagnostics_device (GF_ERR_INVALID_ARG / GF_ERR_UNSUPPORTED)
int gf_diag_check_args(int nchains, int64_t nsteps, int nwalkers, int ndim, const gf_diag_spec* spec, const gf_diag_out* out);
// chain ch [nsteps][nwalkers][ndim] starts at d_chain + ch * chain_stride (doubles); arguments checked by the caller; on `st`
// (current device), chain after chain through the same scratch buffers of the library's cache; synchronous
int gf_diag_run(hipStream_t st, const double* d_chain, int64_t chain_stride, int nchains, int64_t nsteps, int nwalkers, int ndim,
                const gf_diag_spec* spec, const gf_diag_out* out);
