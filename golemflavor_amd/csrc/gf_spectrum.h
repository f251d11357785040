// Internal interface of gf_spectrum.hip (the energy-resolved composition of include/golemflavor_hip.h) for the files
// that own what it works on: gf_model.hip (the model's constants), gf_postprocess.hip (a sampler's stored chain) and
// gf_nested_post.hip (a nested sampler's posterior rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"

// k_bsm_bins, asynchronous on `s`: the composition of every row at every energy bin of the model, values only.
//   bin_major == 0: out [n][nbins][3];  != 0: out [nbins][n][3]
//   status (may be NULL): [n] as the propagate path wrote it; a row whose status is not GF_ST_OK gets NaN in every bin
hipError_t gf_launch_bsm_bins(const GfCommon& c, const GfCommon* d_common, const GfBsm* d_bsm, int nbins, const double* ptab, const double* theta,
                              int layout, int64_t n, double* out, int bin_major, const int32_t* status, int cus, hipStream_t s);

// the public argument checks of the reductions (everything except the rows)
int gf_spectrum_check_args(int nbins_e, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out);
// One chain: d_slab [nbins_e][nrows][3] (bin-major) reduced by gf_marginal_run with the energy bins as its chains; the results
// land at index `ch` of *out's arrays ([nchains][nbins_e]...).  Everything on `st` (current device); synchronous.
int gf_spectrum_reduce(hipStream_t st, const double* d_slab, int nbins_e, int64_t nrows, const gf_spectrum_spec* spec,
                       const gf_spectrum_out* out, int ch);
