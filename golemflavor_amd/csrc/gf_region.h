// Internal interface of gf_region.hip (the credible regions of include/golemflavor_hip.h) for the entry points that own the
// histogram they hand over: gf_flavor_region* in gf_region.hip itself, gf_sampler_regions in gf_sampler.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the public argument checks: GF_OK, GF_ERR_INVALID_ARG, or GF_ERR_UNSUPPORTED for a radius above GF_REGION_MAX_RADIUS
int gf_region_check_args(int nchains, int nbins, int radius, const double* weights, const double* coverage, int ncov, int64_t cap);
// normalise, smooth, select on `st` (current device); d_counts [nchains][nbins]^3 on the device, every output as in
// gf_flavor_region_device; synchronous
int gf_region_run(hipStream_t st, const uint64_t* d_counts, int nchains, int nbins, int radius, const double* weights, const double* coverage,
                  int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                  int32_t* cells, double* density, double* d_smoothed);
// the same stages for a batch of histograms of shape (n0, n1, n2); an axis of length 1 is not filtered.  one_list != 0: cells /
// density are [nchains][cap], the first min(cap, largest thres) sorted cells of each chain (gf_marginal.hip)
int gf_region_run_shape(hipStream_t st, const uint64_t* d_counts, int nchains, int n0, int n1, int n2, int radius, const double* weights,
                        const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out,
                        double* mass, int32_t* cells, double* density, double* d_smoothed, int one_list);
// fr [n][3] -> NaN where status [n] != 0 (asynchronous)
hipError_t gf_launch_mask_fr(double* fr, const int32_t* status, int64_t n, hipStream_t s);
