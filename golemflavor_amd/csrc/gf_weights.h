// Internal interface of the weighted-sample pipeline of gf_weights.hip (weights from log-weights, Kish ESS, weighted mean
// and covariance, the fixed-order prefix, systematic resampling into equal-weight rows) for the callers that bring their own
// log-weights: the posterior of a nested sampler's runs (gf_nested_post.hip) and the reweighting of a stored chain (gf_reweight.hip).
// A caller fills the runs and the arrays; the kernels are the same ones, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_consts.h"

// one run: its points i = 0 .. n - 1 have lnw / w / C at off + i and theta at row toff + i.  Several runs may share their theta rows
// (the targets of a reweighted chain).  n = 0: no posterior.  nd, lnw0: the nested sampler's gather only.
struct GfWeightRun {
    int64_t off, toff, n, nd;
    double lnw0;
};

enum { GF_WST_M = 0, GF_WST_S = 1, GF_WST_S2 = 2, GF_WST_ESS = 3, GF_WST_SP = 4, GF_WST_SP2 = 5, GF_WST_FACT = 6, GF_WEIGHT_STAT = 8 };
// doubles of `part` per run and leaf: with the covariance, without
constexpr int GF_WEIGHT_PART_COV = GF_MAX_DIM * GF_MAX_DIM, GF_WEIGHT_PART = 2 + GF_MAX_DIM;
constexpr int GF_WEIGHT_LEAF = 4096;           // gfnp::LEAF
constexpr int GF_WEIGHT_TOT_PER_LEAF = 64;     // doubles of `tot` per run and leaf

struct GfWeightArgs {
    int32_t ndim;
    int32_t fixed[GF_MAX_DIM];      // != 0: every point of a run holds the same value in the column (mean = that value, covariances 0)
    uint64_t seed;                  // resampling: u = gfnp::resample_offset(seed, ids[run])
    const uint64_t* ids;            // [R], device
    const GfWeightRun* runs;        // [R], device
    const double* lnw;              // compact, a run's at its off
    const double* theta;            // rows of ndim doubles, a run's from its toff on
    double *w, *C;                  // compact as lnw: e, then p; the inclusive prefix (prefix only)
    double* part;                   // [R][maxleaves][GF_WEIGHT_PART_COV or GF_WEIGHT_PART]
    double* stat;                   // [R][GF_WEIGHT_STAT]
    double *mean, *cov;             // [R][GF_MAX_DIM], [R][GF_MAX_DIM][GF_MAX_DIM]
    double* tot;                    // [R][maxleaves * GF_WEIGHT_TOT_PER_LEAF] (prefix only)
    int64_t maxleaves;              // max(1, ceil(largest n / GF_WEIGHT_LEAF))
};

// weights, sums and the mean; moments: the covariance; prefix: C.  Asynchronous on `st`.
hipError_t gf_weights_launch(const GfWeightArgs& a, int R, bool moments, bool prefix, hipStream_t st);
// index [R][N]: the point of every equal-weight row, -1 for a run without a posterior
hipError_t gf_weights_resample(const GfWeightArgs& a, int R, int64_t N, int64_t* d_index, hipStream_t st);
// out [.][N][width] for the runs run0 .. run0 + nruns - 1: theta in the columns from `first` on (those before are left as they are); a
// row without a point is NaN in every column
hipError_t gf_weights_rows(const GfWeightArgs& a, int64_t N, const int64_t* d_index, int run0, int nruns, int width, int first, double* d_out,
                           hipStream_t st);
