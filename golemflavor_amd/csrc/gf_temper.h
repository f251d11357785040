// gf_temper.h -- the two seams of the tempered sampler.  Between its kernels (gf_temper.hip) and its host side
// (gf_temper_host.hip): the kernels' argument structs, which the host fills, and the launchers.  Between its host side and the ensemble
// sampler's (gf_sampler_host.hip), which holds a GfTempered only as a pointer: the four functions at the end.  Not exported from the library.
#pragma once
#include "gf_consts.h"
#include "gf_launch.h"
#include "gf_sampler_launch.h"

// k_lnprior_lnl: lnprior and lnl apart for `rows` rows of each of the grid's blockIdx.y models (row i of model r is row r * rows + i of
// every array), under the likelihood the models carry.  Rows whose unitarity verdict the in-kernel tiers cannot settle are parked
// (pq / pend_rows, capacity: every row) and settled exactly, as the maximiser's candidates are, before k_pt_finish ends the call.
struct GfSplitArgs {
    const GfCommon* commons;        // [nmodels]
    const GfBsm* const* tbs;        // [nmodels]
    const double* const* ptabs;     // [nmodels]
    const double* theta;            // [nmodels * rows][ndim]
    double* lp;                     // [nmodels * rows]: lnprior, -inf outside the box
    double* lnl;                    // [nmodels * rows]: lnL, -inf outside the box, NaN where the reference would have raised
    int32_t* status;                // [nmodels * rows]: gf_status, as gf_lnprob_batch gives it
    GfArbQueue* pq;
    double* pend_rows;              // [nmodels * rows][GF_PEND_STRIDE]
    int32_t rows, ndim, nbins_max;
    // k_pt_finish, optional: T [nmodels * rows] <- lp + betas[r] lnl (gf_temper.hpp), NaN where the reference would have raised
    const double* betas;            // [nmodels]
    double* T;
    // the likelihood the models carry, as StretchArgs has it: [nmodels] the binned measurements (the energy-resolved instance), or the
    // tables in global memory and their sides (the tabulated instance); all NULL: the flux-averaged instance
    const double* const* btabs;
    const double* const* ttabs;
    const int32_t* tsides;
};

// k_pt_swap: one replica-exchange round (gf_temper.hpp) over chains [ngroups][ntemps]
struct GfSwapArgs {
    double* pos;                    // [nchains][nwalkers][ndim]
    double* T;                      // [nchains][nwalkers]: the walkers' scalar, recomputed for both walkers of an exchanged pair
    const double* lp;               // [nchains][nwalkers]: of the current walkers (k_lnprior_lnl, just ahead in stream order)
    const double* lnl;
    const double* betas;            // [nchains]
    const uint64_t* stream_ids;     // [nchains] or NULL
    uint32_t* counts;               // [nchains][2]: pairs (t, t + 1) proposed / accepted, at the entry of chain (g, t)
    uint64_t seed, round;
    int32_t ngroups, ntemps, nwalkers, ndim;
};

// k_pt_series: lnl of every stored sample and its reduction over the walkers of a step (gf_temper.hpp)
struct GfSeriesArgs {
    const GfCommon* commons;        // [nchains]
    const GfBsm* const* tbs;
    const double* const* ptabs;
    const double* chain;            // [nchains][cap][nwalkers][ndim]
    const double* lnp_chain;        // [nchains][cap][nwalkers]: a sample stored at -inf (a start position that never moved) has lnl -inf
    int64_t cap, nstored;
    int32_t nwalkers, ndim;
    const double* d_up;             // [nchains]
    const double* d_dn;
    double* lnl;                    // [nchains][nstored][nwalkers]
    double* out;                    // [nchains][nstored][5]
    const double* const* btabs;     // [nchains], as GfSplitArgs'
    const double* const* ttabs;
    const int32_t* tsides;
};

#define GF_TEMPER_LOCAL __attribute__((visibility("hidden")))
// one tempered half-step of every chain, one model per chain (a.commons set): chain ch samples prior * L^betas[ch]; the instance is the
// tabulated likelihood's where a.ttabs is set, the energy-resolved one's where a.btabs is, else the flux-averaged one's
GF_TEMPER_LOCAL hipError_t gf_launch_stretch_tempered(const StretchArgs& a, const double* d_betas, int ndim, hipStream_t st);
// k_lnprior_lnl, the exact verdict of the rows it parked (ctl: [nmodels * rows][2], zero between uses; state: any GfStepState on the
// device) and k_pt_finish, in stream order
GF_TEMPER_LOCAL hipError_t gf_launch_lnprior_lnl(const GfSplitArgs& a, int nmodels, unsigned int* ctl, const GfStepState* state, int cus, hipStream_t st);
GF_TEMPER_LOCAL hipError_t gf_launch_pt_swap(const GfSwapArgs& a, hipStream_t st);
GF_TEMPER_LOCAL hipError_t gf_launch_pt_series(const GfSeriesArgs& a, int nchains, hipStream_t st);

// What gf_sampler_host.hip asks of a tempered sampler (s->tp set; gf_temper_host.hip):
struct gf_sampler;
struct GfTempered;
struct Run;
struct GridSteps;
// gf_sampler_set_state behind the upload of the positions: the state's scalar T of every walker at its chain's beta, -inf (and counted)
// where the reference would have raised; synchronous on return
GF_TEMPER_LOCAL int gf_temper_start(gf_sampler* s);
// gf_sampler_reset: the swap counters <- 0, on the sampler's stream
GF_TEMPER_LOCAL hipError_t gf_temper_clear_counts(gf_sampler* s);
// the run `r` of the grid kernels `g`, with a replica-exchange round behind every swap_every-th step since creation
GF_TEMPER_LOCAL int gf_temper_run(Run& r, GridSteps& g);
// gf_sampler_destroy: tp (may be null) and its device buffers
GF_TEMPER_LOCAL void gf_temper_free(GfTempered* tp);
