// gf_sampler_launch.h -- the seam between the ensemble sampler's kernels (gf_sampler.hip) and its host side (gf_sampler_host.hip): the
// kernels' argument structs, which the host fills, and the launchers, which gf_sampler.hip defines.  The three structs are KERNEL
// ARGUMENTS: their fields, order and types are part of the kernels' code.
#pragma once
#include "gf_consts.h"
#include "gf_launch.h"

// Step counters live on the device so that a captured hipGraph of GRAPH_STEPS steps can be replayed with
// constant kernel arguments: each kernel node carries its own frozen `step_offset`; the base counters
// are advanced once per replay by k_tick (one extra 1-thread launch per GRAPH_STEPS steps).  (GfStepState: gf_launch.h)

struct StretchArgs {
    GfStepState* state;
    double* pos;            // [nchains][nwalkers][ndim]
    double* lnp;            // [nchains][nwalkers]
    uint32_t* naccept;      // [nchains][nwalkers]
    uint32_t* flags;        // [0]: proposals the reference would have raised on (NON_UNITARY), whichever tier found out; [2]: see stretch_body
    GfArbQueue* pq;         // BSM: proposals whose verdict the in-kernel tiers cannot settle are parked here ...
    double* pend_rows;      // ... with their row [GF_PEND_STRIDE] (theta | lnprob | ln(z^(ndim-1)/u)), for k_stretch_settle
    double* chain;          // [nchains][nstore_cap][nwalkers][ndim] or null
    double* lnp_chain;      // [nchains][nstore_cap][nwalkers] or null
    int64_t nstore_cap;
    uint64_t seed;
    int32_t nchains, nwalkers, half;
    int32_t step_offset;    // step index relative to the device-side base counters
    double a;
    // one model per chain (gf_sampler_create_multi): chain ch evaluates commons[ch] / tbs[ch] / ptabs[ch]
    const GfCommon* commons;
    const GfBsm* const* tbs;
    const double* const* ptabs;
    int32_t nbins_max;      // largest nbins over the chains' models (BSM); sizes the lane-group buffers
    int32_t lpw;            // lanes per walker for this run (host-side dispatch only)
    // random stream of chain ch: Philox counter word = stream_ids[ch] * (nwalkers / 2) + walker slot.  NULL: ch itself.
    // A scan hands in the GLOBAL grid index, so that a grid point's chain does not depend on which rank runs it or on
    // how many other points share its sampler.
    const uint64_t* stream_ids;
    // a sampler of the energy-resolved likelihood (gf_sampler_create_binned): [nmodels] the models' binned measurements
    // (gf_consts.h: GF_BINNED_STRIDE x nbins doubles each), chain ch reads btabs[ch] (one model: btabs[0]); NULL for every other sampler
    const double* const* btabs;
    // a sampler of the tabulated flavour-plane likelihood (gf_sampler_create_table): [nmodels] the models' tables in
    // global memory and their sides, chain ch reads entry ch (one model: entry 0); NULL for every other sampler.  The arrays are the
    // sampler's model set's for good; gf_sampler_run rewrites their entries when a model's table was replaced.
    const double* const* ttabs;
    const int32_t* tsides;
};

// k_stretch_persist: one workgroup per ensemble, a whole run in one launch
struct PersistArgs {
    const GfCommon* commons;        // [nmodels]
    const double* const* ptabs;     // [nmodels]
    int32_t nmodels;                // 1: every chain samples commons[0]; else one per chain
    int32_t nwalkers;
    double* pos;                    // [nchains][nwalkers][ndim]
    double* lnp;                    // [nchains][nwalkers]
    uint32_t* naccept;              // [nchains][nwalkers]
    double* chain;                  // [nchains][nstore_cap][nwalkers][ndim] or null
    double* lnp_chain;
    int64_t nstore_cap, store_base;
    uint64_t seed, iteration_base;
    int64_t nsteps;
    int32_t thin, store;
    double a;
    const uint64_t* stream_ids;     // as StretchArgs::stream_ids
    int32_t workers;                // threads that move walkers; the block's other threads (if any) draw the random numbers one half-step ahead
};

// k_stretch_chain: one workgroup per chain, BSM posteriors
struct ChainArgs {
    const GfCommon* commons;        // [nmodels]
    const GfBsm* const* tbs;        // [nmodels] (nmodels > 1), else null
    const GfBsm* tb;                // nmodels == 1
    const double* const* ptabs;     // [nmodels]
    int32_t nmodels;                // 1: every chain samples commons[0]
    int32_t nwalkers;
    double* pos;                    // [nchains][nwalkers][ndim]
    double* lnp;                    // [nchains][nwalkers]
    uint32_t* naccept;              // [nchains][nwalkers]
    uint32_t* flags;                // [0]: proposals the reference would have raised on
    double* pend_rows;              // [nchains * nwalkers / 2][GF_PEND_STRIDE]: a parked proposal's row
    double* chain;                  // [nchains][nstore_cap][nwalkers][ndim] or null
    double* lnp_chain;
    int64_t nstore_cap, store_base; // chain slot of the RUN's first stored step
    uint64_t seed, iteration_base;  // Philox counter word of this launch's first step
    int64_t run_step_base;          // steps of the run done before this launch (thinning counts from the run's start)
    int32_t nsteps, thin, store;
    double a;
    const uint64_t* stream_ids;     // as StretchArgs::stream_ids
    double* lazy_rows;              // [nchains][lazy_cap][GF_PEND_STRIDE]: undecided proposals that are rejected either way ...
    unsigned long long* lazy_mask;  // [nchains][lazy_cap]: ... with their undecided bins (k_stretch_chain settles them in bulk)
    int32_t lazy_cap;
    unsigned long long* stats;      // [nchains][8] (may be null): per chain, ns on the 100 MHz wall clock spent in [0] proposals, [1] settling
                                    // parked proposals, [2] bulk settlement; [3] proposals waited for, [4] passes that waited, [5] settled in bulk,
                                    // [6] passes, [7] bulk settlements
};

// workgroup of the per-chain sampler: eight waves -- two per SIMD, 256 VGPRs each -- = 56 nine-lane teams when proposals are settled
constexpr int CH_BLOCK = 512;

// The launchers (gf_sampler.hip); not exported from the library.  Each returns the launch's hipGetLastError().
#define GF_SAMPLER_LOCAL __attribute__((visibility("hidden")))
// one half-step of every chain: k_stretch (a.commons null: every chain samples c / tb / ptab) or k_stretch_multi; the instance is the
// tabulated likelihood's where a.ttabs is set, the energy-resolved one's where a.btabs is, else the one of c.mode, at a.lpw lanes
GF_SAMPLER_LOCAL hipError_t gf_launch_stretch(const GfCommon& c, const GfBsm* tb, const double* ptab, const StretchArgs& a, hipStream_t st);
// threads and dynamic LDS of the persistent kernel; lds == 0: the ensemble does not fit one workgroup
GF_SAMPLER_LOCAL void gf_persist_geometry(int nwalkers, int ndim, int* threads, size_t* lds, int* workers, int nchains, int cus);
GF_SAMPLER_LOCAL hipError_t gf_launch_persist(int mode, int ndim, int nchains, int threads, size_t lds, const PersistArgs& a, hipStream_t st);
GF_SAMPLER_LOCAL hipError_t gf_launch_chain(int ndim, int nchains, const ChainArgs& a, hipStream_t st);
// k_tick: the device-side base counters advance by nsteps
GF_SAMPLER_LOCAL hipError_t gf_launch_tick(GfStepState* state, int nsteps, hipStream_t st);
// k_fix_start: lnp[i] = -inf and flags[0] counted where status[i] is ST_NON_UNITARY, i < n
GF_SAMPLER_LOCAL hipError_t gf_launch_fix_start(const int32_t* status, int64_t n, double* lnp, uint32_t* flags, hipStream_t st);
