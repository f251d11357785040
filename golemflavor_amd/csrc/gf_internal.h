// gf_internal.h -- the library's internal functions: everything one translation unit defines and another calls that is not in
// include/golemflavor_hip.h.  Declarations only; the defining file includes this header too, so that every definition is compiled
// against the declaration its callers see.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"

constexpr int POOL_MAX_DEVICES = 64;     // devices the per-device pools (gf_pool.hip) and read-back rings (gf_readback.hip) have room for

extern "C" {
// gf_capi.hip
const char* gf_internal_env(const char* name, int affects_results);   // getenv with a record
void gf_internal_set_error(const char* msg);                          // the text gf_last_hip_error() returns

// gf_model.hip
// gf_model is private to gf_model.hip and gf_capi.hip (gf_model.h): its constants, and (gf_model_internal: sets the device, gives the
// model a stream) its stream
int gf_model_internal(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, void** stream, int* device);
int gf_model_constants(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, int* device, int* cus, int* nbins);
// work items one pass of a bulk launch covers on the model's device: cus x GF_BLOCKS_PER_CU x GF_BLOCK (gf_launch.h gf_pass_items)
int gf_internal_pass_items(gf_model* m, int64_t* items);
// the model's device and the stream it has (NULL: none yet, and it is given none); not exported from the library
__attribute__((visibility("hidden"))) void gf_model_peek_stream(const gf_model* m, int* device, void** stream);
// the constants of multi_gaussian for cov = smearing^2 I, as gf_model_create derives them: logpdf = fma(mh, |fr - bf|^2, k)
void gf_internal_gauss_consts(double smearing, double* inv_smear, double* c0, double* mh, double* k);
// 1 if the model carries a binned measurement (gf_model_set_binned_measurement), else 0; *d_btab <- its device table
// [nbins][5] = {m_k[3], mh_k, k_k} (NULL without one).  The table's address does not change when the measurement is replaced.
int gf_model_binned(gf_model* m, const double** d_btab);
// the side of the model's tabulated likelihood (gf_model_set_table_likelihood), 0 without one; *d_table <- its device
// table (NULL without one).  A replacement of another side moves the table.
int gf_model_table(gf_model* m, const double** d_table);
// how many gf_model_set_table_likelihood and gf_model_set_binned_measurement calls have succeeded on the model: a replacement written in
// place leaves address and side as they were, the count moves (gf_modelset.h; 0 for NULL)
uint64_t gf_model_likelihood_sets(const gf_model* m);
// the model's kernels on a stream of the caller's
int gf_model_lnprob_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_lnprob, double* d_fr, int32_t* d_status);
int gf_model_propagate_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_fr, int32_t* d_status);
// k_bsm_bins (gf_spectrum.hip): d_fr_bins [n][nbins][3], or [nbins][n][3] with bin_major; BSM models only (else GF_ERR_UNSUPPORTED)
int gf_model_bins_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_fr_bins, int bin_major,
                     const int32_t* d_status);

// what a model's lnprob evaluates beside the prior: the flux-averaged likelihood of its mode, a measurement per energy bin
// (gf_model_binned) or a tabulated flavour-plane likelihood (gf_model_table); a model carries one.  GF_LLH_MIXED: the models of a
// refused set (gf_modelset.h) carry different ones.
enum GfLikelihood { GF_LLH_MIXED = -1, GF_LLH_FLUX = 0, GF_LLH_BINNED = 1, GF_LLH_TABLE = 2 };

// gf_pool.hip
// streams of the device's pool (copy stream: for a large read-back that overlaps another stream's kernels); returned idle
int gf_internal_borrow_stream(int device, void** stream);
void gf_internal_return_stream(int device, void* stream);
int gf_internal_borrow_copy_stream(int device, void** stream);
void gf_internal_return_copy_stream(int device, void* stream);
// while `on`, every arbitration launch on `stream` takes the full grid whatever the previous one found
void gf_internal_full_arbitration_grids(int device, void* stream, int on);
// GF_ERR_QUEUE_OVERFLOW if an arbitration queue dropped a pair in the launches on `stream`, which has just been synchronised
int gf_internal_check_overflow(int device, void* stream);

// gf_readback.hip
// device -> host through the pinned ring and the host copy threads.  gated: a chunk is issued once gate(ctx, upto) has returned 0
// for the source bytes [0, upto) it ends in; 2d: `height` rows of `width` bytes; pipe: one pipeline kept open over many 2d copies
int gf_internal_d2h(int device, void* stream, void* dst_host, const void* src_dev, size_t bytes);
int gf_internal_d2h_gated(int device, void* stream, void* dst_host, const void* src_dev, size_t bytes, int (*gate)(void* ctx, size_t upto), void* gate_ctx);
int gf_internal_d2h_2d(int device, void* stream, void* dst_host, size_t dpitch, const void* src_dev, size_t spitch, size_t width, size_t height);
struct gf_d2h_pipe;
int gf_internal_d2h_pipe_open(int device, void* stream, gf_d2h_pipe** out);
int gf_internal_d2h_pipe_rows(gf_d2h_pipe* p, void* dst_host, size_t dpitch, const void* src_dev, size_t spitch, size_t width, size_t height);
int gf_internal_d2h_pipe_close(gf_d2h_pipe* p);
// the host copy pool: `nrows` packed rows of `width` bytes to rows `dpitch` apart, shared out over the pool's threads
void gf_internal_copy_rows(char* dst, size_t dpitch, const char* src, size_t width, size_t nrows);
// release the pinned slots of `device`'s ring unless a read-back holds it (gf_device_trim)
void gf_internal_d2h_ring_trim(int device);

// gf_sampler_host.hip
struct GfChainView {            // the stored chain of a sampler, as post-processing (gf_postprocess.hip) sees it
    int device; hipStream_t stream; int cus;
    int nchains, nwalkers, ndim;
    int64_t nstored, nstore_cap;
    const double* d_chain;        // [nchains][nstore_cap][nwalkers][ndim]
    gf_model* model; gf_model* const* models;   // chain 0's, and one per chain or NULL
    const double* d_lnp_chain;    // [nchains][nstore_cap][nwalkers]: the stored ln_prob of every sample
    uint64_t seed;                // Philox key
    const uint64_t* d_stream_ids; // [nchains] the chains' random stream ids, NULL: chain ch has id ch
};
int gf_internal_sampler_chain_view(const gf_sampler* s, GfChainView* v);
// the likelihood the sampler evaluates: GF_LLH_BINNED for gf_sampler_create_binned's, GF_LLH_TABLE for gf_sampler_create_table's, else
// GF_LLH_FLUX
int gf_internal_sampler_likelihood(const gf_sampler* s);

// gf_sampler.hip
// k_walker_mean on `stream`: chain [nchains][cap][nwalkers][ndim] -> mean [nchains][nstored][ndim], the ensemble mean of every step
hipError_t gf_launch_walker_mean(const double* d_chain, int64_t cap, int64_t nstored, int nchains, int nwalkers, int ndim, double* d_mean,
                                 hipStream_t stream);

// gf_nested.hip
struct GfNestedView {             // the points of a nested sampler's runs, as their posterior (gf_nested_post.hip) sees them
    int device; hipStream_t stream; int cus;
    int nruns, nlive, batch, nscan, ndim;
    uint64_t seed;                // Philox key
    int32_t slot[GF_MAX_DIM];     // column -> scanned slot, -1 = fixed
    const GfCommon* d_commons;    // [nruns]: the box of every run
    const double* d_bases;        // [nruns][GF_MAX_DIM]
    const uint64_t* d_run_ids;    // [nruns]
    const double *d_dead_l, *d_dead_w, *d_dead_u;   // [iteration][nruns][batch] (dead_u: [nscan] each), NULL before the first iteration
    const double *d_live_l, *d_live_u;               // [nruns][nlive] ([nscan] each)
    gf_model* const* models;      // one per run
};
struct GfNestedRunState { int64_t iter; double lnx, lnz; int32_t done, failed; };
// the view, and (state != NULL: [nruns], read back once on the sampler's stream, which is synchronised) where every run stands; a
// sampler that has not drawn its live points yet reports every run with done = 0
int gf_internal_nested_view(gf_nested* s, GfNestedView* v, GfNestedRunState* state);

// gf_nested_post.hip
// The points of every run as the posterior takes them, for the evidence under other measurements (gf_ns_toys.hip).  _runs: the view
// and runs [nruns] (gf_weights.h: a run that has not finished, failed or has ln Z = -inf has n = 0), the points of all runs and of the
// largest; the sampler's stream is synchronised.  _gather: k_np_gather enqueued on the view's stream: d_runs [nruns] <- runs (which
// stay the caller's until the stream is synchronised), d_lnw [total], d_theta [total][ndim].
struct GfWeightRun;
int gf_internal_nested_runs(gf_nested* s, GfNestedView* v, GfWeightRun* runs, int64_t* total, int64_t* maxn);
int gf_internal_nested_gather(const GfNestedView* v, const GfWeightRun* runs, int64_t maxn, GfWeightRun* d_runs, double* d_lnw, double* d_theta);
}
