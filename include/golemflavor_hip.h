/*
 * golemflavor_hip.h -- C ABI of libgolemhip.so, the MI355X (gfx950) evaluation engine for
 * GolemFlavor's ensemble log-posterior callback.
 *
 * The reference has no FFI: the hot path sits behind a Python callable `ln_prob(theta) -> float`
 * that emcee calls once per walker per step (golemflavor/mcmc.py:27-41).  Each entry point below
 * names the reference interface it replaces (file:line under the reference tree).  Everything is
 * plain pointers and sizes; no torch, no C++ types.  The Python side binds this header with ctypes
 * (golemflavor_amd/_lib.py); INTEGRATION.md shows the stub a GolemFlavor maintainer would add.
 *
 * Conventions
 *   - every function returns a gf_error (0 = GF_OK) and never throws; gf_strerror() explains it;
 *   - arrays are caller-owned, fp64, row-major; theta is [n][ndim] exactly as emcee hands it over;
 *   - per-walker outcomes travel in `status` (gf_status), not in the return code;
 *   - a gf_model is bound to one device and one HIP stream.  Thread-safe per handle: the entry points that use the
 *     model's staging buffers or its unitarity queue (gf_lnprob_batch, gf_propagate_batch, gf_lnprob_cube_batch, the
 *     *_device launches) take a per-model lock, so several host threads may share one model (their calls run one
 *     after the other); different models are independent and may be driven concurrently;
 *   - there is NO CPU fallback: without a gfx950 device gf_model_create returns GF_ERR_NO_DEVICE.
 */
#ifndef GOLEMFLAVOR_HIP_H
#define GOLEMFLAVOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 5
#define GF_MAX_DIM 16
#define GF_MAX_BINS 64
/* CP phases (dcp; the NP matrix's for texture NONE) must stay within +-GF_PHASE_MAX: range (sampled) or value
 * (fixed).  The reference's paramsets box them into [0, 2 pi] (scripts/fr.py:41, scripts/mc_unitary.py:39);
 * gf_model_create returns GF_ERR_UNSUPPORTED otherwise. */
#define GF_PHASE_MAX 1.0e6

typedef enum gf_error {
    GF_OK = 0,
    GF_ERR_INVALID_ARG = 1,   /* NULL pointer, ndim out of range, inconsistent descriptor      */
    GF_ERR_NO_DEVICE = 2,     /* no HIP device / not gfx950                                     */
    GF_ERR_HIP = 3,           /* a HIP runtime call failed; gf_last_hip_error() has the string  */
    GF_ERR_ALLOC = 4,
    GF_ERR_COMM = 5,          /* RCCL failure                                                   */
    GF_ERR_UNSUPPORTED = 6,
    GF_ERR_QUEUE_OVERFLOW = 7 /* ABI 3: a unitarity work queue was found full on the device and (walker, bin) pairs were dropped:
                                 the status array of that batch is incomplete.  The host sizes batches to fit, so this is a
                                 library bug surfacing loudly instead of as a silently missing verdict                     */
} gf_error;

/* per-walker outcome.  Reference behaviour: OUT_OF_PRIOR -> ln_prob returns -inf (llh.py:74-78,
 * ipynb:360-361); NON_UNITARY -> AssertionError raised inside params_to_BSMu (fr.py:398-399,
 * 493-498); the Python wrapper re-raises it unless told to map it to -inf. */
typedef enum gf_status {
    GF_ST_OK = 0,
    GF_ST_OUT_OF_PRIOR = 1,
    GF_ST_NON_UNITARY = 2,
    GF_ST_NAN = 3
} gf_status;

/* golemflavor/enums.py:39-42 (same integer values) */
typedef enum gf_prior_kind { GF_PRIOR_UNIFORM = 1, GF_PRIOR_GAUSSIAN = 2, GF_PRIOR_LIMITEDGAUSS = 3 } gf_prior_kind;
/* golemflavor/enums.py:59-63 (same integer values) */
typedef enum gf_texture { GF_TEX_OEU = 1, GF_TEX_OET = 2, GF_TEX_OUT = 3, GF_TEX_NONE = 4 } gf_texture;

typedef enum gf_mode {
    GF_MODE_PRIOR_ONLY = 0,  /* lnprior + flat llh: scripts/mc_unitary.py:121-143, mc_texture.py:148-170 */
    GF_MODE_SM_GAUSS = 1,    /* notebook posterior: examples/inference.ipynb:307-338,356-364            */
    GF_MODE_BSM_GAUSS = 2    /* golemflavor/llh.py:94-130 with the Gaussian substitute for gf.get_llh
                                (README.md:70-74): flux_averaged_BSMu (fr.py:403-458) -> multi_gaussian  */
} gf_mode;

/* Layout of a device-resident theta block handed to the *_device entry points. */
typedef enum gf_layout {
    GF_LAYOUT_AOS = 0,       /* [n][ndim] row-major: the emcee layout                           */
    GF_LAYOUT_SOA = 1        /* [ndim][n]: one contiguous column per parameter                  */
} gf_layout;

/*
 * Flat model descriptor: what the reference carries in (ParamSet, args, asimov ParamSet), compiled
 * once per run by golemflavor_amd/descriptor.py.  Replaces the functools.partial-bound state of
 * `ln_prob` (examples/inference.ipynb:366-371, scripts/fr.py:182-187).
 */
typedef struct gf_model_desc {
    int32_t abi_version;               /* GF_ABI_VERSION                                        */
    int32_t ndim;                      /* len(llh_paramset), 1..GF_MAX_DIM                      */
    int32_t mode;                      /* gf_mode                                               */
    int32_t texture;                   /* gf_texture (BSM only), fr.py:370-378                  */
    int32_t dimension;                 /* BSM operator dimension d (E^(d-3)), fr.py:394         */
    int32_t nbins;                     /* energy bins of the flux average, fr.py:413-414        */
    /* column of theta that holds each named parameter, or -1 = take the *_fixed value          */
    int32_t idx_sm[4];                 /* s_12_2, c_13_4, s_23_2, dcp (fr.py:116-162)           */
    int32_t idx_mass[2];               /* m21_2, m3x_2 (fr.py:422-435)                          */
    int32_t idx_src[2];                /* source flavor angles sin^4(phi), cos(2psi) (fr.py:82) */
    int32_t idx_scale;                 /* logLam (fr.py:380)                                    */
    int32_t idx_mm[4];                 /* NP mixing angles when texture == NONE (fr.py:378)     */
    int32_t idx_gamma;                 /* astroDeltaGamma (llh.py:105); cancels in fr, kept for fidelity */
    int32_t idx_src_x;                 /* astroX: the source is normalize_fr((x, 1 - x, 0)) with x = this column
                                          (scripts/mc_x.py:43,186-190); -1 = not used; excludes idx_src      */
    int32_t reserved0;                 /* 0                                                     */
    int32_t prior_kind[GF_MAX_DIM];    /* gf_prior_kind per column (llh.py:81-90)               */
    double lo[GF_MAX_DIM];             /* Param.ranges[0]  (closed box, llh.py:74-78)           */
    double hi[GF_MAX_DIM];             /* Param.ranges[1]                                       */
    double loc[GF_MAX_DIM];            /* Param.nominal_value (prior centre)                    */
    double sigma[GF_MAX_DIM];          /* Param.std                                             */
    double log_mass[GF_MAX_DIM];       /* log Gaussian mass of the truncation interval (scipy truncnorm) */
    double sm_fixed[4];                /* defaults: NuFIT point, fr.py:313                      */
    double mass_fixed[2];              /* defaults: MASS_EIGENVALUES, fr.py:42                  */
    double source_ratio[3];            /* args.source_ratio when the source is not sampled      */
    double scale_fixed;
    double mm_fixed[4];
    double gamma_fixed;                /* spectral index when astroDeltaGamma is not sampled    */
    double bestfit_fr[3];              /* injected / best-fit composition (llh.py:32-54)        */
    double smearing;                   /* Gaussian width (llh.py:53)                            */
    double offset;                     /* multi_gaussian offset, default -320 (llh.py:32)       */
    double flat_llh;                   /* value of the flat likelihood, 1.0 (mc_unitary.py:131) */
    double bin_edges[GF_MAX_BINS + 1]; /* args.binning after process_args (scripts/fr.py:122-124) */
} gf_model_desc;

typedef struct gf_model gf_model;      /* opaque: device constants + stream + staging buffers   */

/* ---- library / device ------------------------------------------------------------------- */
int gf_abi_version(void);
const char* gf_strerror(int err);
const char* gf_last_hip_error(void);   /* thread-local text of the last failing HIP/RCCL call    */
size_t gf_sizeof_model_desc(void);     /* sizeof(gf_model_desc) as compiled: lets a binding verify its layout */
/* ABI 3.  "NAME=value ..." of every GF_* environment override this process's library has honoured so far ("" = none).  The ones
 * that can change a result (the unitarity tiers' thresholds, GF_UNI_DUMP) are honoured only under GF_DIAGNOSTICS=1 and listed
 * as "NAME(ignored)" otherwise; bench.py and scan.py print the list in their JSON line. */
int gf_diagnostic_overrides(char* buf, size_t buflen);
int gf_device_count(int* count);
/* ABI 3.  Hand back the device memory the library caches between uses on `device`: the unitarity workspaces of idle pooled
 * streams (up to 8 GiB) and pooled constant blocks -- *released_bytes (may be NULL) counts these -- and the 128 MB of pinned
 * host staging slots of gf_memcpy_d2h. */
int gf_device_trim(int device, size_t* released_bytes);
int gf_device_name(int device, char* buf, size_t buflen);   /* gcnArchName, e.g. "gfx950:..."   */

/* ---- model ------------------------------------------------------------------------------ */
/* Validates `desc`, derives the per-run constants (prior normalisations, Gaussian constants,
 * texture matrix, bin tables) and uploads them.  Replaces building the partial-bound ln_prob. */
int gf_model_create(const gf_model_desc* desc, int device, gf_model** out);
void gf_model_destroy(gf_model* m);
int gf_model_ndim(const gf_model* m);
int gf_model_nbins(const gf_model* m);   /* energy bins of a GF_MODE_BSM_GAUSS model, 0 for the other modes */

/* ---- the hot path, host buffers --------------------------------------------------------- */
/* lnprob[i] = ln_prob(theta[i]) for i < n.  Replaces the per-walker Python callback
 * (examples/inference.ipynb:356-364; golemflavor/llh.py:121-130; scripts/mc_unitary.py:134-143).
 * `fr` ([n][3], measured composition the likelihood saw) and `status` ([n]) may be NULL.
 * Synchronous: H2D, one kernel launch, D2H on the model's stream, then a stream sync. */
int gf_lnprob_batch(gf_model* m, const double* theta, int64_t n,
                    double* lnprob, double* fr, int32_t* status);

/* MultiNest-style batch, golemflavor/mn.py:26-45 lnProb(cube, ndim, n_params, ...): cube [n][nscan] lies in the unit
 * cube; column cols[k] of theta is lo + (hi - lo) * cube[.][k] (the model's own box of that column, mn.py:35-36), every
 * other column is base[col] (the paramset's current value, mn.py:37-39); then ln_prob.  The map runs on the device. */
int gf_lnprob_cube_batch(gf_model* m, const double* cube, int64_t n, int nscan, const int32_t* cols, const double* base,
                         double* lnprob, double* fr, int32_t* status);

/* fr[i] = measured flavor composition for theta[i]: chain post-processing of
 * scripts/mc_unitary.py:189-193 (u_to_fr(source_ratio, angles_to_u(x))) and
 * scripts/mc_texture.py:216-221 (flux_averaged_BSMu).  No priors, no likelihood. */
int gf_propagate_batch(gf_model* m, const double* theta, int64_t n, double* fr, int32_t* status);

/* n Haar-distributed mixing matrices: angles ~ U([0,1]^3 x [0,2pi]) (the flat-prior posterior that
 * scripts/mc_unitary.py samples by MCMC), propagated with source_ratio.  Counter-based Philox4x32-10
 * keyed by (seed, draw index): reproducible and independent of the launch geometry.
 * `angles` ([n][4]) may be NULL. */
int gf_haar_draw(gf_model* m, uint64_t seed, int64_t first_draw, int64_t n, double* angles, double* fr);

/* ---- device-resident variants (no PCIe in the timed region) ------------------------------ */
int gf_device_alloc(gf_model* m, size_t bytes, void** dptr);
int gf_device_free(gf_model* m, void* dptr);
int gf_memcpy_h2d(gf_model* m, void* dst_dev, const void* src_host, size_t bytes);  /* async + sync */
/* Synchronous.  From 16 MB on the copy brings its own staging: eight pinned 16 MB slots per device (allocated on first
 * use), filled by the DMA engine while host threads empty the earlier ones into dst_host -- so the rate (43-49 GB/s
 * measured) does not depend on whether dst_host is pinned, touched or fresh memory. */
int gf_memcpy_d2h(gf_model* m, void* dst_host, const void* src_dev, size_t bytes);
/* asynchronous on the model's stream; `layout` is a gf_layout */
int gf_lnprob_batch_device(gf_model* m, const double* d_theta, int layout, int64_t n,
                           double* d_lnprob, double* d_fr, int32_t* d_status);
int gf_propagate_batch_device(gf_model* m, const double* d_theta, int layout, int64_t n,
                              double* d_fr, int32_t* d_status);
int gf_haar_draw_device(gf_model* m, uint64_t seed, int64_t first_draw, int64_t n,
                        double* d_angles, double* d_fr);
/* Flavor-triangle histogram (golemflavor/plot.py:365-370, np.histogramdd on [0,1]^3 with `nbins` bins per
 * axis, last bin closed): counts[nbins][nbins][nbins] += ... ; the device variant is asynchronous and
 * accumulates, the host variant zeroes first. */
int gf_flavor_histogram_device(gf_model* m, const double* d_fr, int64_t n, int nbins, uint64_t* d_counts);
int gf_flavor_histogram(gf_model* m, const double* fr, int64_t n, int nbins, uint64_t* counts);
int gf_model_sync(gf_model* m);
/* Credible regions of the flavor triangle (golemflavor/plot.py:371-392: H / np.sum(H), scipy.ndimage.gaussian_filter, then argsort /
 * cumsum / searchsorted / mask), for `nchains` histograms d_counts [nchains][nbins]^3 (device; what gf_flavor_histogram_device fills) in
 * one set of launches.  H = count / total per cell (total < 2^53, else GF_ERR_UNSUPPORTED); smoothing = three passes of scipy's
 * correlate1d, mode 'reflect', with the 2 * radius + 1 weights the caller computed (golemflavor_amd.contour.gaussian_weights: scipy's
 * own expression, truncate 4.0); radius 0 (every sigma < 0.125, the reference's default 0.05 included) skips them, radius >
 * GF_REGION_MAX_RADIUS is GF_ERR_UNSUPPORTED.  The cells with H_s > 0 are ordered by descending H_s (equal values: descending flat index
 * (i * nbins + j) * nbins + k) and summed sequentially in fp64 in that order (np.cumsum).  Per chain and coverage[q] (percent, in
 * (0, 100], 1 <= ncov <= GF_REGION_MAX_COVERAGES, any order), host arrays [nchains][ncov], each may be NULL:
 *   thres      leading cells whose inclusive running sum is < coverage / 100. (np.searchsorted): the region; the cell that crosses
 *              the coverage is outside, as in the reference
 *   saturated  1: the sum never reaches coverage / 100. (coverage 100, or rounding): the reference's mask is the whole cube; thres is
 *              then the number of cells with H_s > 0
 *   level_in, level_out   H_s of the last cell inside / the first cell outside (NaN where there is none)
 *   mass       the running sum at the last cell inside (0 for an empty region)
 * and the region itself, host arrays [nchains][ncov][cap] (NULL = skip): flat indices `cells` and their H_s `density` in sorted order,
 * the first min(thres, cap) of them -- thres is always the true count, nothing is written past them.  An empty histogram (total == 0)
 * has no region: thres 0, saturated 0, mass 0, both levels NaN.  d_smoothed (device, [nchains][nbins]^3, may be NULL) receives H_s.
 * Synchronous. */
#define GF_REGION_MAX_RADIUS 32
#define GF_REGION_MAX_COVERAGES 8
int gf_flavor_region_device(gf_model* m, const uint64_t* d_counts, int nchains, int nbins, int radius, const double* weights,
                            const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in,
                            double* level_out, double* mass, int32_t* cells, double* density, double* d_smoothed);
/* the same for ONE chain of host compositions fr [n][3]: histogram (as gf_flavor_histogram), then its region */
int gf_flavor_region(gf_model* m, const double* fr, int64_t n, int nbins, int radius, const double* weights, const double* coverage,
                     int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                     int32_t* cells, double* density, double* d_smoothed);
/* Touch the pages of a freshly allocated host buffer from several threads (the content is preserved, and a copy may be filling
 * the buffer at the same time: madvise(MADV_POPULATE_WRITE), or a locked OR of zero per page where the kernel lacks it), so that a following
 * large device-to-host copy (gf_sampler_get_chain: sampler.chain of golemflavor/mcmc.py:43) runs at PCIe speed instead of
 * page-fault speed.  (gf_memcpy_d2h and gf_sampler_postprocess_rows do not need it: their staging threads map the pages.) */
int gf_host_prepare(void* buf, size_t bytes);
/* ABI 3.  The same with the number of threads chosen by the caller (<= 0: the default, up to 16): few threads when the mapping is to
 * run beside the caller's own launches and allocations, which many page-faulting threads hold up. */
int gf_host_prepare_n(void* buf, size_t bytes, int threads);
/* ABI 5.  A result ARENA: host memory of the caller's (a numpy array, a mapping of a shared segment) registered with the HIP runtime, so
 * that the DMA engines write the large read-backs -- sampler.chain (golemflavor/mcmc.py:43), the scans' rows -- STRAIGHT into it at the
 * speed of the PCIe link: no pinned staging ring, no host thread copying (57 GB/s against 28-47 through the ring on the boxes of the
 * pool; profiles/r04/host_register.txt).  Registering maps and pins every page (untouched 2 MiB-page memory: ~25 GB/s, touched: at
 * once; 4 KiB shared-memory pages ~11 GB/s), which is worth it for memory that receives MANY results: a process-lifetime arena
 * (golemflavor_amd.scan.ResultArena), each rank's region of the host segment of a multi-rank job.  Every read-back entry point finds out
 * by itself whether its destination is registered.  gf_host_unregister before the memory is freed or unmapped. */
int gf_host_register(void* buf, size_t bytes);
int gf_host_unregister(void* buf);

/* HIP events on the model's stream (what bench.py times the kernel with) */
int gf_event_create(void** ev);
int gf_event_destroy(void* ev);
int gf_event_record(gf_model* m, void* ev);
int gf_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);  /* synchronises on ev_stop */

/* ---- device-resident ensemble sampler ------------------------------------------------------ */
/* The emcee step either side of the path (golemflavor/mcmc.py:29-49: EnsembleSampler.sample / reset /
 * chain / acceptance_fraction), run entirely on the device: `nchains` independent ensembles of `nwalkers`
 * walkers of the model's posterior, affine-invariant stretch move (scale `a`, emcee's default 2.0),
 * Philox4x32-10 keyed by `seed`; the host sees chains at the end.  Launch shape is chosen per run and does not
 * change the chain: one launch per half-ensemble update (hipGraph replay), or -- small PRIOR_ONLY / SM_GAUSS
 * ensembles -- one workgroup per ensemble with the walkers in LDS and the whole run in one launch; small BSM
 * ensembles split a walker's energy bins over 4 or 16 lanes. */
typedef struct gf_sampler gf_sampler;
int gf_sampler_create(gf_model* m, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out);
/* One ensemble per model (grid scans: submitter/sens_dag.py:75-95 and mc_texture_dag.py:57-71 run one job per
 * grid point; here all of a GPU's grid points advance in one launch per half-step).  Chain ch samples the
 * posterior of models[ch]; the models share device, ndim and mode and must outlive the sampler. */
int gf_sampler_create_multi(gf_model* const* models, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out);
/* A sampler of the energy-resolved Gaussian likelihood: every model carries a binned measurement
 * (gf_model_set_binned_measurement; GF_ERR_INVALID_ARG naming the first model that carries none).  nmodels == 1: every chain
 * samples models[0]; nmodels == nchains: chain ch samples models[ch], under gf_sampler_create_multi's conditions.  The two calls
 * above refuse such a model (GF_ERR_UNSUPPORTED): this is the explicit way in.  The stored lnprob is bit for bit gf_lnprob_batch's of
 * the same model.  One launch shape, one launch per half-ensemble update.  The models' tables are taken here and keep their
 * addresses: a measurement set between two runs is what the next run samples.  Everything that reads a stored chain works as
 * for any sampler, except gf_sampler_reweight* with measurement targets (bestfit_fr / smearing / offset): GF_ERR_UNSUPPORTED,
 * such a chain has no single Gaussian measurement to replace; model targets work. */
int gf_sampler_create_binned(gf_model* const* models, int nmodels, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out);
/* A sampler of the tabulated flavour-plane likelihood: every model carries a table (gf_model_set_table_likelihood;
 * GF_ERR_INVALID_ARG naming the first model that carries none).  nmodels == 1: every chain samples models[0]; nmodels == nchains: chain
 * ch samples models[ch], under gf_sampler_create_multi's conditions; the tables' sides may differ from chain to chain.  The three calls
 * above refuse such a model (GF_ERR_UNSUPPORTED): this is the explicit way in.  The stored lnprob is bit for bit gf_lnprob_batch's of the
 * same model.  One launch shape, one launch per half-ensemble update; the lanes per walker follow the flux-averaged sampler's rule
 * (GF_SAMPLER_LPW forces a choice; any choice gives the same bits).  The tables stay in device memory.  The sampler keeps its models and
 * takes each one's table again at the start of every gf_sampler_run: a table set between two runs, of any side, is what the next run
 * samples (a table a larger one replaced is kept by its model until the model goes).  The walkers' stored lnprob is NOT recomputed then:
 * they hold the old table's values until they move or gf_sampler_set_state is called again.  Everything that reads a stored chain works
 * as for any sampler, except gf_sampler_reweight* with measurement targets: GF_ERR_UNSUPPORTED, such a chain has no Gaussian measurement
 * to replace; model targets work. */
int gf_sampler_create_table(gf_model* const* models, int nmodels, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out);
/* ---- tempered chains, replica exchange, stepping-stone series; additive in ABI 5 ----
 * lnprior and lnL of a BSM model apart: theta [n][ndim] -> lp, lnl, status [n].  lnl is the likelihood the model carries, as
 * gf_lnprob_batch evaluates it: the flux-averaged Gaussian, the energy-resolved one of a binned measurement or the
 * tabulated one (-inf at a hole of the table, with status GF_ST_OK).  status is gf_lnprob_batch's of the row, and where it
 * is GF_ST_OK the rounded sum lp + lnl is gf_lnprob_batch's lnprob bit for bit.  Outside the box lp = lnl = -inf; where the reference
 * would have raised lnl is NaN.  _device: device pointers, rows as [n][ndim].  Refused with GF_ERR_UNSUPPORTED and a message: any other
 * mode. */
int gf_model_lnprior_lnl(gf_model* m, const double* theta, int64_t n, double* lp, double* lnl, int32_t* status);
int gf_model_lnprior_lnl_device(gf_model* m, const double* d_theta, int64_t n, double* d_lp, double* d_lnl, int32_t* d_status);
/* A sampler of ngroups * ntemps chains: chain g * ntemps + t samples prior * L^betas[t] of group g's model (nmodels == 1: models[0] for
 * every group; nmodels == ngroups: models[g]).  betas [ntemps]: strictly decreasing, betas[0] == 1, the last >= 0, ntemps <= 64.  The
 * walker's scalar -- gf_sampler_get_state's lnprob, the stored lnprob chain -- is T = lp + beta * lnl, the product rounded, then the sum;
 * beta == 0 is T = lp with no product, so a point with lnl = -inf is a sample of the prior chain.  At beta == 1 T is gf_lnprob_batch's
 * lnprob bit for bit, and with betas = {1} the sampler is gf_sampler_create_multi's, chain for chain.  The unitarity verdict applies at
 * every beta.  swap_every == 0: no exchange; else a replica-exchange round follows the stored sample of every step i, counted since
 * creation, with (i + 1) % swap_every == 0: round r = (i + 1) / swap_every - 1 pairs walker w of rung t with walker w of rung t + 1 for
 * the t with t % 2 == r % 2, skips (and does not count) a pair with a walker at -inf, and exchanges the two rows iff
 * ln u < (beta_t - beta_t1) * (lnl_t1 - lnl_t); the draw is csrc/gf_temper.hpp's.  One launch shape (the per-half-step grid kernels).
 * Everything that reads a stored chain works as for any sampler.  Refused: models other than flux-averaged BSM models
 * (GF_ERR_UNSUPPORTED), a ladder or nmodels that break the rules above (GF_ERR_INVALID_ARG), each with a message. */
int gf_sampler_create_tempered(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers, uint64_t seed,
                               double a, int swap_every, gf_sampler** out);
/* gf_sampler_create_tempered for the energy-resolved likelihood (_binned: every model carries a binned measurement) and for the tabulated
 * flavour-plane likelihood (_table: every model carries a table; the sides may differ from group to group): the same parameters, the same
 * ladder rules, and L is that likelihood in the half-step, the rounds, gf_sampler_set_state and gf_sampler_tempered_series.  A model
 * that carries another likelihood is refused with gf_sampler_create_binned's / gf_sampler_create_table's code and wording; the call above
 * goes on refusing both kinds (GF_ERR_UNSUPPORTED).  A hole of a table (lnl = -inf) lies in the box: T = -inf at every beta > 0, T = lp at
 * beta == 0, where it is a sample of the prior chain.  _binned runs one lane per walker, _table the lanes of gf_sampler_create_table's rule.
 * _table takes each model's table again at the start of every gf_sampler_run, gf_sampler_set_state and gf_sampler_tempered_series, as
 * gf_sampler_create_table does per run; a model whose kind of likelihood changes under the live sampler is refused by all three
 * (GF_ERR_INVALID_ARG), the chain left as it is.  Additive in ABI 5. */
int gf_sampler_create_tempered_binned(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers, uint64_t seed,
                                      double a, int swap_every, gf_sampler** out);
int gf_sampler_create_tempered_table(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers, uint64_t seed,
                                     double a, int swap_every, gf_sampler** out);
/* lnl of every stored sample of a tempered sampler, reduced on the device over the walkers of a step: series [nchains][nstored][5] =
 * {walkers with a finite lnl, their sum, their max m, S_up = sum_w exp(d_up (lnl_w - m)), S_dn likewise with d_dn}, d_up and d_dn
 * [nchains] >= 0; a walker without a finite lnl contributes 0; the sums follow one fixed tree and the exp is the library's own
 * (csrc/gf_temper.hpp, bit for bit its host build).  lnl_chain (host) and d_lnl_chain (device), [nchains][nstored][nwalkers]: the
 * lnl themselves, either may be NULL.  GF_ERR_UNSUPPORTED for a sampler that is not tempered. */
int gf_sampler_tempered_series(gf_sampler* s, const double* d_up, const double* d_dn, double* series, double* lnl_chain, double* d_lnl_chain);
/* proposed, accepted [ngroups][ntemps]: the pairs (t, t + 1) of group g since the last gf_sampler_reset, at [g][t]; the last rung's
 * entries stay 0.  Either may be NULL. */
int gf_sampler_swap_counts(gf_sampler* s, uint32_t* proposed, uint32_t* accepted);
/* the ladder of a tempered sampler: *ngroups, *ntemps, *swap_every and betas [ntemps] (any may be NULL); GF_ERR_UNSUPPORTED otherwise */
int gf_sampler_betas(const gf_sampler* s, int* ngroups, int* ntemps, double* betas, int* swap_every);
/* Random stream of each chain, ids [nchains] (default: the chain's index in this sampler).  A grid scan passes the
 * global grid index, so that a grid point's chain is the same whichever rank runs it and whatever else shares its
 * sampler (the reference's jobs are seeded per job, scripts/mc_texture.py:137-138).  Before the first run. */
int gf_sampler_set_stream_ids(gf_sampler* s, const uint64_t* ids);
void gf_sampler_destroy(gf_sampler* s);
/* p0 [nchains][nwalkers][ndim]; evaluates its lnprob on the device (mcmc.py:34 sampler.sample(p0, ...)) */
int gf_sampler_set_state(gf_sampler* s, const double* pos);
/* nsteps stretch-move steps, asynchronous; store != 0 appends every thin-th step to the device chain */
int gf_sampler_run(gf_sampler* s, int64_t nsteps, int thin, int store);
int gf_sampler_sync(gf_sampler* s);
/* ABI 3.  gf_sampler_run(s, nsteps, thin, 1) with the read-back overlapped: while the GPU works through the run, every finished
 * block of 16 steps of all chains is copied to the host on a second stream (pinned staging, as gf_memcpy_d2h).  Synchronous: on
 * return the run is complete and chain [nchains][nstored][nwalkers][ndim], lnprob_chain [nchains][nstored][nwalkers] (may be
 * NULL) hold the whole stored chain, nstored = gf_sampler_nstored(s) after the call -- size them for
 * nstored_before + ceil(nsteps / thin).  Replaces run + sync + gf_sampler_get_chain where `sampler.chain` is read after
 * `sampler.run_mcmc` (golemflavor/mcmc.py:41-43).  *readback_tail_s (may be NULL): seconds from the end of the run on the GPU to the
 * end of the last copy, i.e. the part of the read-back that was not hidden behind the run. */
int gf_sampler_run_to_host(gf_sampler* s, int64_t nsteps, int thin, double* chain, double* lnprob_chain, double* readback_tail_s);
/* clears the stored chain and the acceptance counters, keeps the walkers (mcmc.py:36 sampler.reset()) */
int gf_sampler_reset(gf_sampler* s);
int64_t gf_sampler_nstored(const gf_sampler* s);
int64_t gf_sampler_iterations(const gf_sampler* s);
int gf_sampler_get_state(gf_sampler* s, double* pos, double* lnprob);
/* chain [nchains][nstored][nwalkers][ndim], lnprob_chain [nchains][nstored][nwalkers],
 * naccepted [nchains][nwalkers], nonunitary[1] = proposals the reference would have raised on (fr.py:493-498; they were
 * rejected: every proposal's unitarity verdict is settled on the device before its accept step, ABI 3); NULL = skip */
int gf_sampler_get_chain(gf_sampler* s, double* chain, double* lnprob_chain, uint32_t* naccepted, uint32_t* nonunitary);
/* the stored chain packed into caller-owned DEVICE buffers (what gf_comm_allgather sends); NULL = skip; synchronous */
int gf_sampler_get_chain_device(gf_sampler* s, double* d_chain, double* d_lnprob_chain);
/* mean [nchains][nstored][ndim]: ensemble mean of every stored step, the series behind sampler.acor
 * (golemflavor/mcmc.py:45-51), reduced on the device */
int gf_sampler_walker_mean(gf_sampler* s, double* mean);
/* Chain post-processing on the device (scripts/mc_unitary.py:189-193, scripts/mc_texture.py:216-221,
 * golemflavor/plot.py:365-370): composition of every stored sample and/or its [nbins]^3 histogram per
 * chain.  fr [nchains][nstored][nwalkers][3], status [nchains][nstored][nwalkers],
 * counts [nchains][nbins]^3; NULL = skip.
 * Scratch: where a request for the entry point's OWN device scratch is not granted, this entry point and
 * every other one that takes a sampler's stored chain (gf_sampler_postprocess*, _regions, _marginals,
 * _intervals, _element_marginals, _element_intervals, _spectrum) return GF_ERR_ALLOC with a message naming
 * the entry point and the size; earlier builds of these stored-chain entry points returned GF_ERR_HIP
 * with the failed call's text there.  The nested-posterior and reweighting entry points report it the same way.
 * The reducers underneath (marginals, intervals, elements, regions, the energy bins) still report a
 * refused request of theirs as GF_ERR_HIP. */
int gf_sampler_postprocess(gf_sampler* s, double* fr, int32_t* status, int nbins, uint64_t* counts);
/* same, chain ch propagated with models[ch] (NULL: the sampling models): scripts/mc_texture.py samples the
 * priors (:148-170) and pushes every sample through flux_averaged_BSMu of the grid point (:216-221) */
int gf_sampler_postprocess_with(gf_sampler* s, gf_model* const* models, double* fr, int32_t* status, int nbins,
                                uint64_t* counts);

/* The credible regions of every chain's stored samples (gf_flavor_region_device's outputs, [nchains] leading): chain ch is propagated
 * with models[ch] (NULL: the sampling models) and binned as gf_sampler_postprocess_with does, except that a sample the reference would
 * have raised on (status != 0; NaN in the rows a scan saves) is left out of the histogram; the counts of all chains stay on the device
 * and only the results cross PCIe. */
int gf_sampler_regions(gf_sampler* s, gf_model* const* models, int nbins, int radius, const double* weights, const double* coverage,
                       int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                       int32_t* cells, double* density);
/* same with DEVICE destinations d_fr [nchains][nstored][nwalkers][3], d_status (NULL = skip); synchronous */
int gf_sampler_postprocess_device(gf_sampler* s, gf_model* const* models, double* d_fr, int32_t* d_status);
/* the rows a scan saves, assembled on the device: d_rows [nchains][nstored][nwalkers][3 + ndim] = composition (NaN where the
 * reference would have raised) then the sample (scripts/mc_texture.py:216-223); synchronous */
int gf_sampler_postprocess_rows_device(gf_sampler* s, gf_model* const* models, double* d_rows);
/* the same rows in HOST memory, rows [nchains][nstored][nwalkers][3 + ndim]: the chains are post-processed one after the
 * other and every finished group of chains crosses PCIe while the next ones are still being evaluated (what a one-rank scan
 * hands to scripts/mc_texture.py's np.save); synchronous */
int gf_sampler_postprocess_rows(gf_sampler* s, gf_model* const* models, double* rows);

/* ---- device-resident nested sampler ------------------------------------------------------- */
/* The evidence golemflavor/mn.py:71-108 asks MultiNest for (scripts/sens.py runs it at every new-physics scale), computed on the
 * device for `nruns` independent runs in one set of launches.  Run r samples models[r] (one model per run: the null point of
 * sens.py:201,260-263 has its own box; all share device, ndim and mode and must outlive the sampler).  The prior is uniform on
 * the unit cube of the nscan columns cols[] (mn.py:22-23), theta = lo + (hi - lo) u on those (the model's box, mn.py:35-36), every
 * other column is bases[r][col] ([nruns][ndim]); the log-likelihood is the full ln_prob.  nlive <= 4096 live points; each
 * iteration removes the `batch` lowest (1 <= batch < nlive; the j-th removed point sees nlive - j live points) and replaces them
 * by constrained Metropolis walks of `walks` steps in the cube, proposal u + s C z with C the Cholesky factor of the survivors'
 * covariance.  Stops at ln(Z + L_max X) - ln Z < tol (default 0.01, mn.py:61) and adds the live set's X mean(L).  Philox4x32-10
 * keyed by `seed`, counter (run id, iteration, slot, step): a run's result is independent of the other runs.  on_nonunitary: 0 =
 * "raise" (a proposal the reference would have raised on, fr.py:493-498, ends that run and sets its `failed`), 1 = "-inf" (such
 * proposals lie outside the support and are counted). */
typedef struct gf_nested gf_nested;
int gf_nested_create(gf_model* const* models, int nruns, int nscan, const int32_t* cols, const double* bases, int nlive, int batch,
                     int walks, uint64_t seed, int on_nonunitary, gf_nested** out);
/* run ids [nruns] (default: the index in this sampler): a scan passes each point's index in its full list.  Before the first run. */
int gf_nested_set_run_ids(gf_nested* s, const uint64_t* ids);
/* evidence tolerance (mn.py:58-61 --mn-tolerance), default 0.01 */
int gf_nested_set_tolerance(gf_nested* s, double tol);
void gf_nested_destroy(gf_nested* s);
/* Synchronous: iterates until every run has met its tolerance.  More than max_iter iterations of one run: GF_ERR_UNSUPPORTED. */
int gf_nested_run(gf_nested* s, int64_t max_iter);
/* per run [nruns]: ln Z, its error sqrt(H / nlive + the compression variance of the zero-likelihood plateau), H, max lnL,
 * iterations, likelihood evaluations, proposals the reference would have raised on, failed (raise mode); NULL = skip */
int gf_nested_result(gf_nested* s, double* lnz, double* lnz_err, double* info, double* max_lnl, int64_t* niter, int64_t* nevals,
                     uint32_t* nonunitary, int32_t* failed);
/* run `run`'s dead points in removal order followed by its final live set: *n = iterations * batch + nlive rows of lnl, lnw
 * (log-weights) and cube [n][nscan]; NULL = skip; all NULL: only *n.  cap = rows the arrays hold. */
int gf_nested_get_dead(gf_nested* s, int run, int64_t cap, double* lnl, double* lnw, double* cube, int64_t* n);

/* ---- device multi-start Nelder-Mead maximiser (the profile likelihood) ------------------------------------------------------ */
/* The maximum of ln_prob over the unit cube of the nscan columns cols[] for `nruns` independent runs in one set of launches:
 * scripts/sens.py's frequentist statistic (golemflavor/plot.py:605-608).  Models, cols and bases as for gf_nested_create; f(u) =
 * -ln_prob(theta(u)) (-inf, NaN or a non-unitary verdict: +inf) is minimised from every start by scipy's bounded Nelder-Mead
 * (scipy.optimize._optimize._minimize_neldermead, bounds [0, 1]^n) step for step.  Starts: the nstarts best finite points of
 * nseed uniform cube points per run (Philox4x32-10 keyed by `seed`, counter (run id, ...)), then the caller's starts
 * (gf_simplex_set_starts); a run without a finite seed point and without caller's starts has max lnL = -inf and 0 starts.
 * on_nonunitary as for gf_nested_create, counted only for points scipy's sequential algorithm evaluates. */
typedef struct gf_simplex gf_simplex;
int gf_simplex_create(gf_model* const* models, int nruns, int nscan, const int32_t* cols, const double* bases, int nstarts,
                      int nseed, uint64_t seed, int on_nonunitary, gf_simplex** out);
/* run ids [nruns] (default: the index in this maximiser).  Before the first run. */
int gf_simplex_set_run_ids(gf_simplex* s, const uint64_t* ids);
/* nuser caller's starts per run, cube [nruns][nuser][nscan] (clipped to the cube as scipy clips x0).  Before the first run. */
int gf_simplex_set_starts(gf_simplex* s, int nuser, const double* cube);
/* scipy's xatol, fatol, maxiter (default 1e-4, 1e-4, 200 nscan) and adaptive coefficients (0/1, default 0); restarts: how many
 * times a converged start begins again from its best vertex with a fresh simplex (stopping when the gain is <= fatol).  Before
 * the first run. */
int gf_simplex_set_options(gf_simplex* s, double xatol, double fatol, int maxiter, int adaptive, int restarts);
void gf_simplex_destroy(gf_simplex* s);
/* Synchronous: at most max_rounds evaluation rounds in this call (one per Nelder-Mead iteration, one more per shrink); returns
 * when every start of every run is done or the rounds are used up.  A later call continues. */
int gf_simplex_run(gf_simplex* s, int64_t max_rounds);
/* per run [nruns]: max lnL, its cube point [nruns][nscan], starts used, iterations and scipy's nfev summed over the starts,
 * device evaluations (seed points included), non-unitary points counted, candidates whose unitarity verdict the emulated-x87
 * settlement took (evaluated or speculative), failed (raise mode); NULL = skip */
int gf_simplex_result(gf_simplex* s, double* max_lnl, double* argmax_cube, int32_t* nstarts, int64_t* niter, int64_t* nfev,
                      int64_t* nevals, uint32_t* nonunitary, uint32_t* parked, int32_t* failed);
/* run `run`'s starts [nstarts + nuser]: final f (+inf for an unused start), final cube point [..][nscan], nit, nfev; NULL = skip */
int gf_simplex_get_starts(gf_simplex* s, int run, double* fun, double* cube, int32_t* nit, int64_t* nfev);

/* ---- posterior marginals of a chain (the numbers behind golemflavor/plot.py:450-469 plot_Tchain) ---------------------------- */
/* Every chain's rows [nrows][width] reduced on the device to its 1-D and 2-D histograms, moments, order statistics and the
 * credible regions of each marginal.  getdist (the reference's plotter) is not a dependency, so the definition is this
 * package's own, stated in numpy's terms:
 *   counts1 [nchains][width][nbins1]            np.histogram(x_c, bins=nbins1, range=(lo_c, hi_c)): bin b holds edge[b] <= v <
 *                                               edge[b + 1], the last bin closed on the right, decided by comparison with the
 *                                               caller's edges1 [width][nbins1 + 1] (np.linspace(lo, hi, nbins1 + 1));
 *   counts2 [nchains][npairs][nbins2][nbins2]   np.histogram2d(x_i, x_j) over edges2 [width][nbins2 + 1] for the pairs i < j in
 *                                               lexicographic order, npairs = width (width - 1) / 2; a value outside its
 *                                               range or NaN drops the sample from that column's histogram and from every
 *                                               pair with that column;
 *   nvalid [nchains], mean [nchains][width], cov [nchains][width][width]
 *                                               over the rows without a NaN in any column; cov is two-pass, centred on the
 *                                               device mean, ddof = 1; both sums follow one fixed tree (4096-row leaves), so
 *                                               they do not depend on the launch;
 *   ncol [nchains][width]                       the column's non-NaN values;
 *   orank, ostat [nchains][width][nranks + 2 nq]
 *                                               exact order statistics (radix select on the order-preserving key of the
 *                                               double, no interpolation in a histogram) of the column's non-NaN values:
 *                                               first the caller's ranks (k >= 0 from the bottom, k < 0 from the top: -1 is the
 *                                               largest), then for every q (percent) the two neighbours floor(v) and
 *                                               min(floor(v) + 1, n - 1) of numpy's `linear` virtual index v = (n - 1) * (q /
 *                                               100); orank holds the rank used (-1 and NaN where there is none);
 *   regions                                     gf_flavor_region_device's reduction (H / sum, gaussian_filter of `radius` /
 *                                               `weights` along every axis longer than 1, descending sort with ties by
 *                                               descending flat index, sequential running sum) of every 1-D marginal
 *                                               ([nchains][width][ncov]) and 2-D marginal ([nchains][npairs][ncov]).  The
 *                                               regions of one marginal are prefixes of ONE sorted list, returned once:
 *                                               cells1 / density1 [nchains][width][cap1], cells2 / density2
 *                                               [nchains][npairs][cap2] hold its first min(cap, largest thres) entries
 *                                               (flat index b, or b_i * nbins2 + b_j).
 * Any output pointer may be NULL.  At most GF_MARGINAL_MAX_RANKS rank slots; nbins and width so large that one pair's
 * histogram (4 nbins2^2 bytes) plus the 1-D ones (4 width nbins1) exceed 64 KiB of LDS: GF_ERR_UNSUPPORTED. */
#define GF_MARGINAL_MAX_RANKS 16
typedef struct gf_marginal_spec {
    int32_t nbins1, nbins2;
    const double* edges1;       /* host [width][nbins1 + 1], strictly increasing */
    const double* edges2;       /* host [width][nbins2 + 1] */
    int32_t radius, ncov;       /* smoothing: as gf_flavor_region_device */
    const double* weights;      /* host [2 radius + 1], NULL when radius == 0 */
    const double* coverage;     /* host [ncov], percent */
    int32_t nranks, nq;
    const int64_t* ranks;       /* host [nranks] */
    const double* q;            /* host [nq], percent in [0, 100] */
    int64_t cap1, cap2;
} gf_marginal_spec;
typedef struct gf_marginal_out {
    uint64_t *counts1, *counts2;
    int64_t* nvalid;
    double *mean, *cov;
    int64_t *ncol, *orank;
    double* ostat;
    int64_t* thres1; int32_t* saturated1; double *level_in1, *level_out1, *mass1; int32_t* cells1; double* density1;
    int64_t* thres2; int32_t* saturated2; double *level_in2, *level_out2, *mass2; int32_t* cells2; double* density2;
} gf_marginal_out;
/* rows on the device, chain after chain: d_rows [nchains][nrows][width] */
int gf_marginals_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, const gf_marginal_spec* spec,
                        const gf_marginal_out* out);
/* host rows [nrows][width] of one chain: upload, then the same path */
int gf_marginals(gf_model* m, const double* rows, int64_t nrows, int width, const gf_marginal_spec* spec, const gf_marginal_out* out);
/* the stored chains of a sampler, width = ndim; with_fr != 0: the rows a scan saves (gf_sampler_postprocess_rows_device: chain ch
 * propagated with models[ch], NULL = the sampling models), width = 3 + ndim.  The rows stay on the device. */
int gf_sampler_marginals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out);

/* ---- rows in element space (golemflavor/plot.py:528-567, chainer_plot's --plot-elements table) ------------------------------- */
/* A row of sampled columns turned into the row the reference plots for --plot-elements: the four mixing columns (s12^2, c13^4,
 * s23^2, delta) become the nine moduli |U_ij| in row-major order e1 ... tau3 (fr.py:165-167 flat_angles_to_u: abs(angles_to_u(x))
 * cast to float32), the two source columns (sin^4 phi, cos 2psi) become the composition (phi_e, phi_mu, phi_tau) (fr.py:82-113
 * angles_to_fr, no cast), every other column is copied.  The plan lists the output row's groups in output order; which columns
 * form a group is the caller's choice (golemflavor_amd.elements.element_plan states this package's rule).
 *   GF_ELEMENT_COPY  col[0]      -> 1 value
 *   GF_ELEMENT_U9    col[0..3]   -> 9 values; each entry's real and imaginary parts are formed, then the modulus; a NaN, one of
 *                                   the first three outside [0, 1] or |delta| >= 1.6e6 gives NaN in all nine; round32 != 0 writes
 *                                   the reference's table, float32 values: (double)(float)v of the fp64 modulus v (absolute error
 *                                   of a few 1e-16), and for rows with a modulus below 2^-20, where that error exceeds a float32
 *                                   step, the float32 rounding of the modulus by the reference's own 80-bit route; 0 keeps the
 *                                   fp64 value v in every row
 *   GF_ELEMENT_FR3   col[0..1]   -> 3 values; a NaN in either column gives NaN in all three
 * 1 <= ngroups <= GF_ELEMENT_MAX_WIDTH, every column in [0, width_in), 1 <= width_in <= GF_MAX_DIM and an output row of at most
 * GF_ELEMENT_MAX_WIDTH values (what gf_marginals* reduces); anything else: GF_ERR_INVALID_ARG. */
#define GF_ELEMENT_MAX_WIDTH (GF_MAX_DIM + 3)
enum { GF_ELEMENT_COPY = 0, GF_ELEMENT_U9 = 1, GF_ELEMENT_FR3 = 2 };
typedef struct gf_element_group {
    int32_t kind;
    int32_t col[4];
} gf_element_group;
typedef struct gf_element_plan {
    int32_t ngroups, round32;
    gf_element_group group[GF_ELEMENT_MAX_WIDTH];
} gf_element_plan;
/* the plan's output width for rows of width_in columns; < 0: the plan is invalid */
int gf_element_plan_width(const gf_element_plan* plan, int width_in);
/* device rows d_in [nrows][width_in] -> d_out [nrows][width_out], both 8-byte aligned and not overlapping; synchronous */
int gf_element_rows_device(gf_model* m, const double* d_in, int64_t nrows, int width_in, const gf_element_plan* plan, double* d_out);
/* host rows: upload, the same path, download */
int gf_element_rows(gf_model* m, const double* rows, int64_t nrows, int width_in, const gf_element_plan* plan, double* out);
/* the stored chains of a sampler [nchains][nstored * nwalkers][ndim], transformed into a device buffer the library owns and reduced
 * by gf_marginals_device's path with width = the plan's output width; only the results come back, the stored chain is not touched */
int gf_sampler_element_marginals(gf_sampler* s, const gf_element_plan* plan, const gf_marginal_spec* spec, const gf_marginal_out* out);

/* ---- convergence diagnostics of stored chains (golemflavor/mcmc.py:45-51: the acceptance fraction and sampler.acor a job prints) -- */
/* Per chain and column of a stored chain [nsteps][nwalkers][ndim], with n = nsteps and L = maxlag (< 0: n - 1):
 *   A_w(t)     = sum_{i <= n-1-t} (x_i - m_w)(x_{i+t} - m_w) of walker w's series, t = 0 .. L
 *   rho(t)     = mean over the included walkers of A_w(t) / A_w(0); a walker series is excluded, and counted in nexcluded, if it holds
 *                a non-finite value or A_w(0) is zero (a walker that never moved) or not finite; none included: rho and tau are NaN
 *   tau        = taus(window), taus(M) = 2 sum_{t <= M} rho(t) - 1, window = the smallest M with M >= c taus(M), else L
 *   tau_mean, window_mean, rho_mean: the same of the ensemble-mean series (gf_sampler_walker_mean's, bit for bit)
 *   rhat       = split R-hat over the included walkers' first and second halves (n div 2 steps each; odd n: the middle step is in
 *                neither): sqrt(((h-1)/h W + B/h) / W); NaN for n < 4.  Walkers of one ensemble are not independent sequences: a
 *                diagnostic, not a guarantee.
 * Every sum has a fixed order (csrc/gf_diag.hpp) and no atomic is used: the results are the same bits whatever the grid and however
 * many chains are stacked.  The chain is only read.  nsteps < 2, nwalkers < 1, ndim outside [1, GF_MAX_DIM], c <= 0 or
 * maxlag >= nsteps: GF_ERR_INVALID_ARG; nsteps > 16384 (a series is held in LDS): GF_ERR_UNSUPPORTED -- thin the chain. */
typedef struct gf_diag_spec { double c; int64_t maxlag; } gf_diag_spec;      /* maxlag < 0: nsteps - 1 */
typedef struct gf_diag_out {                                                  /* every pointer may be NULL */
    double *tau, *tau_mean, *rhat;            /* [nchains][ndim] */
    int64_t *window, *window_mean;            /* [nchains][ndim] */
    int32_t *nexcluded;                       /* [nchains][ndim] */
    double *rho, *rho_mean;                   /* [nchains][ndim][maxlag + 1] */
} gf_diag_out;
/* device chains: chain ch starts at d_chain + ch * chain_stride (doubles); host destinations; synchronous */
int gf_chain_diagnostics_device(gf_model* m, const double* d_chain, int64_t chain_stride, int nchains, int64_t nsteps, int nwalkers, int ndim,
                                const gf_diag_spec* spec, const gf_diag_out* out);
/* one host chain [nsteps][nwalkers][ndim]: upload, the same path */
int gf_chain_diagnostics(gf_model* m, const double* chain, int64_t nsteps, int nwalkers, int ndim, const gf_diag_spec* spec,
                         const gf_diag_out* out);
/* the stored chains of a sampler, all in one chain loop; nothing stored: GF_ERR_INVALID_ARG */
int gf_sampler_diagnostics(gf_sampler* s, const gf_diag_spec* spec, const gf_diag_out* out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -------------------------------------- */
/* Independent chains (grid points) shard across ranks with no data-path collective; the only
 * exchanges are the broadcast of the packed descriptors at start and the gather of the chain blocks
 * at the end -- the role HTCondor + a shared filesystem play in the reference
 * (submitter/mc_texture_dag.py:57-71, submitter/sens_dag.py:75-95). */
typedef struct gf_comm gf_comm;
#define GF_COMM_ID_BYTES 128
int gf_comm_unique_id(uint8_t id[GF_COMM_ID_BYTES]);                 /* rank 0; ship to the others out of band */
int gf_comm_create(const uint8_t id[GF_COMM_ID_BYTES], int rank, int nranks, int device, gf_comm** out);
void gf_comm_destroy(gf_comm* c);
int gf_comm_broadcast(gf_comm* c, void* host_buf, size_t bytes, int root);            /* host in/out   */
int gf_comm_allgather(gf_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank); /* device  */
/* ABI 3.  Gather to one rank: rank r's block lands at d_recv_on_root + r * bytes_per_rank on `root` (NULL elsewhere); only the
 * root holds nranks x the block.  Stands in for the reference's N jobs saving N chain files to one place
 * (golemflavor/mcmc.py:108-126, submitter/mc_texture_dag.py:57-71): one ncclGroup of point-to-point transfers into the root. */
int gf_comm_gather(gf_comm* c, const void* d_send, void* d_recv_on_root, size_t bytes_per_rank, int root);
/* ABI 3.  The same gather without a communicator, for the ranks of ONE node: gf_ipc_export turns a rank's block (the base of a
 * gf_device_alloc'd buffer) into a 64-byte handle that travels over the caller's control plane; on the root gf_ipc_gather opens the
 * nranks handles (its own slot is ignored: d_own is copied), copies every block to d_recv + r * bytes_per_rank device to device --
 * over xGMI between GPUs -- and closes them.  The senders must keep their blocks until the root has returned (a barrier of the
 * control plane).  Fallback where RCCL cannot be set up; also the one inter-process device path a one-GPU box can exercise. */
#define GF_IPC_HANDLE_BYTES 64
int gf_ipc_export(const void* d_ptr, unsigned char* handle64);
int gf_ipc_gather(int device, const unsigned char* handles, int nranks, int self_rank, const void* d_own, void* d_recv,
                  size_t bytes_per_rank);
int gf_comm_barrier(gf_comm* c);
/* ABI 4.  What the COMMUNICATOR itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) -- the number a bench line
 * quotes as `rccl_nranks`: how many ranks RCCL saw, not how many the caller asked for.  Any pointer may be NULL. */
int gf_comm_info(gf_comm* c, int* nranks, int* rank, int* device);
/* ABI 4.  Device memory without a model handle (the hipIpc probe of golemflavor_amd.dist allocates its 16 bytes before any
 * posterior exists): hipMalloc / hipFree on `device`. */
int gf_device_malloc(int device, size_t bytes, void** dptr);
int gf_device_release(int device, void* dptr);
const char* gf_comm_last_error(void);                 /* thread-local text of the last failing gf_comm_* call */
int gf_comm_library_info(char* buf, size_t buflen);   /* "<ncclGetVersion code> <path of the loaded librccl>" */

/* ---- the posterior of every run of a nested sampler (csrc/gf_nested_post.hpp holds the arithmetic) --------------- */
/* A run's points are gf_nested_get_dead's rows in its order (n = iterations * batch + nlive).  With m = max lnw: e_i = exp(lnw_i - m)
 * (lnw = -inf: 0 exactly), S = sum e, S2 = sum e^2, p_i = e_i / S, ess = S^2 / S2 (Kish), lnz_check = m + log(S); mean =
 * np.average(theta, axis=0, weights=p) and cov = np.cov(theta.T, aweights=p) over the full-width theta (a column that is not scanned
 * has its value as mean and zero covariances, exactly); every sum along one fixed tree.  Equal-weight rows by systematic resampling:
 * C = the inclusive prefix of p in a fixed blocked order, u in [0, 1) from Philox4x32-10 with the sampler's key and counter (run id,
 * 0xFFFFFFFE, 0, 0), t_k = (k + u) / nrows, row k = the point min(first i with C_i > t_k, n - 1).  A run without a posterior (not run
 * to its end, failed in raise mode, ln Z = -inf) has npoints 0, ess 0, NaN moments, NaN rows and index -1; the call is GF_OK for
 * the others.  nrows < 1 or a NULL sampler: GF_ERR_INVALID_ARG; device scratch that is not granted: GF_ERR_ALLOC with a message.
 * The models of gf_nested_create must still be open.  All synchronous, on the sampler's stream; the sampler's state is only read. */
/* per run: npoints, ess, lnz_check [nruns], mean [nruns][ndim], cov [nruns][ndim][ndim]; NULL = skip */
int gf_nested_posterior(gf_nested* s, int64_t* npoints, double* ess, double* lnz_check, double* mean, double* cov);
/* d_rows [nruns][nrows][(with_fr ? 3 : 0) + ndim] on the device: with_fr puts the composition of models[r] in front (NaN where the
 * reference would have raised), the layout of gf_sampler_postprocess_rows_device */
int gf_nested_posterior_rows_device(gf_nested* s, int64_t nrows, int with_fr, double* d_rows);
/* the same rows in host memory, and index [nruns][nrows] (NULL = skip): the point every row came from */
int gf_nested_posterior_rows(gf_nested* s, int64_t nrows, int with_fr, double* rows, int64_t* index);
/* the marginals (gf_marginals_device, nchains = nruns) of those rows, which stay on the device */
int gf_nested_marginals(gf_nested* s, int64_t nrows, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out);
/* the marginals of the theta rows in element space (gf_element_rows_device, then gf_marginals_device) */
int gf_nested_element_marginals(gf_nested* s, int64_t nrows, const gf_element_plan* plan, const gf_marginal_spec* spec,
                                const gf_marginal_out* out);
/* the flavor-triangle credible regions (gf_sampler_regions' outputs, [nruns] leading) of every run's rows propagated with its model */
int gf_nested_regions(gf_nested* s, int64_t nrows, int nbins, int radius, const double* weights, const double* coverage, int ncov,
                      int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass, int32_t* cells,
                      double* density);

/* ---- the evidence of every run under other Gaussian measurements (csrc/gf_ns_toys.hpp holds the arithmetic) ---------- */
/* Additive under ABI 5.  The runs' points (gf_nested_get_dead's rows in its order) reweighted to `ntoys` realisations of the runs'
 * Gaussian measurement: Z_t = sum_i exp(x_ti), x_ti = lnw_i + (l_t(fr_i) - l_0(fr_i)), with fr_i the composition of point i under the
 * run's own model (one propagation of all points), l_0 the Gaussian block of ln_prob under the run's own measurement and l_t the same
 * function under realisation t (bf, smearing; the constants by the rule of gf_model_create), the likelihood offset the run's.  A point
 * carries no weight (x = -inf) where lnw_i = -inf, where the reference would have raised on it (GF_ST_NON_UNITARY), where l_0 is not
 * finite, or where l_t is NaN or -inf.  Per (run, realisation): m = max_i x, s = sum exp(x - m), s2 = sum exp(x - m)^2 along
 * gf_nested_posterior's tree, ess = s^2 / s2 (Kish), kept = the points with a finite x; ln Z_t = m + log(s) is the caller's.  A
 * realisation whose (bf, smearing) are the run's own reproduces gf_nested_posterior's lnz_check and ess bit for bit.  No kept point:
 * m = -inf, s = s2 = 0, ess = 0.  A run without points (not run to its end, failed in raise mode, ln Z = -inf): m, s, s2 NaN, ess 0,
 * kept 0.
 *   bf        [ntoys][3] shared by the runs, or [nruns][ntoys][3] with per_run = 1
 *   smearing  [ntoys]
 *   outputs   [nruns][ntoys] each; NULL = skip
 * Models without a flux-averaged Gaussian measurement (PRIOR_ONLY, a binned measurement): GF_ERR_UNSUPPORTED; a measurement that is
 * not finite or a smearing that is not positive and finite: GF_ERR_INVALID_ARG.  The realisations go through the device in batches
 * whose partial sums stay under 256 MiB of scratch (GF_NS_TOYS_SCRATCH_BYTES overrides); no result depends on the batching, on
 * ntoys or on the runs that share the sampler.  Synchronous, on the sampler's stream; the sampler's state is only read. */
int gf_nested_toys_evidence(gf_nested* s, const double* bf, const double* smearing, int ntoys, int per_run, double* m, double* sum,
                            double* sum2, double* ess, int64_t* kept);

/* ---- the shortest interval around the mode of every column (golemflavor/misc.py:174-213) ------------------------- */
/* Per chain and column of rows [nrows][width], with s the sorted column and n = nrows (csrc/gf_interval.hpp states every operation):
 *   nbins    = floor((s[n-1] - s[0]) / (2 * n**(-1/3) * (p75 - p25))), p25 / p75 np.percentile's default (calc_nbins)
 *   center   = the centre of the FIRST bin of maximal count of np.histogram(s, np.linspace(s[0], s[n-1] + 2, nbins + 1)) (most_likely)
 *   low, up  = s[curr_low], s[curr_up] of misc.interval's walk from the first index nearest to center, for every percentile
 *   nunique  = the number of distinct values (np.unique(column).shape, mcmc.py:47)
 *   status   per (column, percentile): 0 ok; 1 the column holds a NaN or an infinity (this library's rule: low, up, center NaN,
 *            nbins and nunique -1); 2 nbins is NaN, infinite or below 1, where the reference raises before the walk (a constant
 *            column, a zero interquartile range, one row; nbins -1 for NaN); 3 the walk would index s[n], where the reference raises
 *            IndexError (percentile 100, tiny n); 4 nbins above GF_INTERVAL_MAX_BINS, unsupported.  For 2 to 4 low and up are NaN
 *            and center is given where it exists (3).
 * The columns are sorted by a segmented radix sort on the device; the rows are only read.  Two key buffers per batch of chains come
 * from the library's device cache, and the chains are processed batch after batch so that they stay under 2 GiB (one chain at
 * least); no result depends on the batching.  width outside [1, GF_ELEMENT_MAX_WIDTH], nrows < 1, npct outside
 * [1, GF_INTERVAL_MAX_PERCENTILES] or a percentile outside (0, 100]: GF_ERR_INVALID_ARG; nrows >= 2^31: GF_ERR_UNSUPPORTED. */
#define GF_INTERVAL_MAX_BINS (1 << 20)
#define GF_INTERVAL_MAX_PERCENTILES 8
typedef struct gf_interval_spec { int32_t npct; const double* percentile; /* host [npct], percent in (0, 100] */ } gf_interval_spec;
typedef struct gf_interval_out {                                              /* every pointer may be NULL */
    double *low, *up;                         /* [nchains][width][npct] */
    int32_t* status;                          /* [nchains][width][npct] */
    double* center;                           /* [nchains][width] */
    int64_t *nbins, *nunique;                 /* [nchains][width] */
} gf_interval_out;
/* device rows d_rows [nchains][nrows][width] -> d_sorted [nchains][width][nrows], every column ascending (-0.0 before +0.0, NaN
 * last); both 8-byte aligned and not overlapping; synchronous */
int gf_sort_columns_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, double* d_sorted);
/* rows on the device, chain after chain: d_rows [nchains][nrows][width]; host destinations; synchronous */
int gf_column_intervals_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, const gf_interval_spec* spec,
                               const gf_interval_out* out);
/* host rows [nrows][width] of one chain: upload, then the same path */
int gf_column_intervals(gf_model* m, const double* rows, int64_t nrows, int width, const gf_interval_spec* spec, const gf_interval_out* out);
/* the stored chains of a sampler: gf_sampler_marginals' rows (width = ndim, or 3 + ndim with_fr); nothing stored: GF_ERR_INVALID_ARG */
int gf_sampler_intervals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out);
/* the stored chains in element space: gf_sampler_element_marginals' rows */
int gf_sampler_element_intervals(gf_sampler* s, const gf_element_plan* plan, const gf_interval_spec* spec, const gf_interval_out* out);
/* the equal-weight rows of gf_nested_posterior_rows_device, nchains = nruns; a run without a posterior has NaN rows: status 1 */
int gf_nested_intervals(gf_nested* s, int64_t nrows, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out);

/* ---- the composition at every energy bin (golemflavor/fr.py:441-457 before its mean) ---------------------------------- */
/* flux_averaged_BSMu evaluates u_to_fr(source, params_to_BSMu(..., energy = E_k)) at the centre E_k = sqrt(b_k b_{k+1}) of every bin
 * (fr.py:413) and returns the width-weighted mean; these entry points return the nbins = gf_model_nbins(m) terms themselves, the same
 * arithmetic bit for bit: (f_e, f_mu) as the average forms them and f_tau = (1 - f_e) - f_mu.  Values only: a row the reference
 * would have raised on (fr.py:398-399 raises inside flux_averaged_BSMu at the FIRST failing bin, so such a sample has no composition
 * at any energy) is one whose status by the existing propagate path is not GF_ST_OK, and it gets NaN in EVERY bin.  A model that
 * is not GF_MODE_BSM_GAUSS: GF_ERR_UNSUPPORTED. */
/* d_fr_bins [n][nbins][3], or bin-major [nbins][n][3] (bin_major != 0); d_status [n] as gf_propagate_batch_device wrote it for the
 * same rows, or NULL: nothing is masked.  Asynchronous on the model's stream. */
int gf_propagate_bins_device(gf_model* m, const double* d_theta, int layout, int64_t n, double* d_fr_bins, int bin_major,
                             const int32_t* d_status);
/* host rows: upload, the existing propagate for the status (status != NULL), the kernel, download.  fr_bins [n][nbins][3], status [n] */
int gf_propagate_bins(gf_model* m, const double* theta, int64_t n, double* fr_bins, int32_t* status);
/* The posterior of the composition as a function of energy.  Per chain and energy bin k the rows (f_e, f_mu, f_tau)_k of the chain's
 * samples are reduced as gf_marginals_device reduces the rows of a chain (same kernels, the energy bins taking the place of the
 * chains): histograms np.histogram(f, bins = nbins1, range = (0, 1)) per flavour, nvalid / mean / cov (ddof 1) over the samples with
 * a composition, and for every q (percent) the two order statistics np.percentile's `linear` rule reads.  Host arrays, each may be
 * NULL, nbinsE = the model's energy bins (the same for every chain):
 *   nvalid [nchains][nbinsE], mean [nchains][nbinsE][3], cov [nchains][nbinsE][3][3],
 *   ostat, orank [nchains][nbinsE][3][2 nq], counts [nchains][nbinsE][3][nbins1]
 * nbins1 in [1, 1024], nq <= GF_MARGINAL_MAX_RANKS / 2. */
typedef struct gf_spectrum_spec { int32_t nbins1, nq; const double* q; /* host [nq], percent in [0, 100] */ } gf_spectrum_spec;
typedef struct gf_spectrum_out {
    int64_t* nvalid;
    double *mean, *cov;
    double* ostat; int64_t* orank;
    uint64_t* counts;
} gf_spectrum_out;
/* every stored chain of a sampler, chain ch evaluated with models[ch] (NULL: the sampling models), chain after chain on the sampler's
 * stream through ONE bin-major slab [nbinsE][nstored nwalkers][3] of scratch (plus the status array and the reduction's buffers);
 * nothing stored: GF_ERR_INVALID_ARG; synchronous */
int gf_sampler_spectrum(gf_sampler* s, gf_model* const* models, const gf_spectrum_spec* spec, const gf_spectrum_out* out);
/* the nrows equal-weight posterior rows of every run (gf_nested_posterior_rows_device), nchains = nruns; a run without a posterior
 * has nvalid 0 and NaN moments */
int gf_nested_spectrum(gf_nested* s, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out);

/* ---- the energy-resolved Gaussian likelihood: a measurement per energy bin (this package's own definition) ------------- */
/* A GF_MODE_BSM_GAUSS model with K = gf_model_nbins(m) energy bins takes a composition m_k[3] and a width sigma_k > 0 per bin.  From
 * then on every lnprob the model gives -- gf_lnprob_batch[_device], gf_lnprob_cube_batch, the nested sampler, the maximiser, a model
 * target of gf_sampler_reweight* -- is
 *     lnprior + offset + sum_{k = 0..K-1} multi_gaussian(fr_k(theta), m_k, sigma_k, offset = 0),
 * fr_k being bin k of gf_propagate_bins, each term the reference's multi_gaussian (llh.py:32-54) with its underflow wall, the terms
 * added in ascending k from 0.0; one bin at -inf makes the sum -inf.  The status of a row, and the value of a row the reference would
 * have raised on, are those of the same model without the measurement.  Propagation, the spectrum and post-processing are unchanged
 * (the mode stays GF_MODE_BSM_GAUSS, bestfit_fr and smearing stay in the model and are not read by lnprob).
 * fr_bins [nbins][3] finite, sigma [nbins] > 0 and finite, nbins == gf_model_nbins(m): else GF_ERR_INVALID_ARG; a model of another
 * mode: GF_ERR_UNSUPPORTED; either way the model is unchanged.  A measurement can be replaced (no launch of the model may be in flight
 * on a stream other than its own) but not removed.  gf_sampler_create[_multi] refuses such a model (GF_ERR_UNSUPPORTED): the ensemble
 * sampler's posterior under this likelihood is reached by reweighting its chain to the model. */
int gf_model_set_binned_measurement(gf_model* m, int nbins, const double* fr_bins, const double* sigma);
int gf_model_is_binned(const gf_model* m);   /* 1 with a binned measurement, 0 without, -1 for NULL */

/* ---- the tabulated flavour-plane likelihood: bring your own likelihood surface (this package's own definition) -------- */
/* A GF_MODE_BSM_GAUSS model takes ln L at the (nside + 1)(nside + 2) / 2 nodes (i, j), 0 <= j <= nside - i, of the flavour triangle's
 * lattice -- node (i, j) is (fr_e, fr_mu) = (i, j) / nside and lies at values[i (2 nside + 3 - i) / 2 + j].  From then on every lnprob the
 * model gives -- gf_lnprob_batch[_device], gf_lnprob_cube_batch, the nested sampler, the maximiser, a model target of gf_sampler_reweight*
 * -- is lnprior + the table's value at the flux-averaged composition, linearly interpolated in the triangle of the lattice that holds it
 * (csrc/gf_table.hpp holds the operations and their order); a triangle with a node at -inf gives -inf, a NaN composition NaN.  The
 * model's offset is not added.  The status of a row, the composition, and the value of a row the reference would have raised on are those
 * of the same model without the table (the mode stays GF_MODE_BSM_GAUSS, bestfit_fr and smearing stay in the model and are not read by
 * lnprob).
 * 1 <= nside <= GF_TABLE_MAX_NSIDE, every value finite or -inf and one of them finite: else GF_ERR_INVALID_ARG.  A model of another mode,
 * or one with a binned measurement: GF_ERR_UNSUPPORTED (and gf_model_set_binned_measurement refuses a model with a table); either way
 * the model is unchanged.  A table can be replaced (no launch of the model may be in flight on a stream other than its own; a nested
 * sampler or maximiser created earlier reads the new one if it has not run yet, and once its runs have begun its next gf_nested_run /
 * gf_simplex_run is GF_ERR_INVALID_ARG -- a run that has begun does not change likelihood, its results so far stay readable; an
 * ensemble sampler of gf_sampler_create_table reads the new one from its next run on) but not removed.  A model that gains its first
 * table, or its first binned measurement, after a sampler, nested sampler, maximiser or seed set was created over it is refused by
 * that handle's next set_state / run / seed call (GF_ERR_INVALID_ARG naming the model; what the handle holds stays readable).
 * The ensemble sampler samples such a model through gf_sampler_create_table alone.
 * Refused with GF_ERR_UNSUPPORTED: gf_sampler_create, gf_sampler_create_multi and gf_sampler_create_binned (their kernels evaluate another
 * likelihood), and what sets or reweights to a Gaussian measurement -- gf_toys_create*, gf_toys_set_measurements, gf_toys_set_binned_measurements,
 * gf_nested_toys_evidence.  Of the models of one nested sampler or maximiser all carry a table or none; the sides may differ. */
#define GF_TABLE_MAX_NSIDE 2048
int gf_model_set_table_likelihood(gf_model* m, int nside, const double* values);
int gf_model_table_nside(const gf_model* m);   /* the table's side, 0 without one (and for NULL) */

/* ---- every stored chain reweighted to other targets (csrc/gf_reweight.hpp holds the rules for lnw) ------------------- */
/* Chain c's rows are its stored samples in the device's order, i = step * nwalkers + walker, n = nstored * nwalkers (NOT emcee's
 * walker-major flatchain; every index below refers to this order), l0_i their stored ln_prob.  Every chain has ntargets targets t.
 *   model targets        models != NULL: l_t and the row's status are models[c][t]'s lnprob (the kernels of gf_lnprob_batch_device) on
 *                        the rows in place; lnw = l_t - l0, one rounded subtraction.  Each model has the sampler's ndim and device.
 *   measurement targets  models == NULL: target (c, t) is the chain's own sampling model with bestfit_fr, smearing and offset replaced;
 *                        the sampling model must be GF_MODE_SM_GAUSS or GF_MODE_BSM_GAUSS (else GF_ERR_INVALID_ARG).  The chain is
 *                        propagated ONCE; lnw = mg(fr_i; target) - mg(fr_i; sampling model), mg the Gaussian block of lnprob (the
 *                        priors cancel).  smearing must be > 0 and bestfit_fr finite.
 * lnw = -inf, counted once under the first rule that holds: bad_base[c] (l0, or the sampling model's mg, is not finite),
 * nonunitary[c][t] (the row's status under the target is GF_ST_NON_UNITARY), outside[c][t] (l_t is -inf or NaN).
 * From lnw on it is gf_nested_posterior's arithmetic unchanged, with no fixed columns: ess (Kish), mean, cov, the prefix C, and
 * equal-weight rows at t_k = (k + u) / nrows with u = Philox(seed; stream_id(c) * GF_REWEIGHT_MAX_TARGETS + t), seed the sampler's
 * unless use_sampler_seed == 0 -- so the rows of (c, t) do not depend on which other chains or targets share the call.
 * lnz_ratio = m + log(S) - log(n), a diagnostic that estimates ln(Z_t / Z_0); it is a Bayes factor only for model targets on the same
 * data.  A target all of whose weights are zero has no posterior: ess 0, lnz_ratio, mean, cov and rows NaN, index -1.
 * Chains go one after another on the sampler's stream; scratch per chain is its compositions and status plus three doubles per (target,
 * row), cut into batches of targets to stay under 2 GiB (GF_REWEIGHT_SCRATCH_BYTES overrides; no result depends on it).  Synchronous;
 * the sampler is only read.  Nothing stored, ntargets outside [1, GF_REWEIGHT_MAX_TARGETS]: GF_ERR_INVALID_ARG. */
#define GF_REWEIGHT_MAX_TARGETS 64
typedef struct gf_reweight_spec {
    int32_t ntargets;
    int32_t use_sampler_seed;            /* != 0: `seed` is ignored */
    uint64_t seed;
    gf_model* const* models;             /* [nchains][ntargets], or NULL: measurement targets */
    const double* bestfit_fr;            /* [nchains][ntargets][3] */
    const double* smearing;              /* [nchains][ntargets] */
    const double* offset;                /* [nchains][ntargets] */
} gf_reweight_spec;
typedef struct gf_reweight_out {         /* host; every pointer may be NULL */
    double *ess, *lnz_ratio;             /* [nchains][ntargets] */
    double* mean;                        /* [nchains][ntargets][ndim] */
    double* cov;                         /* [nchains][ntargets][ndim][ndim] */
    int64_t* bad_base;                   /* [nchains] */
    int64_t *nonunitary, *outside;       /* [nchains][ntargets] */
    int64_t* n;                          /* [nchains] */
} gf_reweight_out;
int gf_sampler_reweight(gf_sampler* s, const gf_reweight_spec* spec, const gf_reweight_out* out);
/* the log-weights of one chain, lnw [ntargets][n] on the host: for tests and for estimators of the caller's own */
int gf_sampler_reweight_lnw(gf_sampler* s, const gf_reweight_spec* spec, int chain, double* lnw);
/* d_rows [nchains][ntargets][nrows][(with_fr ? 3 : 0) + ndim] on the device; with_fr puts the row's composition under the target in
 * front (measurement targets: gathered from the chain's one propagation; model targets: the nrows rows propagated with the target) */
int gf_sampler_reweight_rows_device(gf_sampler* s, const gf_reweight_spec* spec, int64_t nrows, int with_fr, double* d_rows);
/* the same rows in host memory, and index [nchains][ntargets][nrows] (NULL = skip): the row of the chain each came from */
int gf_sampler_reweight_rows(gf_sampler* s, const gf_reweight_spec* spec, int64_t nrows, int with_fr, double* rows, int64_t* index);
/* the reductions of those rows, which stay on the device, with nchains * ntargets in place of nchains: gf_marginals_device,
 * gf_column_intervals_device, and gf_sampler_regions' outputs of the rows' compositions */
int gf_sampler_reweight_marginals(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int with_fr, const gf_marginal_spec* spec,
                                  const gf_marginal_out* out);
int gf_sampler_reweight_intervals(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int with_fr, const gf_interval_spec* spec,
                                  const gf_interval_out* out);
int gf_sampler_reweight_regions(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int nbins, int radius, const double* weights,
                                const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in,
                                double* level_out, double* mass, int32_t* cells, double* density);

/* ---- realisation ensembles: the shared seeding of many mock measurements --------------------------------- */
/* A realisation of a Gaussian measurement (bf, smearing) is m = bf + smearing z, z ~ N(0, I_3) (thrown by the caller).  Profiling T of
 * them at S scales needs S * T maximisations, but a seed point's composition, prior sum and unitarity verdict do not depend on the
 * measurement: gf_toys draws and evaluates the nseed seed points of every scale once (the points gf_simplex_create's seeding draws for
 * the same seed and run id, evaluated by the scale model's bulk path), and gf_toys_select ranks them under every realisation:
 *   score(t, i) = lp_i + gauss(m_t, fr_i), lnprob's own two operations, -inf for a seed the reference would have raised on and for NaN;
 *   the starts of (scale, t) are the K <= GF_TOY_MAX_STARTS best seeds with a score > -inf, score descending then seed index ascending.
 * The polish is gf_simplex with nstarts = 0, nseed = 0, the scale's model once per realisation, the selected cube points as the
 * caller's starts and gf_toys_set_measurements.  Models as for gf_simplex_create (one per scale); flux-averaged Gaussian
 * likelihoods only (binned measurement, PRIOR_ONLY: GF_ERR_UNSUPPORTED), one likelihood offset for all. */
#define GF_TOY_MAX_STARTS 16
/* A measurement of its own for every run of a maximiser: bf [nruns][3] and smearing [nruns] replace the Gaussian measurement of run r's
 * model in that run's kernels, with the constants gf_model_create derives, so the run evaluates exactly what a model compiled with
 * (bf_r, smearing_r) evaluates.  Before the first gf_simplex_run.  Refused: a smearing that is not positive and finite, a bf that is not
 * finite, models with a binned measurement or without a Gaussian one (GF_ERR_UNSUPPORTED), and a maximiser created with nseed > 0 --
 * its seeding goes through the models' own lnprob and would score under their measurement. */
int gf_toys_set_measurements(gf_simplex* s, const double* bf, const double* smearing);
/* counts [nruns], each 0 .. nuser: run r keeps the first counts[r] of its caller's starts (gf_simplex_set_starts; the rows behind them
 * are read but never evaluated, give them any finite value) -- a realisation with fewer finite seeds than K has fewer starts.  For a
 * maximiser created with nstarts = 0; after gf_simplex_set_starts (should a later gf_simplex_set_starts give fewer starts, a run keeps at
 * most those), before the first gf_simplex_run. */
int gf_toys_set_start_counts(gf_simplex* s, const int32_t* counts);
typedef struct gf_toys gf_toys;
int gf_toys_create(gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed, uint64_t seed,
                   gf_toys** out);
void gf_toys_destroy(gf_toys* t);
/* run ids [nscales] (default: the index): the Philox stream of each scale's seeds.  Before gf_toys_seed. */
int gf_toys_set_run_ids(gf_toys* t, const uint64_t* ids);
/* Draws and evaluates the seeds, once.  nonunitary [nscales] (NULL = skip): the seeds the reference would have raised on.  Synchronous. */
int gf_toys_seed(gf_toys* t, uint32_t* nonunitary);
/* scale `scale`'s seeds (NULL = skip): cube [nseed][nscan], the scale model's own lnprob [nseed], prior sum lp [nseed] (-inf outside the
 * box), composition fr [nseed][3], status [nseed] */
int gf_toys_get_seeds(gf_toys* t, int scale, double* cube, double* lnprob, double* lp, double* fr, int32_t* status);
/* The starts of every (scale, realisation).  bf [ntoys][3] shared by the scales (per_scale == 0) or [nscales][ntoys][3]; smearing
 * [ntoys].  Out (NULL = skip): cube [nscales][ntoys][K][nscan] the selected seeds' cube points (NaN behind the count), index and score
 * [nscales][ntoys][K] (-1 and -inf behind the count), count [nscales][ntoys].  The seeds stay on the device; synchronous. */
int gf_toys_select(gf_toys* t, const double* bf, int per_scale, const double* smearing, int ntoys, int K, double* cube, int32_t* index,
                   double* score, int32_t* count);
/* every score the selection ranks, scores [nscales][ntoys][nseed] (ntoys <= 65535): for tests and estimators of the caller's own */
int gf_toys_scores(gf_toys* t, const double* bf, int per_scale, const double* smearing, int ntoys, double* scores);
/* The selection alone on host arrays, on `device`: lp [nseed], fr [nseed][3], status [nseed]; bf [ntoys][3], smearing [ntoys], one
 * offset; out_index and out_score [ntoys][K], out_count [ntoys]. */
int gf_toy_select(int device, const double* lp, const double* fr, const int32_t* status, int nseed, const double* bf,
                  const double* smearing, double offset, int ntoys, int K, int32_t* out_index, double* out_score, int32_t* out_count);

/* ---- realisation ensembles of the energy-resolved likelihood (csrc/gf_toys_binned.hpp holds the arithmetic) - */
/* A realisation of a binned measurement (m_k, sigma_k), k < nbins, is m_{t,k} = m_k + sigma_k z_{t,k}, z ~ N(0, I_3) independent per bin
 * (thrown by the caller).  A seed's prior sum, verdict and composition at every energy bin do not depend on the measurement, so the seeds
 * of every scale are drawn and propagated once -- the points gf_simplex_create's seeding draws for the same seed and run id -- and
 * ranked under every realisation:
 *   score(t, i) = lp_i + (sum_k log_of_exp(fma(mh_{t,k}, |fr_{i,k} - m_{t,k}|^2, k_{t,k})) + offset), the binned lnprob's own operations
 *   in their order (the sum ascends in k); -inf for a seed the reference would have raised on and for NaN;
 *   order, starts and GF_TOY_MAX_STARTS as in 6j.
 * Models as for gf_simplex_create (one per scale), every one with a binned measurement (gf_model_set_binned_measurement; else
 * GF_ERR_UNSUPPORTED), one number of energy bins and one likelihood offset for all.  The per-bin compositions take
 * 24 * nscales * nseed * nbins bytes of device memory. */
typedef struct gf_toys_binned gf_toys_binned;
int gf_toys_create_binned(gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed, uint64_t seed,
                          gf_toys_binned** out);
void gf_toys_destroy_binned(gf_toys_binned* t);
/* run ids [nscales] (default: the index).  Before gf_toys_seed_binned. */
int gf_toys_set_run_ids_binned(gf_toys_binned* t, const uint64_t* ids);
/* Draws and evaluates the seeds, once.  nonunitary [nscales] (NULL = skip).  Synchronous. */
int gf_toys_seed_binned(gf_toys_binned* t, uint32_t* nonunitary);
/* scale `scale`'s seeds (NULL = skip): as gf_toys_get_seeds (lnprob: the scale model's own, under its binned measurement; fr: the
 * flux-averaged composition), and fr_bins [nseed][nbins][3], NaN for a seed whose status is not GF_ST_OK */
int gf_toys_get_seeds_binned(gf_toys_binned* t, int scale, double* cube, double* lnprob, double* lp, double* fr, double* fr_bins, int32_t* status);
/* The starts of every (scale, realisation).  meas [ntoys][nbins][3] shared by the scales (per_scale == 0) or [nscales][ntoys][nbins][3];
 * sigma [nbins] shared by the realisations (per_toy_sigma == 0) or [ntoys][nbins].  Out as gf_toys_select. */
int gf_toys_select_binned(gf_toys_binned* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, int K,
                          double* cube, int32_t* index, double* score, int32_t* count);
/* every score the selection ranks, scores [nscales][ntoys][nseed] (ntoys <= 65535) */
int gf_toys_scores_binned(gf_toys_binned* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, double* scores);
/* The selection alone on host arrays, on `device`: lp [nseed], fr_bins [nseed][nbins][3], status [nseed]; meas [ntoys][nbins][3], sigma
 * [nbins] or [ntoys][nbins], one offset; out_index and out_score [ntoys][K], out_count [ntoys]. */
int gf_toy_select_binned(int device, const double* lp, const double* fr_bins, const int32_t* status, int nseed, int nbins, const double* meas,
                         const double* sigma, int per_toy_sigma, double offset, int ntoys, int K, int32_t* out_index, double* out_score,
                         int32_t* out_count);
/* A binned measurement of its own for every run of a maximiser over models with a binned measurement: fr_bins [nruns][nbins][3] and sigma
 * [nruns][nbins] become the table run r's kernels read in place of its model's, built as gf_model_set_binned_measurement builds it, so
 * the run evaluates exactly what a model given (fr_bins_r, sigma_r) evaluates.  Before the first gf_simplex_run; may be called again
 * before it.  Refused: models without a binned measurement (GF_ERR_UNSUPPORTED), a maximiser created with nseed > 0, another nbins than
 * the models', a composition that is not finite, a width that is not positive and finite or whose constants are not finite. */
int gf_toys_set_binned_measurements(gf_simplex* s, int nbins, const double* fr_bins, const double* sigma);

#ifdef __cplusplus
}
#endif
#endif /* GOLEMFLAVOR_HIP_H */
