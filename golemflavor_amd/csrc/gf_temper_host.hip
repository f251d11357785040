// gf_temper_host.hip -- the host side of the tempered ensemble sampler, and only here: GfTempered, which a gf_sampler
// (gf_sampler_host.h) holds as an opaque pointer, the replica-exchange round and the run that puts one between the grid shape's steps,
// what gf_sampler_host.hip asks of a tempered sampler (gf_temper.h), the C ABI of the tempered sampler and the bulk entry point
// gf_model_lnprior_lnl[_device].  The kernels and their launchers are gf_temper.hip's.  No kernel here.
#include <new>

#include "gf_sampler_host.h"
#include "gf_temper.h"
#include "gf_temper.hpp"                // MAX_TEMPS, SERIES

// A tempered sampler: chain g * ntemps + t samples prior * L^betas[t] of group g's model.  Its model set has one entry per
// chain (group g's model ntemps times), so everything that takes one model per chain -- the settle kernel, the chain view -- is the
// multi-model sampler's.
struct GfTempered {
    int ngroups = 0, ntemps = 0, swap_every = 0;
    std::vector<double> betas;          // [ntemps]
    double* d_betas = nullptr;          // [nchains]: the chain's beta
    double* d_lp = nullptr;             // [nchains][nwalkers]: lnprior and lnl of the current walkers, as the last split evaluation left them
    double* d_lnl = nullptr;
    int32_t* d_status = nullptr;
    GfArbQueue* d_pq = nullptr;         // the split evaluation's parked rows (capacity: every walker), apart from the half-step's
    double* d_pend_rows = nullptr;
    unsigned int* d_pend_ctl = nullptr;
    uint32_t* d_counts = nullptr;       // [nchains][2]: pairs (t, t + 1) proposed / accepted since creation
};

namespace {
// a BSM model: what every entry point here says to any other mode
int mode_refusal(gf_model* m, const char* who, int index)
{
    const GfCommon* c; const GfBsm* tb; const double* ptab; int device, cus, nbins;
    if (!m || gf_model_constants(m, &c, &tb, &ptab, &device, &cus, &nbins) != GF_OK) return GF_ERR_INVALID_ARG;
    if (c->mode != GF_MODE_BSM_GAUSS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: model %d has mode %d; lnprior and lnL are taken apart for the flux-averaged BSM likelihood only", who, index, c->mode);
    return GF_OK;
}

// the flux-averaged BSM likelihood only: what gf_sampler_create_tempered says to any other model (the energy-resolved and the tabulated
// likelihood have entry points of their own, as the untempered sampler's)
int model_refusal(gf_model* m, const char* who, int index)
{
    if (const int rc = mode_refusal(m, who, index)) return rc;
    if (gf_model_table(m, nullptr) > 0)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: model %d carries a tabulated likelihood; the flux-averaged BSM likelihood only", who, index);
    if (gf_model_binned(m, nullptr))
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: model %d carries a binned measurement; the flux-averaged BSM likelihood only", who, index);
    return GF_OK;
}

// lnprior, lnl and status of the current walkers of every chain in one launch (k_lnprior_lnl and the exact verdict behind it); T (may
// be null) <- the walkers' scalar at their chain's beta, NaN where the reference would have raised
hipError_t tempered_split(gf_sampler* s, double* T)
{
    GfTempered* tp = s->tp;
    GfSplitArgs a = {};
    a.commons = s->set.d_commons; a.tbs = s->set.d_tbs; a.ptabs = s->set.d_ptabs;
    a.theta = s->d_pos; a.lp = tp->d_lp; a.lnl = tp->d_lnl; a.status = tp->d_status;
    a.pq = tp->d_pq; a.pend_rows = tp->d_pend_rows;
    a.rows = s->nwalkers; a.ndim = s->ndim; a.nbins_max = s->set.nbins_max;
    a.betas = tp->d_betas; a.T = T;
    a.btabs = s->set.d_btabs; a.ttabs = s->set.d_ttabs; a.tsides = s->set.d_tsides;       // the instance of the sampler's kind
    return gf_launch_lnprior_lnl(a, s->nchains, tp->d_pend_ctl, s->d_state, s->set.cus, s->set.stream);
}

// replica-exchange round `round`, eagerly on the sampler's stream: (lp, lnl) of every current walker again -- one step's evaluations --
// then k_pt_swap
hipError_t tempered_round(gf_sampler* s, uint64_t round)
{
    GfTempered* tp = s->tp;
    hipError_t e = tempered_split(s, nullptr);
    if (e != hipSuccess) return e;
    GfSwapArgs w = {};
    w.pos = s->d_pos; w.T = s->d_lnp; w.lp = tp->d_lp; w.lnl = tp->d_lnl; w.betas = tp->d_betas; w.stream_ids = s->d_stream_ids;
    w.counts = tp->d_counts; w.seed = s->seed; w.round = round;
    w.ngroups = tp->ngroups; w.ntemps = tp->ntemps; w.nwalkers = s->nwalkers; w.ndim = s->ndim;
    return gf_launch_pt_swap(w, s->set.stream);
}
}  // namespace

int gf_temper_start(gf_sampler* s)
{
    // every chain's walkers in one split evaluation, T at the chain's beta, then k_fix_start as for every BSM sampler
    hipStream_t st = s->set.stream;
    // a table sampler: the models' tables of now, as at the start of a run (the upload of the positions is all the stream holds)
    GF_HIP(hipStreamSynchronize(st));
    if (const int rc = gf_modelset_refresh_tables(&s->set, "gf_sampler_set_state")) return rc;
    hipError_t e = tempered_split(s, s->d_lnp);
    if (e == hipSuccess) e = gf_launch_fix_start(s->tp->d_status, (int64_t)s->nchains * s->nwalkers, s->d_lnp, s->d_flags, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_set_state");
    return gf_internal_check_overflow(s->set.device, st);
}

hipError_t gf_temper_clear_counts(gf_sampler* s)
{
    return hipMemsetAsync(s->tp->d_counts, 0, sizeof(uint32_t) * 2 * (size_t)s->nchains, s->set.stream);
}

// The steps between two rounds are the grid shape's loop (run_grid: graph replays and eager blocks), a round's launches eagerly behind
// the step whose stored sample it follows: the captured graph stays the serial chain of GRAPH_STEPS steps it is for every grid-shape
// sampler, and knows nothing of rounds.
int gf_temper_run(Run& r, GridSteps& g)
{
    gf_sampler* s = r.s;
    const GfTempered* tp = s->tp;
    g.betas = tp->d_betas;
    grid_begin(r, g);
    while (r.done < r.nsteps) {
        const uint64_t i0 = s->iteration + (uint64_t)r.done;            // the next step, counted since creation
        int64_t seg = r.nsteps - r.done;
        bool round = false;
        if (tp->swap_every > 0) {
            const int64_t until = tp->swap_every - (int64_t)(i0 % (uint64_t)tp->swap_every);     // steps up to and including the round's
            if (until <= seg) { seg = until; round = true; }
        }
        const int rc = run_grid(r, g, r.done + seg);
        if (rc != GF_OK) return rc;
        if (round) {
            const hipError_t e = tempered_round(s, (i0 + (uint64_t)seg) / (uint64_t)tp->swap_every - 1);
            if (e != hipSuccess) return gf_hip_fail(e, "replica-exchange round");
        }
    }
    return GF_OK;
}

void gf_temper_free(GfTempered* tp)
{
    if (!tp) return;
    void* ptrs[] = {tp->d_betas, tp->d_lp, tp->d_lnl, tp->d_status, tp->d_pq, tp->d_pend_rows, tp->d_pend_ctl, tp->d_counts};
    for (void* p : ptrs) if (p) (void)gf_cached_free(p);
    delete tp;
}

namespace {
// A tempered sampler (the header has the contract).  The model set holds group g's model once per rung, so the sampler is
// a multi-model one whose chain g * ntemps + t also has a beta.  want: the likelihood every model carries, as sampler_create's -- the
// flux-averaged entry point words its own refusal of the other two, the entry points of those leave it to sampler_create.
int create_tempered(const char* who, int want, gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers,
                    uint64_t seed, double a, int swap_every, gf_sampler** out)
{
    if (!models || !betas || !out) return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_internal_set_error("");
    if (ngroups < 1 || ntemps < 1 || swap_every < 0 || (int64_t)ngroups * ntemps > 65535)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d groups of %d rungs, a round every %d steps: at least one of each, no negative period, at most 65535 chains", who, ngroups, ntemps, swap_every);
    if (ntemps > gftp::MAX_TEMPS) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d rungs; a ladder has at most %d", who, ntemps, gftp::MAX_TEMPS);
    if (nmodels != 1 && nmodels != ngroups)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d models for %d groups; one for all groups, or one per group", who, nmodels, ngroups);
    if (!(betas[0] == 1.0)) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: betas[0] is %g; the first rung is the posterior itself, beta = 1", who, betas[0]);
    for (int t = 1; t < ntemps; ++t)
        if (!(betas[t] < betas[t - 1])) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: betas[%d] = %g does not lie below betas[%d] = %g; a ladder is strictly decreasing", who, t, betas[t], t - 1, betas[t - 1]);
    if (!(betas[ntemps - 1] >= 0.0)) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the last rung's beta is %g; it is >= 0", who, betas[ntemps - 1]);
    for (int g = 0; g < nmodels; ++g) {
        if (!models[g]) return GF_ERR_INVALID_ARG;
        if (const int rc = want == GF_LLH_FLUX ? model_refusal(models[g], who, g) : mode_refusal(models[g], who, g)) return rc;
        // gf_sampler_create_binned's / _table's refusal, naming the group's model (the model set numbers the chains')
        if (want != GF_LLH_FLUX) {
            const int has = gf_model_table(models[g], nullptr) > 0 ? GF_LLH_TABLE : gf_model_binned(models[g], nullptr) ? GF_LLH_BINNED : GF_LLH_FLUX;
            if (const int rc = sampler_likelihood_refusal(want, has, g)) return rc;
        }
    }
    const int nchains = ngroups * ntemps;
    std::vector<gf_model*> per_chain((size_t)nchains);
    std::vector<double> chain_beta((size_t)nchains);
    for (int ch = 0; ch < nchains; ++ch) { per_chain[ch] = models[nmodels == 1 ? 0 : ch / ntemps]; chain_beta[ch] = betas[ch % ntemps]; }
    gf_sampler* s = nullptr;
    int rc = sampler_create(per_chain.data(), true, nchains, nwalkers, seed, a, &s, want);
    if (rc != GF_OK) return rc;
    GfTempered* tp = new (std::nothrow) GfTempered();
    if (!tp) { gf_sampler_destroy(s); return GF_ERR_ALLOC; }
    s->tp = tp;                                                     // (one launch shape, the per-half-step grid kernels: run_shape)
    tp->ngroups = ngroups; tp->ntemps = ntemps; tp->swap_every = swap_every;
    tp->betas.assign(betas, betas + ntemps);
    const size_t nw = (size_t)nchains * nwalkers;
    hipStream_t st = s->set.stream;
    hipError_t e = gf_cached_malloc((void**)&tp->d_betas, sizeof(double) * (size_t)nchains);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&tp->d_lp, sizeof(double) * nw);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&tp->d_lnl, sizeof(double) * nw);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&tp->d_status, sizeof(int32_t) * nw);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&tp->d_counts, sizeof(uint32_t) * 2 * (size_t)nchains);
    if (e == hipSuccess) e = gf_alloc_arb_queue(GF_MEM_CACHED, nw, st, &tp->d_pq, &tp->d_pend_rows, &tp->d_pend_ctl);
    if (e == hipSuccess) e = hipMemcpyAsync(tp->d_betas, chain_beta.data(), sizeof(double) * (size_t)nchains, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(tp->d_counts, 0, sizeof(uint32_t) * 2 * (size_t)nchains, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);              // chain_beta goes out of scope
    if (e != hipSuccess) { gf_sampler_destroy(s); return gf_hip_fail(e, who); }
    *out = s;
    return GF_OK;
}
}  // namespace

extern "C" {

int gf_sampler_create_tempered(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers, uint64_t seed,
                               double a, int swap_every, gf_sampler** out)
{
    return create_tempered("gf_sampler_create_tempered", GF_LLH_FLUX, models, nmodels, ngroups, ntemps, betas, nwalkers, seed, a, swap_every, out);
}

// the tempered sampler of the energy-resolved likelihood: every model carries a binned measurement, as gf_sampler_create_binned's
int gf_sampler_create_tempered_binned(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers,
                                      uint64_t seed, double a, int swap_every, gf_sampler** out)
{
    return create_tempered("gf_sampler_create_tempered_binned", GF_LLH_BINNED, models, nmodels, ngroups, ntemps, betas, nwalkers, seed, a, swap_every, out);
}

// the tempered sampler of the tabulated flavour-plane likelihood: every model carries a table, as gf_sampler_create_table's;
// the set's tables are taken again at the start of every run, every gf_sampler_set_state and every gf_sampler_tempered_series
int gf_sampler_create_tempered_table(gf_model* const* models, int nmodels, int ngroups, int ntemps, const double* betas, int nwalkers,
                                     uint64_t seed, double a, int swap_every, gf_sampler** out)
{
    return create_tempered("gf_sampler_create_tempered_table", GF_LLH_TABLE, models, nmodels, ngroups, ntemps, betas, nwalkers, seed, a, swap_every, out);
}

int gf_sampler_betas(const gf_sampler* s, int* ngroups, int* ntemps, double* betas, int* swap_every)
{
    if (!s) return GF_ERR_INVALID_ARG;
    if (!s->tp) return GF_ERR_UNSUPPORTED;
    if (ngroups) *ngroups = s->tp->ngroups;
    if (ntemps) *ntemps = s->tp->ntemps;
    if (swap_every) *swap_every = s->tp->swap_every;
    if (betas) for (int t = 0; t < s->tp->ntemps; ++t) betas[t] = s->tp->betas[t];
    return GF_OK;
}

int gf_sampler_swap_counts(gf_sampler* s, uint32_t* proposed, uint32_t* accepted)
{
    if (!s) return GF_ERR_INVALID_ARG;
    if (!s->tp) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(s->set.device));
    std::vector<uint32_t> h(2 * (size_t)s->nchains);
    GF_HIP(hipMemcpyAsync(h.data(), s->tp->d_counts, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost, s->set.stream));
    GF_HIP(hipStreamSynchronize(s->set.stream));
    for (int ch = 0; ch < s->nchains; ++ch) {
        if (proposed) proposed[ch] = h[2 * (size_t)ch];
        if (accepted) accepted[ch] = h[2 * (size_t)ch + 1];
    }
    return GF_OK;
}

// series [nchains][nstored][5], lnl_chain (host) / d_lnl_chain (device) [nchains][nstored][nwalkers], either may be NULL
int gf_sampler_tempered_series(gf_sampler* s, const double* d_up, const double* d_dn, double* series, double* lnl_chain, double* d_lnl_chain)
{
    if (!s || !d_up || !d_dn || !series) return GF_ERR_INVALID_ARG;
    if (!s->tp) return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_sampler_tempered_series: the sampler is not a tempered one (gf_sampler_create_tempered)");
    if (const int rc = sampler_kind_refusal(s, "gf_sampler_tempered_series")) return rc;
    for (int ch = 0; ch < s->nchains; ++ch)
        if (!(d_up[ch] >= 0.0) || !(d_dn[ch] >= 0.0) || !std::isfinite(d_up[ch]) || !std::isfinite(d_dn[ch]))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_sampler_tempered_series: the exponents of chain %d are %g and %g; finite and >= 0", ch, d_up[ch], d_dn[ch]);
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    GF_HIP(hipStreamSynchronize(st));
    if (s->nstored == 0) return GF_OK;
    if (const int rc = gf_modelset_refresh_tables(&s->set, "gf_sampler_tempered_series")) return rc;      // a table sampler: the models' tables of now
    const size_t nch = (size_t)s->nchains, ns = (size_t)s->nstored;
    GfScratch sc(GF_MEM_CACHED);
    double *dd_up = nullptr, *dd_dn = nullptr, *d_out = nullptr, *d_lnl = d_lnl_chain;
    (void)sc.take(&dd_up, sizeof(double) * nch, "gf_sampler_tempered_series");
    (void)sc.take(&dd_dn, sizeof(double) * nch, "gf_sampler_tempered_series");
    if (!d_lnl) (void)sc.take(&d_lnl, sizeof(double) * nch * ns * (size_t)s->nwalkers, "gf_sampler_tempered_series");
    if (const int ra = sc.take(&d_out, sizeof(double) * nch * ns * gftp::SERIES, "gf_sampler_tempered_series")) return ra;
    GF_HIP(hipMemcpyAsync(dd_up, d_up, sizeof(double) * nch, hipMemcpyHostToDevice, st));
    GF_HIP(hipMemcpyAsync(dd_dn, d_dn, sizeof(double) * nch, hipMemcpyHostToDevice, st));
    GfSeriesArgs a = {};
    a.commons = s->set.d_commons; a.tbs = s->set.d_tbs; a.ptabs = s->set.d_ptabs;
    a.chain = s->d_chain; a.lnp_chain = s->d_lnp_chain; a.cap = s->nstore_cap; a.nstored = s->nstored;
    a.nwalkers = s->nwalkers; a.ndim = s->ndim; a.d_up = dd_up; a.d_dn = dd_dn; a.lnl = d_lnl; a.out = d_out;
    a.btabs = s->set.d_btabs; a.ttabs = s->set.d_ttabs; a.tsides = s->set.d_tsides;
    hipError_t e = gf_launch_pt_series(a, s->nchains, st);
    if (e == hipSuccess) e = hipMemcpyAsync(series, d_out, sizeof(double) * nch * ns * gftp::SERIES, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && lnl_chain) e = hipMemcpyAsync(lnl_chain, d_lnl, sizeof(double) * nch * ns * (size_t)s->nwalkers, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_tempered_series");
    return GF_OK;
}

// d_theta [n][ndim] (AoS) -> d_lp, d_lnl [n], d_status [n], all on the device; synchronous on return
int gf_model_lnprior_lnl_device(gf_model* m, const double* d_theta, int64_t n, double* d_lp, double* d_lnl, int32_t* d_status)
{
    if (!m || n < 0 || (n > 0 && (!d_theta || !d_lp || !d_lnl || !d_status))) return GF_ERR_INVALID_ARG;
    gf_internal_set_error("");
    if (const int rc = mode_refusal(m, "gf_model_lnprior_lnl", 0)) return rc;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device, cus, nbins;
    int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc == GF_OK) rc = gf_model_constants(m, &c, &tb, &ptab, &device, &cus, &nbins);
    if (rc != GF_OK) return rc;
    if (n == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    constexpr int64_t PIECE = 1 << 18;                       // rows per launch: bounds the parked rows' buffers
    const int64_t piece = n < PIECE ? n : PIECE;
    // the likelihood the model carries now, as gf_lnprob_batch evaluates it: a table, a binned measurement, or neither
    const double* ltab = nullptr; const double* bmeas = nullptr;
    const int32_t tside = gf_model_table(m, &ltab);
    const bool binned = tside <= 0 && gf_model_binned(m, &bmeas);
    if (binned) ltab = bmeas;
    // one model: the kernels' per-model arrays have one entry each
    GfScratch sc(GF_MEM_CACHED);
    GfCommon* d_common = nullptr; const GfBsm** d_tbs = nullptr; const double** d_ptabs = nullptr; GfStepState* d_state = nullptr;
    const double** d_ltab = nullptr; int32_t* d_tside = nullptr;
    (void)sc.take(&d_ltab, sizeof(void*), "gf_model_lnprior_lnl");
    (void)sc.take(&d_tside, sizeof(int32_t), "gf_model_lnprior_lnl");
    (void)sc.take(&d_common, sizeof(GfCommon), "gf_model_lnprior_lnl");
    (void)sc.take(&d_tbs, sizeof(void*), "gf_model_lnprior_lnl");
    (void)sc.take(&d_ptabs, sizeof(void*), "gf_model_lnprior_lnl");
    if (const int ra = sc.take(&d_state, sizeof(GfStepState), "gf_model_lnprior_lnl")) return ra;
    GfArbQueue* pq = nullptr; double* pend = nullptr; unsigned int* ctl = nullptr;
    hipError_t e = gf_alloc_arb_queue(GF_MEM_CACHED, (size_t)piece, st, &pq, &pend, &ctl);
    if (e == hipSuccess) e = hipMemcpyAsync(d_common, c, sizeof(GfCommon), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync((void*)d_tbs, &tb, sizeof(void*), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync((void*)d_ptabs, &ptab, sizeof(void*), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync((void*)d_ltab, &ltab, sizeof(void*), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tside, &tside, sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_state, 0, sizeof(GfStepState), st);
    for (int64_t w0 = 0; w0 < n && e == hipSuccess; w0 += piece) {
        GfSplitArgs a = {};
        a.commons = d_common; a.tbs = d_tbs; a.ptabs = d_ptabs;
        a.theta = d_theta + w0 * c->ndim; a.lp = d_lp + w0; a.lnl = d_lnl + w0; a.status = d_status + w0;
        a.pq = pq; a.pend_rows = pend; a.rows = (int32_t)(n - w0 < piece ? n - w0 : piece); a.ndim = c->ndim; a.nbins_max = nbins;
        if (tside > 0) { a.ttabs = d_ltab; a.tsides = d_tside; }
        else if (binned) a.btabs = d_ltab;
        e = gf_launch_lnprior_lnl(a, 1, ctl, d_state, cus, st);
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    for (void* p : {(void*)pq, (void*)pend, (void*)ctl}) if (p) (void)gf_cached_free(p);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_model_lnprior_lnl");
    return GF_OK;
}

// theta [n][ndim] -> lp, lnl [n], status [n] on the host
int gf_model_lnprior_lnl(gf_model* m, const double* theta, int64_t n, double* lp, double* lnl, int32_t* status)
{
    if (!m || n < 0 || (n > 0 && (!theta || !lp || !lnl || !status))) return GF_ERR_INVALID_ARG;
    gf_internal_set_error("");
    if (const int rc = mode_refusal(m, "gf_model_lnprior_lnl", 0)) return rc;
    if (n == 0) return GF_OK;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    const int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    GfScratch sc(GF_MEM_CACHED);
    double *d_theta = nullptr, *d_lp = nullptr, *d_lnl = nullptr; int32_t* d_status = nullptr;
    (void)sc.take(&d_theta, sizeof(double) * (size_t)n * c->ndim, "gf_model_lnprior_lnl");
    (void)sc.take(&d_lp, sizeof(double) * (size_t)n, "gf_model_lnprior_lnl");
    (void)sc.take(&d_lnl, sizeof(double) * (size_t)n, "gf_model_lnprior_lnl");
    if (const int ra = sc.take(&d_status, sizeof(int32_t) * (size_t)n, "gf_model_lnprior_lnl")) return ra;
    GF_HIP(hipMemcpyAsync(d_theta, theta, sizeof(double) * (size_t)n * c->ndim, hipMemcpyHostToDevice, st));
    GF_HIP(hipStreamSynchronize(st));
    const int re = gf_model_lnprior_lnl_device(m, d_theta, n, d_lp, d_lnl, d_status);
    if (re != GF_OK) return re;
    GF_HIP(hipMemcpyAsync(lp, d_lp, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    GF_HIP(hipMemcpyAsync(lnl, d_lnl, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    GF_HIP(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

}  // extern "C"
