// gf_postprocess.hip -- a sampler's STORED chain turned into what the scripts save: compositions, flavor histograms, the scan's rows,
// credible regions, marginals and convergence diagnostics.  Host code only; the sampler is seen through a GfChainView (gf_internal.h), and every entry point
// works in order on the sampler's stream, the one the chain was written on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_devcache.h"                // the scratch buffers of a scan's post-processing are the multi-gigabyte allocations the cache exists for
#include "gf_host.h"                    // (after gf_devcache.h: GfScratch allocates through the cache)
#include "gf_region.h"
#include "gf_marginal.h"
#include "gf_elements.h"
#include "gf_diag.h"
#include "gf_interval.h"
#include "gf_spectrum.h"

namespace {

// the model chain ch is post-processed with: models[ch] if the caller gives models, else the posterior the chain samples
gf_model* chain_model(const GfChainView& v, gf_model* const* models, int ch) { return models ? models[ch] : v.models ? v.models[ch] : v.model; }

// every chain's model must have the sampler's ndim and device.  *cus (may be NULL): the CUs the last chain's model sizes its grids for
int check_chain_models(const GfChainView& v, gf_model* const* models, int* cus = nullptr)
{
    for (int ch = 0; ch < v.nchains; ++ch) {
        const GfCommon* c; const GfBsm* tb; const double* ptab; int device, mcus, nbins;
        if (gf_model_constants(chain_model(v, models, ch), &c, &tb, &ptab, &device, &mcus, &nbins) != GF_OK || c->ndim != v.ndim || device != v.device)
            return GF_ERR_INVALID_ARG;
        if (cus) *cus = mcus;
    }
    return GF_OK;
}

const double* chain_theta(const GfChainView& v, int ch) { return v.d_chain + (size_t)ch * v.nstore_cap * v.nwalkers * v.ndim; }
inline hipError_t first_error(hipError_t a, hipError_t b) { return a != hipSuccess ? a : b; }

// for every chain: propagate it with its model on v.stream, then *e = after(ch, d_theta, d_fr_ch, d_st_ch); stops at the first failure
// of either (returns the propagation's code); nothing for an empty chain.  per_chain_scratch: chain ch has its own part of d_fr [.][3]
// and d_st (may be NULL), else all go through the same one.  full_grids: the chains are enqueued faster than they run, so the arbitration
// grid of each would follow what some EARLIER chain found, and the chains of a scan differ (its high-scale grid points sit in the failing
// region, the others have empty queues): full grids throughout, ~30 us per chain (measured: the hint left 57 of 64 chains of the C4 scan
// on a sixth of the GPU, 114 ms of arbitration instead of ~20)
template <class After>
int for_each_chain(const GfChainView& v, gf_model* const* models, double* d_fr, int32_t* d_st, bool per_chain_scratch, bool full_grids,
                   hipError_t* e, After after)
{
    const int64_t per_chain = v.nstored * v.nwalkers;
    int rc = GF_OK;
    if (full_grids) gf_internal_full_arbitration_grids(v.device, v.stream, 1);
    for (int ch = 0; ch < v.nchains && rc == GF_OK && *e == hipSuccess && per_chain > 0; ++ch) {
        const size_t at = per_chain_scratch ? (size_t)ch * per_chain : 0;
        rc = gf_model_propagate_on(chain_model(v, models, ch), v.stream, chain_theta(v, ch), GF_LAYOUT_AOS, per_chain, d_fr + at * 3, d_st ? d_st + at : nullptr);
        if (rc == GF_OK) *e = after(ch, chain_theta(v, ch), d_fr + at * 3, d_st ? d_st + at : nullptr);
    }
    if (full_grids) gf_internal_full_arbitration_grids(v.device, v.stream, 0);
    return rc;
}

}  // namespace

extern "C" {

// Chain post-processing on the device (scripts/mc_unitary.py:189-193, mc_texture.py:216-221, and the
// histogram of golemflavor/plot.py:365-370): measured composition of every stored sample, optionally
// reduced to the [nbins]^3 flavor histogram so that only the counts cross PCIe.
//   fr      [nchains][nstored][nwalkers][3]  or NULL
//   status  [nchains][nstored][nwalkers]     or NULL
//   counts  [nchains][nbins][nbins][nbins]   or NULL (nbins ignored then)
int gf_sampler_postprocess(gf_sampler* s, double* fr, int32_t* status, int nbins, uint64_t* counts)
{
    return gf_sampler_postprocess_with(s, nullptr, fr, status, nbins, counts);
}

// Same, but chain ch is propagated with models[ch] instead of the posterior it was sampled from
// (scripts/mc_texture.py: the chain samples the priors, mc_texture.py:148-170, and every sample is then pushed
// through flux_averaged_BSMu at the grid point's scale and source, mc_texture.py:216-221).  models == NULL:
// the sampling models.  Each model must have the sampler's ndim and device.
int gf_sampler_postprocess_with(gf_sampler* s, gf_model* const* models, double* fr, int32_t* status, int nbins, uint64_t* counts)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || (counts && (nbins < 1 || nbins > 1024))) return GF_ERR_INVALID_ARG;
    int cus = 256;
    if (check_chain_models(v, models, &cus) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GF_HIP(hipStreamSynchronize(st));
    if (v.nstored == 0) return GF_OK;
    const int64_t per_chain = v.nstored * v.nwalkers;
    const size_t nbin3 = counts ? (size_t)nbins * nbins * nbins : 0;
    GfScratch buf;
    double* d_fr = nullptr; int32_t* d_st = nullptr; uint64_t* d_c = nullptr;
    hipError_t e = buf.get(&d_fr, sizeof(double) * 3 * per_chain);
    if (e == hipSuccess && status) e = buf.get(&d_st, sizeof(int32_t) * per_chain);
    if (e == hipSuccess && counts) e = buf.get(&d_c, sizeof(uint64_t) * nbin3);
    // propagate, histogram, copies back; the scratch buffers are reused chain after chain, one sync at the end.
    // Not under full arbitration grids, alone among the entry points: inherited, not decided (it sizes grids, so it is a speed question)
    const int rc = for_each_chain(v, models, d_fr, d_st, false, false, &e, [&](int ch, const double*, double*, int32_t*) {
        hipError_t ea = hipSuccess;
        if (counts) {
            ea = hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nbin3, st);
            if (ea == hipSuccess) ea = gf_launch_flavor_hist(d_fr, per_chain, nbins, (unsigned long long*)d_c, cus, st);
        }
        if (ea == hipSuccess && fr) ea = hipMemcpyAsync(fr + (size_t)ch * per_chain * 3, d_fr, sizeof(double) * 3 * per_chain, hipMemcpyDeviceToHost, st);
        if (ea == hipSuccess && status) ea = hipMemcpyAsync(status + (size_t)ch * per_chain, d_st, sizeof(int32_t) * per_chain, hipMemcpyDeviceToHost, st);
        if (ea == hipSuccess && counts) ea = hipMemcpyAsync(counts + (size_t)ch * nbin3, d_c, sizeof(uint64_t) * nbin3, hipMemcpyDeviceToHost, st);
        return ea;
    });
    e = first_error(e, hipStreamSynchronize(st));
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_postprocess");
    return status ? gf_internal_check_overflow(v.device, st) : GF_OK;
}

// Same with DEVICE destinations: d_fr [nchains][nstored][nwalkers][3], d_status [nchains][nstored][nwalkers] (NULL = skip);
// synchronous on return.
int gf_sampler_postprocess_device(gf_sampler* s, gf_model* const* models, double* d_fr, int32_t* d_status)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !d_fr) return GF_ERR_INVALID_ARG;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipError_t e = hipSuccess;
    int rc = for_each_chain(v, models, d_fr, d_status, true, true, &e, [](int, const double*, double*, int32_t*) { return hipSuccess; });
    GF_HIP(hipStreamSynchronize(v.stream));
    if (rc == GF_OK && d_status) rc = gf_internal_check_overflow(v.device, v.stream);
    return rc;
}

// The scan's output rows on the device: d_rows [nchains][nstored][nwalkers][3 + ndim] = composition (NaN where the
// reference would have raised) then the sample, each chain propagated with models[ch] (NULL: the sampling models).
// All propagations first (gf_sampler_postprocess_device), then all joins.  Synchronous on return.  scripts/mc_texture.py:216-223.
int gf_sampler_postprocess_rows_device(gf_sampler* s, gf_model* const* models, double* d_rows)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !d_rows) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    const int64_t per_chain = v.nstored * v.nwalkers;
    if (per_chain == 0) { GF_HIP(hipStreamSynchronize(st)); return GF_OK; }
    GfScratch buf;
    double* d_fr = nullptr; int32_t* d_st = nullptr;
    GF_HIP(buf.get(&d_fr, sizeof(double) * 3 * per_chain * v.nchains));
    GF_HIP(buf.get(&d_st, sizeof(int32_t) * per_chain * v.nchains));
    const int rc = gf_sampler_postprocess_device(s, models, d_fr, d_st);
    hipError_t e = hipSuccess;
    for (int ch = 0; ch < v.nchains && rc == GF_OK && e == hipSuccess; ++ch)
        e = gf_launch_join_rows(d_fr + (size_t)ch * per_chain * 3, d_st + (size_t)ch * per_chain, chain_theta(v, ch), v.ndim, per_chain,
                                d_rows + (size_t)ch * per_chain * (3 + v.ndim), v.cus, st);
    e = first_error(e, hipStreamSynchronize(st));
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_postprocess_rows_device");
    return GF_OK;
}

// The scan's rows straight to the host.  The chains are post-processed in turn on the sampler's stream (everything is enqueued
// at once); an event marks the end of every group of chains, and one pinned-ring copy on a SECOND stream follows the events
// chunk by chunk -- so the read-back of finished groups overlaps the evaluation (and the x87 arbitration, which dominates a
// texture scan's post-processing) of the later ones.
int gf_sampler_postprocess_rows(gf_sampler* s, gf_model* const* models, double* rows)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !rows) return GF_ERR_INVALID_ARG;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    const int64_t per_chain = v.nstored * v.nwalkers;
    if (per_chain == 0) { GF_HIP(hipStreamSynchronize(st)); return GF_OK; }
    const size_t width = 3 + (size_t)v.ndim, chain_bytes = sizeof(double) * width * (size_t)per_chain;
    constexpr int MAX_GROUPS = 16;
    const int per_group = (v.nchains + MAX_GROUPS - 1) / MAX_GROUPS;
    const int ngroups = (v.nchains + per_group - 1) / per_group;
    GfScratch buf;
    double *d_fr = nullptr, *d_rows = nullptr; int32_t* d_st = nullptr;
    void* copy_stream = nullptr;
    hipEvent_t ev[MAX_GROUPS] = {};
    int rc = GF_OK;
    hipError_t e = buf.get(&d_fr, sizeof(double) * 3 * per_chain * v.nchains);
    if (e == hipSuccess) e = buf.get(&d_st, sizeof(int32_t) * per_chain * v.nchains);
    if (e == hipSuccess) e = buf.get(&d_rows, chain_bytes * v.nchains);
    for (int g = 0; g < ngroups && e == hipSuccess; ++g) e = hipEventCreateWithFlags(&ev[g], hipEventDisableTiming);
    if (e == hipSuccess) rc = gf_internal_borrow_copy_stream(v.device, &copy_stream);
    if (e == hipSuccess && rc == GF_OK) {
        rc = for_each_chain(v, models, d_fr, d_st, true, true, &e, [&](int ch, const double* d_theta, double* d_fr_ch, int32_t* d_st_ch) {
            const hipError_t ea = gf_launch_join_rows(d_fr_ch, d_st_ch, d_theta, v.ndim, per_chain, d_rows + (size_t)ch * per_chain * width, v.cus, st);
            return ea == hipSuccess && ((ch + 1) % per_group == 0 || ch + 1 == v.nchains) ? hipEventRecord(ev[ch / per_group], st) : ea;
        });
        // the rows cross PCIe on the copy stream through the library's pinned ring (gf_internal_d2h_gated: the DMA fills a slot
        // while host threads empty the previous ones into `rows`, mapping its pages as they go) -- ONE pipeline over the whole
        // block, each 16 MB chunk issued as soon as the group of chains it ends in has been post-processed on the sampler's stream
        if (rc == GF_OK && e == hipSuccess) {
            struct Gate { hipEvent_t* ev; size_t group_bytes; int ngroups, passed; } gt = {ev, chain_bytes * (size_t)per_group, ngroups, 0};
            auto gate = [](void* ctx, size_t upto) -> int {
                Gate* g = static_cast<Gate*>(ctx);
                int need = (int)((upto + g->group_bytes - 1) / g->group_bytes);
                if (need > g->ngroups) need = g->ngroups;
                for (; g->passed < need; ++g->passed)
                    if (hipEventSynchronize(g->ev[g->passed]) != hipSuccess) return 1;
                return 0;
            };
            rc = gf_internal_d2h_gated(v.device, copy_stream, rows, d_rows, chain_bytes * (size_t)v.nchains, gate, &gt);
        }
    }
    e = first_error(e, hipStreamSynchronize(st));
    if (copy_stream) { (void)hipStreamSynchronize((hipStream_t)copy_stream); gf_internal_return_copy_stream(v.device, copy_stream); }
    for (int g = 0; g < ngroups; ++g) if (ev[g]) (void)hipEventDestroy(ev[g]);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_postprocess_rows");
    return gf_internal_check_overflow(v.device, st);
}

// Stored chain -> compositions -> histogram (the steps of gf_sampler_postprocess_with, one chain after the other through the same
// scratch buffers) -> credible regions of all chains at once (gf_region.hip).  The counts never leave the device.
int gf_sampler_regions(gf_sampler* s, gf_model* const* models, int nbins, int radius, const double* weights, const double* coverage,
                       int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                       int32_t* cells, double* density)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    int rc = gf_region_check_args(v.nchains, nbins, radius, weights, coverage, ncov, cap);
    if (rc != GF_OK) return rc;
    int cus = 256;
    if (check_chain_models(v, models, &cus) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    const int64_t per_chain = v.nstored * v.nwalkers;
    const size_t nbin3 = (size_t)nbins * nbins * nbins;
    GfScratch buf;
    double* d_fr = nullptr; int32_t* d_st = nullptr; uint64_t* d_c = nullptr;
    hipError_t e = buf.get(&d_c, sizeof(uint64_t) * nbin3 * v.nchains);
    if (e == hipSuccess) e = hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nbin3 * v.nchains, st);
    if (e == hipSuccess && per_chain > 0) e = buf.get(&d_fr, sizeof(double) * 3 * per_chain);
    if (e == hipSuccess && per_chain > 0) e = buf.get(&d_st, sizeof(int32_t) * per_chain);
    if (e == hipSuccess && per_chain > 0)
        rc = for_each_chain(v, models, d_fr, d_st, false, true, &e, [&](int ch, const double*, double*, int32_t*) {
            const hipError_t ea = gf_launch_mask_fr(d_fr, d_st, per_chain, st);
            return ea != hipSuccess ? ea : gf_launch_flavor_hist(d_fr, per_chain, nbins, (unsigned long long*)(d_c + (size_t)ch * nbin3), cus, st);
        });
    if (e == hipSuccess && rc == GF_OK)
        rc = gf_region_run(st, d_c, v.nchains, nbins, radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells,
                           density, nullptr);
    else
        (void)hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_regions");
    return per_chain > 0 ? gf_internal_check_overflow(v.device, st) : GF_OK;
}

// The marginals of every stored chain (gf_marginal.hip).  with_fr: the rows a scan saves are assembled first
// (gf_sampler_postprocess_rows_device) and reduced in place of the chain; either way the rows never leave the device.
int gf_sampler_marginals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !out) return GF_ERR_INVALID_ARG;
    const int width = (with_fr ? 3 : 0) + v.ndim;
    const int64_t per_chain = v.nstored * v.nwalkers;
    int rc = gf_marginal_check_args(v.nchains, per_chain, width, spec);
    if (rc != GF_OK) return rc;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    if (!with_fr || per_chain == 0) {
        GF_HIP(hipStreamSynchronize(st));
        return gf_marginal_run(st, v.d_chain, with_fr ? 0 : v.nstore_cap * v.nwalkers * v.ndim, v.nchains, per_chain, width, spec, out);
    }
    GfScratch buf;
    double* d_rows = nullptr;
    GF_HIP(buf.get(&d_rows, sizeof(double) * (size_t)per_chain * width * v.nchains));
    rc = gf_sampler_postprocess_rows_device(s, models, d_rows);
    return rc != GF_OK ? rc : gf_marginal_run(st, d_rows, per_chain * width, v.nchains, per_chain, width, spec, out);
}

// The marginals of every stored chain in element space (gf_elements.hip): the chains are transformed into a buffer of the
// library's cache, which is reduced in place of the chain; the stored chain is only read and the rows never leave the device.
int gf_sampler_element_marginals(gf_sampler* s, const gf_element_plan* plan, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !out) return GF_ERR_INVALID_ARG;
    const int width = gf_element_plan_width(plan, v.ndim);
    if (width < 0) return GF_ERR_INVALID_ARG;
    const int64_t per_chain = v.nstored * v.nwalkers;
    const int rc = gf_marginal_check_args(v.nchains, per_chain, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GfScratch buf;
    double* d_rows = nullptr;
    GF_HIP(buf.get(&d_rows, sizeof(double) * (size_t)per_chain * width * v.nchains));
    const hipError_t e = gf_element_run(st, v.d_chain, v.nstore_cap * v.nwalkers * v.ndim, v.nchains, per_chain, v.ndim, plan, d_rows,
                                        per_chain * width, v.cus);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_element_marginals");
    return gf_marginal_run(st, d_rows, per_chain * width, v.nchains, per_chain, width, spec, out);
}

// The convergence diagnostics of every stored chain (gf_diag.hip); the stored chain is only read and only the results come back.
int gf_sampler_diagnostics(gf_sampler* s, const gf_diag_spec* spec, const gf_diag_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    const int rc = gf_diag_check_args(v.nchains, v.nstored, v.nwalkers, v.ndim, spec, out);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    GF_HIP(hipStreamSynchronize(v.stream));
    return gf_diag_run(v.stream, v.d_chain, v.nstore_cap * v.nwalkers * v.ndim, v.nchains, v.nstored, v.nwalkers, v.ndim, spec, out);
}

// The column intervals of every stored chain (gf_interval.hip) over gf_sampler_marginals' rows, which never leave the device.
int gf_sampler_intervals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !spec || !out) return GF_ERR_INVALID_ARG;
    const int width = (with_fr ? 3 : 0) + v.ndim;
    const int64_t per_chain = v.nstored * v.nwalkers;
    int rc = gf_interval_check_args(v.nchains, per_chain, width, spec);
    if (rc != GF_OK) return rc;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    if (!with_fr) {
        GF_HIP(hipStreamSynchronize(st));
        return gf_interval_run(st, v.d_chain, v.nstore_cap * v.nwalkers * v.ndim, v.nchains, per_chain, width, spec, out, nullptr);
    }
    GfScratch buf;
    double* d_rows = nullptr;
    GF_HIP(buf.get(&d_rows, sizeof(double) * (size_t)per_chain * width * v.nchains));
    rc = gf_sampler_postprocess_rows_device(s, models, d_rows);
    return rc != GF_OK ? rc : gf_interval_run(st, d_rows, per_chain * width, v.nchains, per_chain, width, spec, out, nullptr);
}

// The column intervals of every stored chain in element space: gf_sampler_element_marginals' rows.
int gf_sampler_element_intervals(gf_sampler* s, const gf_element_plan* plan, const gf_interval_spec* spec, const gf_interval_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK || !spec || !out) return GF_ERR_INVALID_ARG;
    const int width = gf_element_plan_width(plan, v.ndim);
    if (width < 0) return GF_ERR_INVALID_ARG;
    const int64_t per_chain = v.nstored * v.nwalkers;
    const int rc = gf_interval_check_args(v.nchains, per_chain, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GfScratch buf;
    double* d_rows = nullptr;
    GF_HIP(buf.get(&d_rows, sizeof(double) * (size_t)per_chain * width * v.nchains));
    const hipError_t e = gf_element_run(st, v.d_chain, v.nstore_cap * v.nwalkers * v.ndim, v.nchains, per_chain, v.ndim, plan, d_rows,
                                        per_chain * width, v.cus);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_element_intervals");
    return gf_interval_run(st, d_rows, per_chain * width, v.nchains, per_chain, width, spec, out, nullptr);
}

// The energy-resolved composition of every stored chain (gf_spectrum.hip).  Chain after chain through one bin-major slab: the
// propagation leaves the verdict in d_st (its compositions go to the head of the slab and are overwritten), k_bsm_bins fills the slab,
// gf_marginal_run reduces it with the energy bins as its chains (synchronous, so the slab is free for the next chain).
int gf_sampler_spectrum(gf_sampler* s, gf_model* const* models, const gf_spectrum_spec* spec, const gf_spectrum_out* out)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    const int64_t per_chain = v.nstored * v.nwalkers;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    int nbins_e = -1;
    for (int ch = 0; ch < v.nchains; ++ch) {
        const int nb = gf_model_nbins(chain_model(v, models, ch));
        if (nb < 1) return GF_ERR_UNSUPPORTED;
        if (nbins_e >= 0 && nb != nbins_e) return gf_fail_msg(GF_ERR_INVALID_ARG, "spectrum: chain %d has %d energy bins, chain 0 has %d", ch, nb, nbins_e);
        nbins_e = nb;
    }
    int rc = gf_spectrum_check_args(nbins_e, per_chain, spec, out);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GfScratch buf;
    double* d_slab = nullptr; int32_t* d_st = nullptr;
    hipError_t e = buf.get(&d_slab, sizeof(double) * 3 * (size_t)per_chain * nbins_e);
    if (e == hipSuccess) e = buf.get(&d_st, sizeof(int32_t) * (size_t)per_chain);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_spectrum: scratch");
    int rs = GF_OK;
    rc = for_each_chain(v, models, d_slab, d_st, false, true, &e, [&](int ch, const double* d_theta, double*, int32_t*) {
        rs = gf_model_bins_on(chain_model(v, models, ch), st, d_theta, GF_LAYOUT_AOS, per_chain, d_slab, 1, d_st);
        if (rs == GF_OK) rs = gf_spectrum_reduce(st, d_slab, nbins_e, per_chain, spec, out, ch);
        return rs == GF_OK ? hipSuccess : hipErrorUnknown;
    });
    e = first_error(e, hipStreamSynchronize(st));
    if (rc != GF_OK) return rc;
    if (rs != GF_OK) return rs;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_spectrum");
    return gf_internal_check_overflow(v.device, st);
}

}  // extern "C"
