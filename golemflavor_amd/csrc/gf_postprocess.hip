// gf_postprocess.hip -- a sampler's STORED chain turned into what the scripts save: compositions, flavor histograms, the scan's rows,
// credible regions, marginals, intervals, the energy-resolved composition and convergence diagnostics.  Host code only; the sampler is
// seen through a GfChainView (gf_internal.h), and every entry point works in order on the sampler's stream, the one the chain was
// written on.  The chain is one of the three sources of gf_rowsets.h: chain_rows says where its rows are (the chain itself, or the
// rows a scan saves in scratch), the reducers, the region counts, the spectrum step and the propagate loop are that header's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_devcache.h"                // the scratch buffers of a scan's post-processing are the multi-gigabyte allocations the cache exists for
#include "gf_host.h"
#include "gf_rowsets.h"
#include "gf_diag.h"

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

// gf_propagate_sets (gf_rowsets.h) over the stored chains, chain ch with its model; nothing for an empty chain
template <class After>
int for_each_chain(const GfChainView& v, gf_model* const* models, double* d_fr, int32_t* d_st, bool per_chain_scratch, bool full_grids,
                   hipError_t* e, After after)
{
    return gf_propagate_sets(v.device, v.stream, v.nchains, v.nstored * v.nwalkers, d_fr, d_st, per_chain_scratch, full_grids, e,
                             [&](int ch, const double** th) { *th = chain_theta(v, ch); return chain_model(v, models, ch); }, after, [](int) { return hipSuccess; });
}

// the stored chain itself as row sets: no copy, nothing enqueued
GfRowSets chain_as_rows(const GfChainView& v)
{
    return GfRowSets{const_cast<double*>(v.d_chain), v.nstore_cap * v.nwalkers * v.ndim, v.nchains, v.nstored * v.nwalkers, v.ndim, v.device, v.stream, v.cus};
}

// The rows of every stored chain for a reducer.  with_fr = 0 (and an empty chain): the chain itself once the stream has drained;
// with_fr = 1: the rows a scan saves, assembled in scratch (gf_sampler_postprocess_rows_device).  They never leave the device.
int chain_rows(gf_sampler* s, const GfChainView& v, gf_model* const* models, int with_fr, GfScratch& buf, const char* who, GfRowSets* r)
{
    *r = chain_as_rows(v);
    if (!with_fr || r->n == 0) {
        GF_HIP(hipStreamSynchronize(v.stream));
        if (with_fr) { r->stride = 0; r->width = 3 + v.ndim; }
        return GF_OK;
    }
    const int rc = gf_rowsets_take(buf, *r, 3 + v.ndim, who, r);
    return rc != GF_OK ? rc : gf_sampler_postprocess_rows_device(s, models, r->d_rows);
}

// A reducer (gf_rowsets_reduce: marginals or intervals, by the spec's type) over chain_rows' rows, or (elements) over the stored chains
// pushed through `plan` into a buffer of the library's cache (gf_elements.hip: the stored chain is only read, models play no part)
template <class Spec, class Out>
int chain_reduce(gf_sampler* s, gf_model* const* models, int with_fr, bool elements, const gf_element_plan* plan, const Spec* spec, const Out* out,
                 const char* who)
{
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    const int width = elements ? gf_element_plan_width(plan, v.ndim) : (with_fr ? 3 : 0) + v.ndim;
    if (width < 0) return GF_ERR_INVALID_ARG;
    int rc = gf_rowsets_check(v.nchains, v.nstored * v.nwalkers, width, spec);
    if (rc != GF_OK) return rc;
    if (!elements && check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    GfScratch buf(GF_MEM_CACHED); GfRowSets r;
    if (!elements) rc = chain_rows(s, v, models, with_fr, buf, who, &r);
    else if ((rc = gf_rowsets_take(buf, chain_as_rows(v), width, who, &r)) == GF_OK) rc = gf_rowsets_elements(chain_as_rows(v), plan, r, who);
    return rc != GF_OK ? rc : gf_rowsets_reduce(r, spec, out);
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
    GfScratch buf(GF_MEM_CACHED);
    double* d_fr = nullptr; int32_t* d_st = nullptr; uint64_t* d_c = nullptr;
    const char* who = "gf_sampler_postprocess";
    buf.take(&d_fr, sizeof(double) * 3 * per_chain, who);             // sticky (gf_host.h): a run of takes is checked once
    if (status) buf.take(&d_st, sizeof(int32_t) * per_chain, who);
    if (counts) buf.take(&d_c, sizeof(uint64_t) * nbin3, who);
    if (buf.failed != GF_OK) return buf.failed;
    hipError_t e = hipSuccess;
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
    if (e != hipSuccess) return gf_hip_fail(e, who);
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
    GfScratch buf(GF_MEM_CACHED);
    double* d_fr = nullptr; int32_t* d_st = nullptr;
    buf.take(&d_fr, sizeof(double) * 3 * per_chain * v.nchains, "gf_sampler_postprocess_rows_device");
    if (buf.take(&d_st, sizeof(int32_t) * per_chain * v.nchains, "gf_sampler_postprocess_rows_device") != GF_OK) return buf.failed;
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
    GfScratch buf(GF_MEM_CACHED);
    double *d_fr = nullptr, *d_rows = nullptr; int32_t* d_st = nullptr;
    void* copy_stream = nullptr;
    hipEvent_t ev[MAX_GROUPS] = {};
    const char* who = "gf_sampler_postprocess_rows";
    buf.take(&d_fr, sizeof(double) * 3 * per_chain * v.nchains, who);
    buf.take(&d_st, sizeof(int32_t) * per_chain * v.nchains, who);
    int rc = buf.take(&d_rows, chain_bytes * v.nchains, who);
    if (rc != GF_OK) return rc;
    hipError_t e = hipSuccess;
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
    if (e != hipSuccess) return gf_hip_fail(e, who);
    return gf_internal_check_overflow(v.device, st);
}

// Stored chain -> compositions -> histogram (the steps of gf_sampler_postprocess_with, one chain after the other through the same
// scratch buffers) -> credible regions of all chains at once (gf_region.hip).  The counts never leave the device.
int gf_sampler_regions(gf_sampler* s, gf_model* const* models, int nbins, int radius, const double* weights, const double* coverage,
                       int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                       int32_t* cells, double* density)
{
    const char* who = "gf_sampler_regions";
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    int rc = gf_region_check_args(v.nchains, nbins, radius, weights, coverage, ncov, cap);
    if (rc != GF_OK) return rc;
    int cus = 256;
    if (check_chain_models(v, models, &cus) != GF_OK) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    const int64_t per_chain = v.nstored * v.nwalkers;
    GfScratch buf(GF_MEM_CACHED); GfRegionSets sets; double* d_fr = nullptr; int32_t* d_st = nullptr;
    rc = sets.begin(buf, v.nchains, nbins, cus, st, who);
    if (rc == GF_OK && per_chain > 0) { buf.take(&d_fr, sizeof(double) * 3 * per_chain, who); rc = buf.take(&d_st, sizeof(int32_t) * per_chain, who); }
    hipError_t e = hipSuccess;
    if (rc == GF_OK && per_chain > 0)
        rc = for_each_chain(v, models, d_fr, d_st, false, true, &e, [&](int ch, const double*, double*, int32_t*) { return sets.add(ch, d_fr, d_st, per_chain); });
    if (e == hipSuccess && rc == GF_OK)
        rc = sets.run(radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density);
    else
        (void)hipStreamSynchronize(st);             // a refused take included: the counts' memset may be pending when they are released
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, who);
    return per_chain > 0 ? gf_internal_check_overflow(v.device, st) : GF_OK;
}

// The marginals of every stored chain (gf_marginal.hip), and of every stored chain in element space
int gf_sampler_marginals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    return out ? chain_reduce(s, models, with_fr, false, nullptr, spec, out, "gf_sampler_marginals") : GF_ERR_INVALID_ARG;
}

int gf_sampler_element_marginals(gf_sampler* s, const gf_element_plan* plan, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    return out ? chain_reduce(s, nullptr, 0, true, plan, spec, out, "gf_sampler_element_marginals") : GF_ERR_INVALID_ARG;
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

// The column intervals of every stored chain (gf_interval.hip), and of every stored chain in element space
int gf_sampler_intervals(gf_sampler* s, gf_model* const* models, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out)
{
    return spec && out ? chain_reduce(s, models, with_fr, false, nullptr, spec, out, "gf_sampler_intervals") : GF_ERR_INVALID_ARG;
}

int gf_sampler_element_intervals(gf_sampler* s, const gf_element_plan* plan, const gf_interval_spec* spec, const gf_interval_out* out)
{
    return spec && out ? chain_reduce(s, nullptr, 0, true, plan, spec, out, "gf_sampler_element_intervals") : GF_ERR_INVALID_ARG;
}

// The energy-resolved composition of every stored chain (gf_spectrum.hip).  Chain after chain through one bin-major slab: the
// propagation leaves the verdict in d_st (its compositions go to the head of the slab and are overwritten), gf_spectrum_set fills the
// slab and reduces it with the energy bins as its chains (synchronous, so the slab is free for the next chain).
int gf_sampler_spectrum(gf_sampler* s, gf_model* const* models, const gf_spectrum_spec* spec, const gf_spectrum_out* out)
{
    const char* who = "gf_sampler_spectrum";
    GfChainView v; if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    const int64_t per_chain = v.nstored * v.nwalkers;
    if (check_chain_models(v, models) != GF_OK) return GF_ERR_INVALID_ARG;
    int nbins_e = -1;
    int rc = gf_spectrum_common_nbins(v.nchains, [&](int ch) { return chain_model(v, models, ch); }, "chain", &nbins_e);
    if (rc == GF_OK) rc = gf_spectrum_check_args(nbins_e, per_chain, spec, out);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GfScratch buf(GF_MEM_CACHED);
    double* d_slab = nullptr; int32_t* d_st = nullptr;
    buf.take(&d_slab, sizeof(double) * 3 * (size_t)per_chain * nbins_e, who);
    if (buf.take(&d_st, sizeof(int32_t) * (size_t)per_chain, who) != GF_OK) return buf.failed;
    int rs = GF_OK;
    hipError_t e = hipSuccess;
    rc = for_each_chain(v, models, d_slab, d_st, false, true, &e, [&](int ch, const double* d_theta, double*, int32_t*) {
        rs = gf_spectrum_set(chain_model(v, models, ch), st, d_theta, per_chain, d_slab, d_st, nbins_e, spec, out, ch);
        return rs == GF_OK ? hipSuccess : hipErrorUnknown;
    });
    e = first_error(e, hipStreamSynchronize(st));
    if (rc != GF_OK) return rc;
    if (rs != GF_OK) return rs;
    if (e != hipSuccess) return gf_hip_fail(e, who);
    return gf_internal_check_overflow(v.device, st);
}

}  // extern "C"
