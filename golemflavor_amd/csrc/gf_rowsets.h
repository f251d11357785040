// Host pieces shared by the three sources of samples -- a sampler's stored chain (gf_postprocess.hip), a nested sampler's posterior
// (gf_nested_post.hip), a reweighted chain (gf_reweight.hip) -- for the reductions "of every set on the device".  A source checks its
// own arguments and says where its rows are (GfRowSets); the reducers by the spec's type, the element push, the region counts, the
// spectrum step and the propagate loop are written here once.  The pieces take scratch (gf_host.h: the order matters) and enqueue work
// where they are called.
#pragma once
#include "gf_host.h"
#include "gf_elements.h"
#include "gf_interval.h"
#include "gf_marginal.h"
#include "gf_region.h"
#include "gf_spectrum.h"

#pragma GCC visibility push(hidden)

// nsets sets of n rows [n][width] of doubles on the device, set k at d_rows + k * stride (written only where they are scratch)
struct GfRowSets { double* d_rows; int64_t stride; int nsets; int64_t n; int width; int device; hipStream_t stream; int cus; };

// *out: as many sets and rows as `like` (which may be *out itself), `width` columns, packed, in a buffer of buf for a source (or
// gf_rowsets_elements) to fill
inline int gf_rowsets_take(GfScratch& buf, const GfRowSets& like, int width, const char* who, GfRowSets* out)
{
    *out = like; out->width = width; out->stride = out->n * width;
    return buf.take(&out->d_rows, sizeof(double) * (size_t)out->nsets * (size_t)out->n * (size_t)width, who);
}

// the reducers, chosen by the spec's type: what check_args says of the shape (before any device work), and the reduction of the sets
inline int gf_rowsets_check(int nsets, int64_t n, int width, const gf_marginal_spec* spec) { return gf_marginal_check_args(nsets, n, width, spec); }
inline int gf_rowsets_check(int nsets, int64_t n, int width, const gf_interval_spec* spec) { return gf_interval_check_args(nsets, n, width, spec); }
inline int gf_rowsets_reduce(const GfRowSets& r, const gf_marginal_spec* spec, const gf_marginal_out* out)
{ return gf_marginal_run(r.stream, r.d_rows, r.stride, r.nsets, r.n, r.width, spec, out); }
inline int gf_rowsets_reduce(const GfRowSets& r, const gf_interval_spec* spec, const gf_interval_out* out)
{ return gf_interval_run(r.stream, r.d_rows, r.stride, r.nsets, r.n, r.width, spec, out, nullptr); }

// `in` in element space (gf_elements.hip) into `out`, a row set taken with the plan's width; enqueued on in.stream
inline int gf_rowsets_elements(const GfRowSets& in, const gf_element_plan* plan, const GfRowSets& out, const char* who)
{
    const hipError_t e = gf_element_run(in.stream, in.d_rows, in.stride, in.nsets, in.n, in.width, plan, out.d_rows, out.stride, in.cus);
    return e == hipSuccess ? GF_OK : gf_hip_fail(e, who);
}

// the flavor histograms of nsets sets of compositions, [nsets][nbins^3] in the call's scratch, and their credible regions
struct GfRegionSets {
    uint64_t* d_c = nullptr; int nsets = 0, nbins = 0, cus = 0; hipStream_t st = nullptr;
    size_t nbin3() const { return (size_t)nbins * nbins * nbins; }
    // the counts taken from buf and zeroed on `stream`
    int begin(GfScratch& buf, int nsets_, int nbins_, int cus_, hipStream_t stream, const char* who)
    {
        nsets = nsets_; nbins = nbins_; cus = cus_; st = stream;
        if (buf.take(&d_c, sizeof(uint64_t) * nbin3() * nsets, who) != GF_OK) return buf.failed;
        const hipError_t e = hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nbin3() * nsets, st);
        if (e != hipSuccess) (void)hipStreamSynchronize(st);          // what the caller enqueued before is done when its scratch goes
        return e == hipSuccess ? GF_OK : gf_hip_fail(e, who);
    }
    // set k's compositions d_fr [n][3] added to its histogram; d_status: those whose status is not GF_ST_OK are left out (overwritten)
    hipError_t add(int k, double* d_fr, const int32_t* d_status, int64_t n) const
    {
        const hipError_t e = d_status ? gf_launch_mask_fr(d_fr, d_status, n, st) : hipSuccess;
        return e != hipSuccess ? e : gf_launch_flavor_hist(d_fr, n, nbins, (unsigned long long*)(d_c + (size_t)k * nbin3()), cus, st);
    }
    // the regions of all sets at once (gf_region.hip, whose outputs these are); synchronous
    int run(int radius, const double* weights, const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in,
            double* level_out, double* mass, int32_t* cells, double* density) const
    {
        return gf_region_run(st, d_c, nsets, nbins, radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density, nullptr);
    }
};

// *nbins: the energy bins of model_of(k), k < nsets, all the same number; a model without any: GF_ERR_UNSUPPORTED.  what: "chain", "run"
template <class ModelOf>
int gf_spectrum_common_nbins(int nsets, ModelOf model_of, const char* what, int* nbins)
{
    *nbins = -1;
    for (int k = 0; k < nsets; ++k) {
        const int nb = gf_model_nbins(model_of(k));
        if (nb < 1) return GF_ERR_UNSUPPORTED;
        if (*nbins >= 0 && nb != *nbins)
            return gf_fail_msg(GF_ERR_INVALID_ARG, "spectrum: %s %d has %d energy bins, %s 0 has %d", what, k, nb, what, *nbins);
        *nbins = nb;
    }
    return GF_OK;
}

// set k of a spectrum call: the compositions of d_theta's n rows at every energy bin of `m` into the bin-major slab (the verdicts of
// the set's propagation are in d_st), reduced into `out` at k.  gf_marginal_run underneath is synchronous: the slab is free again
inline int gf_spectrum_set(gf_model* m, hipStream_t st, const double* d_theta, int64_t n, double* d_slab, const int32_t* d_st, int nbins_e,
                           const gf_spectrum_spec* spec, const gf_spectrum_out* out, int k)
{
    const int rs = gf_model_bins_on(m, st, d_theta, GF_LAYOUT_AOS, n, d_slab, 1, d_st);
    return rs != GF_OK ? rs : gf_spectrum_reduce(st, d_slab, nbins_e, n, spec, out, k);
}

// Set k = 0 .. nsets - 1 of n rows: model = set_of(k, &theta), theta propagated with it on `st` into d_fr [.][3] and d_st (may be NULL),
// then *e = after(k, theta, fr_k, st_k); a set that has nothing (model NULL): *e = nothing(k) instead.  Stops at the first failure of
// either (returns the propagation's code).  per_set: set k has its own part of d_fr and d_st, else all share one.
// full_grids: the sets are enqueued faster than they run, so the arbitration grid of each would follow what some EARLIER set found,
// and the sets of a scan differ (its high-scale grid points sit in the failing region, the others have empty queues): full grids
// throughout, ~30 us per set (measured: the hint left 57 of 64 chains of the C4 scan on a sixth of the GPU, 114 ms instead of ~20)
template <class SetOf, class After, class Nothing>
int gf_propagate_sets(int device, hipStream_t st, int nsets, int64_t n, double* d_fr, int32_t* d_st, bool per_set, bool full_grids, hipError_t* e,
                      SetOf set_of, After after, Nothing nothing)
{
    int rc = GF_OK;
    if (full_grids) gf_internal_full_arbitration_grids(device, st, 1);
    for (int k = 0; k < nsets && rc == GF_OK && *e == hipSuccess && n > 0; ++k) {
        const size_t at = per_set ? (size_t)k * n : 0;
        const double* theta = nullptr;
        gf_model* m = set_of(k, &theta);
        if (!m) { *e = nothing(k); continue; }
        rc = gf_model_propagate_on(m, st, theta, GF_LAYOUT_AOS, n, d_fr + at * 3, d_st ? d_st + at : nullptr);
        if (rc == GF_OK) *e = after(k, theta, d_fr + at * 3, d_st ? d_st + at : nullptr);
    }
    if (full_grids) gf_internal_full_arbitration_grids(device, st, 0);
    return rc;
}

#pragma GCC visibility pop
