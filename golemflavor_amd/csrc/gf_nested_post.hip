// gf_nested_post.hip -- the posterior of every run of a nested sampler (gf_nested.hip), computed where the runs' points lie: MultiNest,
// which the sampler stands in for (golemflavor/mn.py:89-101), writes its weighted samples, post_equal_weights and stats beside the
// evidence.  The arithmetic and the order of every sum are gf_nested_post.hpp's.  All runs go through one set of
// launches, blockIdx.y = run; a run without a posterior (not finished, failed, ln Z = -inf) has no points.
//   k_np_gather        the iteration-major dead points and the live set -> per-run compact lnw [n] and full-width theta [n][ndim]
// is this file's one kernel, the only one that reads the sampler's view; from the log-weights on it is the weight pipeline (gf_weights.h,
// gf_weights.hip).  The equal-weight rows [nruns][nrows][width] go through the MCMC chains' reductions (gf_rowsets.h), nchains = nruns.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_rowsets.h"
#include "gf_nested_post.hpp"
#include "gf_weights.h"

namespace {
using namespace gfnp;

constexpr int NP_BLOCK = LANES;

// what the kernels see (gf_weights.h): only k_np_gather reads the sampler's view
using NpRun = GfWeightRun;
using NpArgs = GfWeightArgs;

__global__ __launch_bounds__(NP_BLOCK) void k_np_gather(const NpArgs a, const GfNestedView v, double* __restrict__ lnw, double* __restrict__ theta)
{
    const int r = blockIdx.y, ndim = v.ndim, D = v.nscan, B = v.batch, K = v.nlive;
    const NpRun R = a.runs[r];
    const int64_t e = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x;
    if (e >= R.n * ndim) return;
    const int64_t i = e / ndim;
    const int c = (int)(e - i * ndim);
    int64_t src;                                  // the point's place in the dead or in the live arrays
    const bool dead = i < R.nd;
    if (dead) { const int64_t it = i / B; src = (it * v.nruns + r) * B + (i - it * B); }
    else src = (int64_t)r * K + (i - R.nd);
    const int sl = v.slot[c];
    double x;
    if (sl >= 0) {
        const double u = (dead ? v.d_dead_u : v.d_live_u)[src * D + sl];
        x = cube_theta(v.d_commons[r].lo[c], v.d_commons[r].hi[c], u);
    } else {
        x = v.d_bases[r * MAX_DIM + c];
    }
    theta[(R.toff + i) * ndim + c] = x;
    if (c == 0) lnw[R.off + i] = dead ? v.d_dead_w[src] : live_lnw(R.lnw0, v.d_live_l[src]);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct NpWork {
    GfScratch buf{GF_MEM_CACHED};
    NpArgs a = {};
    GfNestedView v = {};
    std::vector<GfNestedRunState> state;
    std::vector<NpRun> runs;
    int64_t total = 0, maxn = 0;
};

// the view, where every run stands, and the runs' points: w.v, w.state, w.runs, w.total, w.maxn
int np_runs(gf_nested* s, NpWork& w)
{
    GfNestedView& v = w.v;
    int rc = gf_internal_nested_view(s, &v, nullptr);
    if (rc != GF_OK) return rc;
    const int R = v.nruns;
    w.state.resize(R);
    w.runs.resize(R);
    rc = gf_internal_nested_view(s, &v, w.state.data());
    if (rc != GF_OK) return rc;
    for (int r = 0; r < R; ++r) {
        const GfNestedRunState& x = w.state[r];
        NpRun& q = w.runs[r];
        const bool ok = x.done && !x.failed && x.lnz > -HUGE_VAL;
        q.off = q.toff = w.total;
        q.nd = ok ? x.iter * v.batch : 0;
        q.n = ok ? q.nd + v.nlive : 0;
        q.lnw0 = x.lnx - std::log((double)v.nlive);          // gf_nested_get_dead's expression
        w.total += q.n;
        w.maxn = std::max(w.maxn, q.n);
    }
    return GF_OK;
}

// the gather of the runs' points on the view's stream; h_runs stays the caller's until the stream is synchronised
int np_gather(const GfNestedView& v, const NpRun* h_runs, int64_t maxn, NpRun* d_runs, double* d_lnw, double* d_theta)
{
    NpArgs a = {};
    a.runs = d_runs;
    GF_HIP(hipMemcpyAsync(d_runs, h_runs, sizeof(NpRun) * v.nruns, hipMemcpyHostToDevice, v.stream));
    const unsigned gblocks = (unsigned)std::max<int64_t>(1, (maxn * v.ndim + NP_BLOCK - 1) / NP_BLOCK);
    hipLaunchKernelGGL(k_np_gather, dim3(gblocks, (unsigned)v.nruns), dim3(NP_BLOCK), 0, v.stream, a, v, d_lnw, d_theta);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

// gather, weights and (moments) mean and covariance, (prefix) C.  Everything is enqueued on the sampler's stream; no sync at the end.
int np_prepare(gf_nested* s, NpWork& w, bool moments, bool prefix, const char* who)
{
    NpArgs& a = w.a;
    GfNestedView& v = w.v;
    int rc = np_runs(s, w);
    if (rc != GF_OK) return rc;
    const int R = v.nruns;
    a.ndim = v.ndim;
    for (int c = 0; c < MAX_DIM; ++c) a.fixed[c] = v.slot[c] < 0;
    a.seed = v.seed;
    a.ids = v.d_run_ids;
    a.maxleaves = std::max<int64_t>(1, (w.maxn + LEAF - 1) / LEAF);
    if (a.maxleaves * std::max(1, v.ndim) > 0x7fffffffll) return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: too many points per run", who);
    const size_t T = (size_t)w.total, K = moments ? GF_WEIGHT_PART_COV : GF_WEIGHT_PART;
    NpRun* d_runs = nullptr;
    double *d_lnw = nullptr, *d_theta = nullptr;
    GfScratch& buf = w.buf;
    buf.take(&d_runs, sizeof(NpRun) * R, who); buf.take(&d_lnw, sizeof(double) * T, who); buf.take(&d_theta, sizeof(double) * T * v.ndim, who);
    buf.take(&a.w, sizeof(double) * T, who); buf.take(&a.part, sizeof(double) * R * a.maxleaves * K, who);
    buf.take(&a.stat, sizeof(double) * R * GF_WEIGHT_STAT, who); buf.take(&a.mean, sizeof(double) * R * MAX_DIM, who);
    buf.take(&a.cov, sizeof(double) * R * MAX_DIM * MAX_DIM, who);
    if (prefix) { buf.take(&a.C, sizeof(double) * T, who); buf.take(&a.tot, sizeof(double) * R * a.maxleaves * GF_WEIGHT_TOT_PER_LEAF, who); }
    if (buf.failed != GF_OK) return buf.failed;
    a.runs = d_runs; a.lnw = d_lnw; a.theta = d_theta;
    rc = np_gather(v, w.runs.data(), w.maxn, d_runs, d_lnw, d_theta);
    if (rc != GF_OK) return rc;
    GF_HIP(gf_weights_launch(a, R, moments, prefix, v.stream));
    return GF_OK;
}

// Every run's N theta rows into d_theta [R][N][ndim] (d_index [R][N] filled), then gf_propagate_sets (gf_rowsets.h) over the runs into
// d_fr [.][3] and d_st (per_run: [R][N] each, else one run's, reused); a run without a posterior is not propagated: after_none(r).
// Enqueued on the sampler's stream, which is synchronised at the end.
template <class After, class AfterNone>
int np_propagated(NpWork& w, int64_t N, int64_t* d_index, double* d_theta, double* d_fr, int32_t* d_st, bool per_run, const char* who, After after,
                  AfterNone after_none)
{
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    hipError_t e = gf_weights_resample(w.a, v.nruns, N, d_index, st);
    if (e == hipSuccess) e = gf_weights_rows(w.a, N, d_index, 0, v.nruns, v.ndim, 0, d_theta, st);
    const int rc = gf_propagate_sets(v.device, st, v.nruns, N, d_fr, d_st, per_run, true, &e,
                                     [&](int r, const double** th) { *th = d_theta + (size_t)r * N * v.ndim; return w.runs[r].n ? v.models[r] : nullptr; }, after,
                                     after_none);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, who);
    return gf_internal_check_overflow(v.device, st);
}

// the equal-weight rows of every run into d_rows [R][N][(with_fr ? 3 : 0) + ndim], d_index [R][N] (NULL: scratch); synchronous
int np_rows(gf_nested* s, int64_t N, int with_fr, double* d_rows, int64_t* d_index, const char* who)
{
    if (!s || N < 1 || !d_rows) return GF_ERR_INVALID_ARG;
    NpWork w;
    int rc = np_prepare(s, w, false, true, who);
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    const size_t RN = (size_t)v.nruns * N;
    if (!d_index && (rc = w.buf.take(&d_index, sizeof(int64_t) * RN, who)) != GF_OK) return rc;
    if (!with_fr) {
        hipError_t e = gf_weights_resample(w.a, v.nruns, N, d_index, st);
        if (e == hipSuccess) e = gf_weights_rows(w.a, N, d_index, 0, v.nruns, v.ndim, 0, d_rows, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        return e != hipSuccess || e2 != hipSuccess ? gf_hip_fail(e != hipSuccess ? e : e2, who) : GF_OK;
    }
    double *d_theta = nullptr, *d_fr = nullptr; int32_t* d_st = nullptr;
    w.buf.take(&d_theta, sizeof(double) * RN * v.ndim, who); w.buf.take(&d_fr, sizeof(double) * RN * 3, who);     // sticky: checked at the last take
    if (w.buf.take(&d_st, sizeof(int32_t) * RN, who) != GF_OK) return w.buf.failed;
    const int width = 3 + v.ndim;
    return np_propagated(w, N, d_index, d_theta, d_fr, d_st, true, who,
                         [&](int r, const double* th, const double* fr, const int32_t* stt) {
                             return gf_launch_join_rows(fr, stt, th, v.ndim, N, d_rows + (size_t)r * N * width, v.cus, st); },
                         [&](int r) { return gf_weights_rows(w.a, N, d_index, r, 1, width, 3, d_rows, st); });
}

// A reducer (gf_rowsets_reduce: marginals or intervals, by the spec's type) over np_rows' rows [nruns][nrows][(with_fr ? 3 : 0) + ndim] in
// a buffer of the call's scratch, or (elements) over the theta rows pushed through `plan` into a second buffer, taken before the rows
// are made
template <class Spec, class Out>
int np_reduce(gf_nested* s, int64_t nrows, int with_fr, bool elements, const gf_element_plan* plan, const Spec* spec, const Out* out, const char* who)
{
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1) return GF_ERR_INVALID_ARG;
    const int width = elements ? gf_element_plan_width(plan, v.ndim) : (with_fr ? 3 : 0) + v.ndim;
    if (width < 0) return GF_ERR_INVALID_ARG;
    int rc = gf_rowsets_check(v.nruns, nrows, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    GfScratch buf(GF_MEM_CACHED); GfRowSets r = {nullptr, 0, v.nruns, nrows, 0, v.device, v.stream, v.cus}, e = r;
    rc = gf_rowsets_take(buf, r, elements ? v.ndim : width, who, &r);
    if (elements) rc = gf_rowsets_take(buf, r, width, who, &e);
    if (rc == GF_OK) rc = np_rows(s, nrows, with_fr, r.d_rows, nullptr, who);
    if (rc == GF_OK && elements) rc = gf_rowsets_elements(r, plan, e, who);
    return rc != GF_OK ? rc : gf_rowsets_reduce(elements ? e : r, spec, out);
}

}  // namespace

extern "C" {

// gf_internal.h: the runs' points for gf_ns_toys.hip
int gf_internal_nested_runs(gf_nested* s, GfNestedView* v, GfWeightRun* runs, int64_t* total, int64_t* maxn)
{
    if (!s || !v || !runs || !total || !maxn) return GF_ERR_INVALID_ARG;
    NpWork w;
    const int rc = np_runs(s, w);
    if (rc != GF_OK) return rc;
    *v = w.v;
    for (int r = 0; r < w.v.nruns; ++r) runs[r] = w.runs[r];
    *total = w.total;
    *maxn = w.maxn;
    return GF_OK;
}

int gf_internal_nested_gather(const GfNestedView* v, const GfWeightRun* runs, int64_t maxn, GfWeightRun* d_runs, double* d_lnw, double* d_theta)
{
    if (!v || !runs || !d_runs || !d_lnw || !d_theta) return GF_ERR_INVALID_ARG;
    return np_gather(*v, runs, maxn, d_runs, d_lnw, d_theta);
}

int gf_nested_posterior(gf_nested* s, int64_t* npoints, double* ess, double* lnz_check, double* mean, double* cov)
{
    if (!s) return GF_ERR_INVALID_ARG;
    NpWork w;
    const int rc = np_prepare(s, w, true, false, "gf_nested_posterior");
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    const int R = v.nruns, nd = v.ndim;
    std::vector<double> h_stat((size_t)R * GF_WEIGHT_STAT), h_mean((size_t)R * MAX_DIM), h_cov((size_t)R * MAX_DIM * MAX_DIM);
    hipError_t e = hipMemcpyAsync(h_stat.data(), w.a.stat, sizeof(double) * h_stat.size(), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_mean.data(), w.a.mean, sizeof(double) * h_mean.size(), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_cov.data(), w.a.cov, sizeof(double) * h_cov.size(), hipMemcpyDeviceToHost, v.stream);
    const hipError_t e2 = hipStreamSynchronize(v.stream);
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, "gf_nested_posterior");
    for (int r = 0; r < R; ++r) {
        const double* q = h_stat.data() + (size_t)r * GF_WEIGHT_STAT;
        if (npoints) npoints[r] = w.runs[r].n;
        if (ess) ess[r] = q[GF_WST_ESS];
        if (lnz_check) lnz_check[r] = w.runs[r].n ? q[GF_WST_M] + std::log(q[GF_WST_S]) : gfnp::nan();      // the host's log: a diagnostic
        for (int a = 0; a < nd; ++a) {
            if (mean) mean[(size_t)r * nd + a] = h_mean[(size_t)r * MAX_DIM + a];
            for (int b = 0; b < nd && cov; ++b) cov[((size_t)r * nd + a) * nd + b] = h_cov[((size_t)r * MAX_DIM + a) * MAX_DIM + b];
        }
    }
    return GF_OK;
}

int gf_nested_posterior_rows_device(gf_nested* s, int64_t nrows, int with_fr, double* d_rows)
{
    return np_rows(s, nrows, with_fr, d_rows, nullptr, "gf_nested_posterior_rows_device");
}

int gf_nested_posterior_rows(gf_nested* s, int64_t nrows, int with_fr, double* rows, int64_t* index)
{
    const char* who = "gf_nested_posterior_rows";
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1 || !rows) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    const size_t RN = (size_t)v.nruns * nrows, width = (with_fr ? 3 : 0) + (size_t)v.ndim;
    GfScratch buf(GF_MEM_CACHED); double* d_rows = nullptr; int64_t* d_index = nullptr;
    buf.take(&d_rows, sizeof(double) * RN * width, who);
    int rc = buf.take(&d_index, sizeof(int64_t) * RN, who);
    if (rc == GF_OK) rc = np_rows(s, nrows, with_fr, d_rows, d_index, who);
    if (rc == GF_OK) rc = gf_internal_d2h(v.device, v.stream, rows, d_rows, sizeof(double) * RN * width);
    if (rc == GF_OK && index) {
        GF_HIP(hipMemcpyAsync(index, d_index, sizeof(int64_t) * RN, hipMemcpyDeviceToHost, v.stream));
        GF_HIP(hipStreamSynchronize(v.stream));
    }
    return rc;
}

int gf_nested_marginals(gf_nested* s, int64_t nrows, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    return out ? np_reduce(s, nrows, with_fr, false, nullptr, spec, out, "gf_nested_marginals") : GF_ERR_INVALID_ARG;
}

// the column intervals (gf_interval.hip, nchains = nruns) of gf_nested_posterior_rows_device's rows, which stay on the device
int gf_nested_intervals(gf_nested* s, int64_t nrows, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out)
{
    return spec && out ? np_reduce(s, nrows, with_fr, false, nullptr, spec, out, "gf_nested_intervals") : GF_ERR_INVALID_ARG;
}

// the energy-resolved composition (gf_spectrum.hip) of every run's equal-weight rows, run after run through one bin-major slab; a run
// without a posterior is not evaluated: nvalid 0, NaN moments and order statistics, rank -1, empty histograms
int gf_nested_spectrum(gf_nested* s, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out)
{
    const char* who = "gf_nested_spectrum";
    GfNestedView v0;
    if (gf_internal_nested_view(s, &v0, nullptr) != GF_OK || nrows < 1) return GF_ERR_INVALID_ARG;
    int nbins_e = -1;
    int rc = gf_spectrum_common_nbins(v0.nruns, [&](int r) { return v0.models[r]; }, "run", &nbins_e);
    if (rc == GF_OK) rc = gf_spectrum_check_args(nbins_e, nrows, spec, out);
    if (rc != GF_OK) return rc;
    NpWork w;
    rc = np_prepare(s, w, false, true, who);
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    const size_t RN = (size_t)v.nruns * nrows;
    int64_t* d_index = nullptr; double *d_theta = nullptr, *d_slab = nullptr; int32_t* d_st = nullptr;
    w.buf.take(&d_index, sizeof(int64_t) * RN, who); w.buf.take(&d_theta, sizeof(double) * RN * v.ndim, who);
    w.buf.take(&d_slab, sizeof(double) * 3 * (size_t)nrows * nbins_e, who);
    if (w.buf.take(&d_st, sizeof(int32_t) * (size_t)nrows, who) != GF_OK) return w.buf.failed;
    const int nb1 = spec->nbins1, R2 = 2 * spec->nq;
    int rs = GF_OK;
    rc = np_propagated(w, nrows, d_index, d_theta, d_slab, d_st, false, who,
                       [&](int r, const double* th, const double*, const int32_t*) {
                           rs = gf_spectrum_set(v.models[r], st, th, nrows, d_slab, d_st, nbins_e, spec, out, r);
                           return rs == GF_OK ? hipSuccess : hipErrorUnknown;
                       },
                       [&](int r) {
                           const size_t at = (size_t)r * nbins_e;
                           for (size_t i = 0; i < (size_t)nbins_e; ++i) {
                               if (out->nvalid) out->nvalid[at + i] = 0;
                               for (int j = 0; j < 3 && out->mean; ++j) out->mean[(at + i) * 3 + j] = gfnp::nan();
                               for (int j = 0; j < 9 && out->cov; ++j) out->cov[(at + i) * 9 + j] = gfnp::nan();
                               for (int j = 0; j < 3 * R2 && out->ostat; ++j) out->ostat[(at + i) * 3 * R2 + j] = gfnp::nan();
                               for (int j = 0; j < 3 * R2 && out->orank; ++j) out->orank[(at + i) * 3 * R2 + j] = -1;
                               for (int j = 0; j < 3 * nb1 && out->counts; ++j) out->counts[(at + i) * 3 * nb1 + j] = 0;
                           }
                           return hipSuccess;
                       });
    return rs != GF_OK ? rs : rc;
}

int gf_nested_element_marginals(gf_nested* s, int64_t nrows, const gf_element_plan* plan, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    return out ? np_reduce(s, nrows, 0, true, plan, spec, out, "gf_nested_element_marginals") : GF_ERR_INVALID_ARG;
}

int gf_nested_regions(gf_nested* s, int64_t nrows, int nbins, int radius, const double* weights, const double* coverage, int ncov, int64_t cap,
                      int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass, int32_t* cells, double* density)
{
    if (!s || nrows < 1) return GF_ERR_INVALID_ARG;
    const char* who = "gf_nested_regions";
    NpWork w;
    {
        GfNestedView v;
        if (gf_internal_nested_view(s, &v, nullptr) != GF_OK) return GF_ERR_INVALID_ARG;
        const int rc = gf_region_check_args(v.nruns, nbins, radius, weights, coverage, ncov, cap);
        if (rc != GF_OK) return rc;
        GF_HIP(hipSetDevice(v.device));
    }
    int rc = np_prepare(s, w, false, true, who);
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    const size_t RN = (size_t)v.nruns * nrows;
    int64_t* d_index = nullptr; double *d_theta = nullptr, *d_fr = nullptr; int32_t* d_st = nullptr;
    GfRegionSets sets;
    w.buf.take(&d_index, sizeof(int64_t) * RN, who); w.buf.take(&d_theta, sizeof(double) * RN * v.ndim, who);
    w.buf.take(&d_fr, sizeof(double) * nrows * 3, who); w.buf.take(&d_st, sizeof(int32_t) * nrows, who);
    rc = sets.begin(w.buf, v.nruns, nbins, v.cus, v.stream, who);
    if (rc != GF_OK) return rc;
    rc = np_propagated(w, nrows, d_index, d_theta, d_fr, d_st, false, who,
                       [&](int r, const double*, double* fr, const int32_t* stt) { return sets.add(r, fr, stt, nrows); },
                       [](int) { return hipSuccess; });
    if (rc != GF_OK) return rc;
    return sets.run(radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density);
}

}  // extern "C"
