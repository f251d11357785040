// gf_reweight.hip -- every stored chain of a sampler reweighted to other targets: the log-weights lnw = l_t - l0 of the
// chain's rows under each target by gf_reweight.hpp's rules, then the weight pipeline (gf_weights.h, gf_weights.hip) with the T
// targets of a chain as T runs that share one theta, the chain's rows in place.  The equal-weight rows [nchains * T][N][width] are
// one of the three sources of gf_rowsets.h (rw_row_sets) for the reductions.
//   k_rw_gauss   measurement targets: a lane per row; the row's composition and status (one propagation of the chain) are read once,
//                the Gaussian block of lnprob is evaluated for the sampling model and for every target (constants in the kernel
//                arguments), lnw [t][i] is written target by target, consecutive lanes on consecutive rows
//   k_rw_sub     model targets: l_t (the target's lnprob, in place) and the stored l0 -> lnw, the same rules
//   counters     per chain bad_base, per (chain, target) nonunitary, outside, kept: a ballot per wave and one vector atomic per wave
//   k_rw_runs    the batch's runs for the weight pipeline, on the device: a target without a kept row has no posterior (n = 0)
//   k_rw_take_fr the composition of every equal-weight row, gathered by its index from the chain's propagation
// Chains go one after another on the sampler's stream, all targets of a chain in one set of launches; the targets are cut into
// batches so that the three doubles per (target, row) stay under GF_REWEIGHT_SCRATCH_DEFAULT (GF_REWEIGHT_SCRATCH_BYTES overrides:
// the batching changes, no result does).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_rowsets.h"
#include "gf_device.hpp"
#include "gf_reweight.hpp"
#include "gf_weights.h"

#define GF_REWEIGHT_SCRATCH_DEFAULT ((size_t)2 << 30)

namespace {
using namespace gfrw;

constexpr int RW_BLOCK = 256;
constexpr int RW_CNT = 3;               // counters per (chain, target): nonunitary, outside, kept; one per chain in front: bad_base
static_assert(MAX_TARGETS == GF_REWEIGHT_MAX_TARGETS, "gf_reweight.hpp states the public limit");
static_assert(STATUS_NON_UNITARY == GF_ST_NON_UNITARY, "gf_reweight.hpp states the public status");

struct RwGauss { double bf[3], mh, k, offset; };          // gf_device.hpp's gauss_llh: GfCommon's bf, gauss_mh, gauss_k, offset

struct RwGaussArgs {
    const double* fr;                   // [n][3]
    const int32_t* st;                  // [n]
    int64_t n;
    int32_t T, count_base;              // targets of this launch; != 0: this launch counts bad_base
    double* lnw;                        // [T][n]
    unsigned long long* cnt;            // the chain's [1 + RW_CNT * ntargets], from this launch's first target on: cnt_t = cnt + 1 + RW_CNT * t
    unsigned long long* cnt_base;       // the chain's bad_base
    RwGauss base;
    RwGauss tg[MAX_TARGETS];
};

// gauss_llh (gf_device.hpp) on a target's constants: the same operations in the same order.  Restated, not shared: gauss_llh takes
// a GfCommon, and giving it a helper to forward to changes the register allocation and the schedule of the lnprob, BSM and sampler
// kernels (compared in their assembly), which this file must leave as they are.  tests/test_gpu_reweight.py holds the two to each
// other: lnw of this path against the model path at the bound of identical Gaussian blocks.
__device__ __forceinline__ double rw_mg(const RwGauss& g, const double fr[3])
{
    const double d0 = fr[0] - g.bf[0];
    const double d1 = fr[1] - g.bf[1];
    const double d2 = fr[2] - g.bf[2];
    const double r2 = fma(d2, d2, fma(d1, d1, d0 * d0));
    const double logpdf = fma(g.mh, r2, g.k);
    return gfdev::log_of_exp(logpdf) + g.offset;
}

// the rows of the wave that are of `kind`, added to *c by one lane
__device__ __forceinline__ void rw_count(bool mine, unsigned long long* c)
{
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(c, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(RW_BLOCK) void k_rw_gauss(const RwGaussArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const bool live = i < a.n;
    double fr[3] = {0.0, 0.0, 0.0};
    int32_t st = 0;
    if (live) { fr[0] = a.fr[3 * i]; fr[1] = a.fr[3 * i + 1]; fr[2] = a.fr[3 * i + 2]; st = a.st[i]; }
    const double l0 = rw_mg(a.base, fr);
    if (a.count_base) rw_count(live && classify(0.0, l0, st) == RW_BAD_BASE, a.cnt_base);
    for (int t = 0; t < a.T; ++t) {                                   // uniform: the constants come by scalar loads
        const double lt = rw_mg(a.tg[t], fr);
        const int kind = classify(lt, l0, st);
        if (live) a.lnw[(int64_t)t * a.n + i] = lnw(lt, l0, kind);
        unsigned long long* c = a.cnt + RW_CNT * t;
        rw_count(live && kind == RW_NONUNITARY, c);
        rw_count(live && kind == RW_OUTSIDE, c + 1);
        rw_count(live && kind == RW_KEPT, c + 2);
    }
}

// lt [n]: the target's lnprob in, lnw out; l0 [n] the stored ln_prob; st [n] the rows' status under the target
__global__ __launch_bounds__(RW_BLOCK) void k_rw_sub(double* __restrict__ lt, const double* __restrict__ l0, const int32_t* __restrict__ st,
                                                     int64_t n, unsigned long long* cnt, unsigned long long* cnt_base, int count_base)
{
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const bool live = i < n;
    const double b = live ? l0[i] : 0.0, x = live ? lt[i] : 0.0;
    const int kind = classify(x, b, live ? st[i] : 0);
    if (live) lt[i] = lnw(x, b, kind);
    if (count_base) rw_count(live && kind == RW_BAD_BASE, cnt_base);
    rw_count(live && kind == RW_NONUNITARY, cnt);
    rw_count(live && kind == RW_OUTSIDE, cnt + 1);
    rw_count(live && kind == RW_KEPT, cnt + 2);
}

// one block: the runs and resampling ids of the targets t0 .. t0 + Tb - 1 of a chain
__global__ __launch_bounds__(MAX_TARGETS) void k_rw_runs(GfWeightRun* runs, uint64_t* ids, const unsigned long long* cnt, int64_t n, int Tb,
                                                         int t0, uint64_t sid)
{
    const int r = threadIdx.x;
    if (r >= Tb) return;
    GfWeightRun q;
    q.off = (int64_t)r * n;
    q.toff = 0;
    q.n = cnt[RW_CNT * r + 2] ? n : 0;
    q.nd = 0;
    q.lnw0 = 0.0;
    runs[r] = q;
    ids[r] = resample_id(sid, t0 + r);
}

// rows [R][N][width]: columns 0 .. 2 of every row with a point = the composition of that point; fr [n][3], index [R][N]
__global__ __launch_bounds__(RW_BLOCK) void k_rw_take_fr(const double* __restrict__ fr, const int64_t* __restrict__ index, int64_t RN, int width,
                                                         double* __restrict__ rows)
{
    const int64_t e = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (e >= RN * 3) return;
    const int64_t k = e / 3;
    const int c = (int)(e - k * 3);
    const int64_t idx = index[k];
    if (idx >= 0) rows[k * width + c] = fr[idx * 3 + c];
}

// fr3 [n][3] = the first three columns of rows [n][width]
__global__ __launch_bounds__(RW_BLOCK) void k_rw_fr3(const double* __restrict__ rows, int64_t n, int width, double* __restrict__ fr3)
{
    const int64_t e = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (e >= n * 3) return;
    const int64_t k = e / 3;
    fr3[e] = rows[k * width + (e - k * 3)];
}

unsigned rw_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + RW_BLOCK - 1) / RW_BLOCK); }

size_t rw_scratch_cap()
{
    const char* v = gf_internal_env("GF_REWEIGHT_SCRATCH_BYTES", 0);
    if (v) {
        const long long b = std::atoll(v);
        if (b > 0) return (size_t)b;
    }
    return (size_t)GF_REWEIGHT_SCRATCH_DEFAULT;
}

gf_model* rw_chain_model(const GfChainView& v, int ch) { return v.models ? v.models[ch] : v.model; }

// what a call wants of the engine
struct RwWant {
    const gf_reweight_out* out = nullptr;       // the summary
    int lnw_chain = -1;                         // >= 0: this chain alone, its log-weights to lnw [T][n]
    double* lnw = nullptr;
    int64_t N = 0;                              // > 0: equal-weight rows
    int with_fr = 0;
    double* d_rows = nullptr;                   // [nchains][T][N][width]
    int64_t* d_index = nullptr;                 // [nchains][T][N], NULL: scratch
};

int rw_check(const GfChainView& v, const gf_reweight_spec* spec, const char* who)
{
    if (!spec || spec->ntargets < 1 || spec->ntargets > GF_REWEIGHT_MAX_TARGETS) return GF_ERR_INVALID_ARG;
    if (v.nstored < 1 || !v.d_chain || !v.d_lnp_chain) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: nothing stored", who);
    const int T = spec->ntargets;
    for (int ch = 0; ch < v.nchains; ++ch) {
        const GfCommon* c; const GfBsm* tb; const double* ptab; int device, cus, nbins;
        if (spec->models) {
            for (int t = 0; t < T; ++t)
                if (gf_model_constants(spec->models[(size_t)ch * T + t], &c, &tb, &ptab, &device, &cus, &nbins) != GF_OK || c->ndim != v.ndim ||
                    device != v.device)
                    return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: target %d of chain %d is no model of the sampler's ndim and device", who, t, ch);
            continue;
        }
        if (!spec->bestfit_fr || !spec->smearing || !spec->offset) return GF_ERR_INVALID_ARG;
        if (gf_model_constants(rw_chain_model(v, ch), &c, &tb, &ptab, &device, &cus, &nbins) != GF_OK) return GF_ERR_INVALID_ARG;
        if (c->mode != GF_MODE_SM_GAUSS && c->mode != GF_MODE_BSM_GAUSS)
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: chain %d was not sampled under a Gaussian measurement; give model targets", who, ch);
        for (int t = 0; t < T; ++t) {
            const size_t at = (size_t)ch * T + t;
            const double* bf = spec->bestfit_fr + 3 * at;
            if (!(spec->smearing[at] > 0.0) || !std::isfinite(spec->smearing[at]) || !std::isfinite(bf[0]) || !std::isfinite(bf[1]) ||
                !std::isfinite(bf[2]) || !std::isfinite(spec->offset[at]))
                return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: target %d of chain %d: smearing must be > 0, bestfit_fr and offset finite", who, t, ch);
        }
    }
    return GF_OK;
}

// The engine: for the chains [c0, c1) and every batch of targets -- lnw, the runs, the weight pipeline, and what `want` asks for.
// Everything is enqueued on the sampler's stream, which is synchronised at the end.
int rw_run(gf_sampler* s, const gf_reweight_spec* spec, const RwWant& want, const char* who)
{
    GfChainView v;
    if (gf_internal_sampler_chain_view(s, &v) != GF_OK) return GF_ERR_INVALID_ARG;
    int rc = rw_check(v, spec, who);
    if (rc != GF_OK) return rc;
    // measurement targets replace the chain's own Gaussian measurement; a chain sampled under a measurement per energy bin has none
    const int sampled = gf_internal_sampler_likelihood(s);
    if (!spec->models && sampled == GF_LLH_BINNED)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the sampler's chains were sampled under the energy-resolved likelihood, which has no single "
                           "Gaussian measurement to replace; give model targets", who);
    if (!spec->models && sampled == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the sampler's chains were sampled under a tabulated likelihood, which has no Gaussian measurement "
                           "to replace; give model targets", who);
    const int T = spec->ntargets, nd = v.ndim, nch = v.nchains;
    const int64_t n = v.nstored * v.nwalkers, N = want.N;
    const bool measured = !spec->models, moments = want.out && (want.out->mean || want.out->cov), prefix = N > 0;
    if (want.lnw_chain >= nch || (N > 0 && !want.d_rows)) return GF_ERR_INVALID_ARG;
    const int c0 = want.lnw_chain >= 0 ? want.lnw_chain : 0, c1 = want.lnw_chain >= 0 ? want.lnw_chain + 1 : nch;
    GF_HIP(hipSetDevice(v.device));
    hipStream_t st = v.stream;
    GF_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> sid(nch);
    for (int ch = 0; ch < nch; ++ch) sid[ch] = (uint64_t)ch;
    if (v.d_stream_ids) GF_HIP(hipMemcpy(sid.data(), v.d_stream_ids, sizeof(uint64_t) * nch, hipMemcpyDeviceToHost));

    const int Tb = (int)std::min<size_t>((size_t)T, std::max<size_t>(1, rw_scratch_cap() / (3 * sizeof(double) * (size_t)n)));
    GfWeightArgs a = {};
    a.ndim = nd;
    a.seed = spec->use_sampler_seed ? v.seed : spec->seed;
    a.maxleaves = std::max<int64_t>(1, (n + GF_WEIGHT_LEAF - 1) / GF_WEIGHT_LEAF);
    if (a.maxleaves * std::max(1, nd) > 0x7fffffffll) return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: too many rows per chain", who);
    const size_t K = moments ? GF_WEIGHT_PART_COV : GF_WEIGHT_PART, CT = (size_t)nch * T, ncnt = 1 + (size_t)RW_CNT * T;
    const int width = (want.with_fr ? 3 : 0) + nd;

    GfScratch buf(GF_MEM_CACHED);
    double *d_fr = nullptr, *d_lnw = nullptr, *d_stat = nullptr, *d_mean = nullptr, *d_cov = nullptr, *d_thN = nullptr, *d_frN = nullptr;
    int32_t *d_st = nullptr, *d_stN = nullptr;
    GfWeightRun* d_runs = nullptr;
    uint64_t* d_ids = nullptr;
    unsigned long long* d_cnt = nullptr;
    int64_t* d_index = want.d_index;
    buf.take(&d_st, sizeof(int32_t) * n, who);                        // sticky (gf_host.h): the run of takes is checked once, below
    if (measured) buf.take(&d_fr, sizeof(double) * 3 * n, who);
    buf.take(&d_lnw, sizeof(double) * Tb * n, who); buf.take(&a.w, sizeof(double) * Tb * n, who);
    buf.take(&a.part, sizeof(double) * Tb * a.maxleaves * K, who); buf.take(&d_stat, sizeof(double) * CT * GF_WEIGHT_STAT, who);
    buf.take(&d_mean, sizeof(double) * CT * GF_MAX_DIM, who); buf.take(&d_cov, sizeof(double) * CT * GF_MAX_DIM * GF_MAX_DIM, who);
    buf.take(&d_runs, sizeof(GfWeightRun) * Tb, who); buf.take(&d_ids, sizeof(uint64_t) * Tb, who);
    buf.take(&d_cnt, sizeof(unsigned long long) * nch * ncnt, who);
    if (prefix) { buf.take(&a.C, sizeof(double) * Tb * n, who); buf.take(&a.tot, sizeof(double) * Tb * a.maxleaves * GF_WEIGHT_TOT_PER_LEAF, who); }
    if (prefix && !d_index) buf.take(&d_index, sizeof(int64_t) * CT * N, who);
    if (prefix && want.with_fr && !measured) {
        buf.take(&d_thN, sizeof(double) * Tb * N * nd, who); buf.take(&d_frN, sizeof(double) * 3 * N, who); buf.take(&d_stN, sizeof(int32_t) * N, who);
    }
    if (buf.failed != GF_OK) return buf.failed;
    a.lnw = d_lnw;
    a.runs = d_runs;
    a.ids = d_ids;

    hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * nch * ncnt, st);
    std::vector<unsigned long long> h_cnt((size_t)nch * ncnt, 0);
    gf_internal_full_arbitration_grids(v.device, st, 1);             // the chains of a scan differ (gf_rowsets.h gf_propagate_sets)
    for (int ch = c0; ch < c1 && rc == GF_OK && e == hipSuccess; ++ch) {
        const double* theta = v.d_chain + (size_t)ch * v.nstore_cap * v.nwalkers * nd;
        const double* l0 = v.d_lnp_chain + (size_t)ch * v.nstore_cap * v.nwalkers;
        unsigned long long* cnt = d_cnt + (size_t)ch * ncnt;
        a.theta = theta;
        RwGaussArgs g = {};
        if (measured) {
            gf_model* m = rw_chain_model(v, ch);
            rc = gf_model_propagate_on(m, st, theta, GF_LAYOUT_AOS, n, d_fr, d_st);
            if (rc != GF_OK) break;
            const GfCommon* c; const GfBsm* tb; const double* ptab; int device, cus, nbins;
            (void)gf_model_constants(m, &c, &tb, &ptab, &device, &cus, &nbins);
            g.fr = d_fr; g.st = d_st; g.n = n; g.lnw = d_lnw; g.cnt_base = cnt;
            g.base = RwGauss{{c->bf[0], c->bf[1], c->bf[2]}, c->gauss_mh, c->gauss_k, c->offset};
        }
        for (int t0 = 0; t0 < T && rc == GF_OK && e == hipSuccess; t0 += Tb) {
            const int tb_n = std::min(Tb, T - t0);
            unsigned long long* cnt_t = cnt + 1 + (size_t)RW_CNT * t0;
            if (measured) {
                g.T = tb_n; g.count_base = t0 == 0; g.cnt = cnt_t;
                for (int r = 0; r < tb_n; ++r) {
                    const size_t at = (size_t)ch * T + t0 + r;
                    double inv_smear, c0g;
                    RwGauss& q = g.tg[r];
                    for (int k = 0; k < 3; ++k) q.bf[k] = spec->bestfit_fr[3 * at + k];
                    gf_internal_gauss_consts(spec->smearing[at], &inv_smear, &c0g, &q.mh, &q.k);
                    q.offset = spec->offset[at];
                }
                hipLaunchKernelGGL(k_rw_gauss, dim3(rw_blocks(n)), dim3(RW_BLOCK), 0, st, g);
            } else {
                for (int r = 0; r < tb_n && rc == GF_OK; ++r) {
                    double* lt = d_lnw + (size_t)r * n;
                    rc = gf_model_lnprob_on(spec->models[(size_t)ch * T + t0 + r], st, theta, GF_LAYOUT_AOS, n, lt, nullptr, d_st);
                    if (rc == GF_OK)
                        hipLaunchKernelGGL(k_rw_sub, dim3(rw_blocks(n)), dim3(RW_BLOCK), 0, st, lt, l0, d_st, n, cnt_t + RW_CNT * r, cnt,
                                           (int)(t0 + r == 0));
                }
                if (rc != GF_OK) break;
            }
            e = hipGetLastError();
            if (e == hipSuccess && want.lnw)
                e = hipMemcpyAsync(want.lnw + (size_t)t0 * n, d_lnw, sizeof(double) * tb_n * n, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess || (!want.out && !prefix)) continue;
            hipLaunchKernelGGL(k_rw_runs, dim3(1), dim3(MAX_TARGETS), 0, st, d_runs, d_ids, cnt_t, n, tb_n, t0, sid[ch]);
            const size_t at = (size_t)ch * T + t0;
            a.stat = d_stat + at * GF_WEIGHT_STAT;
            a.mean = d_mean + at * GF_MAX_DIM;
            a.cov = d_cov + at * GF_MAX_DIM * GF_MAX_DIM;
            e = gf_weights_launch(a, tb_n, moments, prefix, st);
            if (e != hipSuccess || !prefix) continue;
            int64_t* idx = d_index + at * N;
            double* rows = want.d_rows + at * N * width;
            e = gf_weights_resample(a, tb_n, N, idx, st);
            if (e == hipSuccess && (!want.with_fr || measured)) e = gf_weights_rows(a, N, idx, 0, tb_n, width, want.with_fr ? 3 : 0, rows, st);
            if (e == hipSuccess && want.with_fr && measured) {
                hipLaunchKernelGGL(k_rw_take_fr, dim3(rw_blocks((int64_t)tb_n * N * 3)), dim3(RW_BLOCK), 0, st, d_fr, idx, (int64_t)tb_n * N, width, rows);
                e = hipGetLastError();
            }
            if (e == hipSuccess && want.with_fr && !measured) {
                // the nrows rows of every target propagated with it (a target without a posterior is not: NaN rows); which targets have
                // one is read back here, the only wait inside the loop
                e = gf_weights_rows(a, N, idx, 0, tb_n, nd, 0, d_thN, st);
                if (e == hipSuccess) e = hipMemcpyAsync(h_cnt.data() + (size_t)ch * ncnt, cnt, sizeof(unsigned long long) * ncnt, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipStreamSynchronize(st);
                for (int r = 0; r < tb_n && rc == GF_OK && e == hipSuccess; ++r) {
                    if (!h_cnt[(size_t)ch * ncnt + 1 + (size_t)RW_CNT * (t0 + r) + 2]) { e = gf_weights_rows(a, N, idx, r, 1, width, 3, rows, st); continue; }
                    const double* th = d_thN + (size_t)r * N * nd;
                    rc = gf_model_propagate_on(spec->models[at + r], st, th, GF_LAYOUT_AOS, N, d_frN, d_stN);
                    if (rc == GF_OK) e = gf_launch_join_rows(d_frN, d_stN, th, nd, N, rows + (size_t)r * N * width, v.cus, st);
                }
            }
        }
    }
    gf_internal_full_arbitration_grids(v.device, st, 0);
    std::vector<double> h_stat, h_mean, h_cov;
    if (rc == GF_OK && e == hipSuccess) e = hipMemcpyAsync(h_cnt.data(), d_cnt, sizeof(unsigned long long) * nch * ncnt, hipMemcpyDeviceToHost, st);
    if (rc == GF_OK && e == hipSuccess && want.out) {
        h_stat.resize(CT * GF_WEIGHT_STAT);
        e = hipMemcpyAsync(h_stat.data(), d_stat, sizeof(double) * h_stat.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && moments) {
            h_mean.resize(CT * GF_MAX_DIM);
            h_cov.resize(CT * GF_MAX_DIM * GF_MAX_DIM);
            e = hipMemcpyAsync(h_mean.data(), d_mean, sizeof(double) * h_mean.size(), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h_cov.data(), d_cov, sizeof(double) * h_cov.size(), hipMemcpyDeviceToHost, st);
        }
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, who);
    rc = gf_internal_check_overflow(v.device, st);
    if (rc != GF_OK || !want.out) return rc;
    const gf_reweight_out& o = *want.out;
    for (int ch = 0; ch < nch; ++ch) {
        const unsigned long long* cnt = h_cnt.data() + (size_t)ch * ncnt;
        if (o.n) o.n[ch] = n;
        if (o.bad_base) o.bad_base[ch] = (int64_t)cnt[0];
        for (int t = 0; t < T; ++t) {
            const size_t at = (size_t)ch * T + t;
            const unsigned long long* ct = cnt + 1 + (size_t)RW_CNT * t;
            const double* q = h_stat.data() + at * GF_WEIGHT_STAT;
            if (o.nonunitary) o.nonunitary[at] = (int64_t)ct[0];
            if (o.outside) o.outside[at] = (int64_t)ct[1];
            if (o.ess) o.ess[at] = q[GF_WST_ESS];
            if (o.lnz_ratio) o.lnz_ratio[at] = ct[2] ? q[GF_WST_M] + std::log(q[GF_WST_S]) - std::log((double)n) : __builtin_nan("");   // the host's log: a diagnostic
            for (int c = 0; c < nd && moments; ++c) {
                if (o.mean) o.mean[at * nd + c] = h_mean[at * GF_MAX_DIM + c];
                for (int b = 0; b < nd && o.cov; ++b) o.cov[(at * nd + c) * nd + b] = h_cov[(at * GF_MAX_DIM + c) * GF_MAX_DIM + b];
            }
        }
    }
    return GF_OK;
}

// what the rows and reduction entry points ask first
bool rw_view(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, GfChainView* v)
{
    return gf_internal_sampler_chain_view(s, v) == GF_OK && rw && rw->ntargets >= 1 && rw->ntargets <= GF_REWEIGHT_MAX_TARGETS && nrows >= 1;
}

// The equal-weight rows of every (chain, target) for a reducer, in a buffer of buf: *r [nchains * T][N][(with_fr ? 3 : 0) + ndim].
// check: what the reducer's check_args says of (nchains * T, N, width), before any device work
template <class Check>
int rw_row_sets(gf_sampler* s, const gf_reweight_spec* rw, int64_t N, int with_fr, Check check, GfScratch& buf, const char* who, GfRowSets* r)
{
    GfChainView v;
    if (!rw_view(s, rw, N, &v)) return GF_ERR_INVALID_ARG;
    const int width = (with_fr ? 3 : 0) + v.ndim, batch = v.nchains * rw->ntargets;
    int rc = check(batch, N, width);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    RwWant w; w.N = N; w.with_fr = with_fr;
    rc = gf_rowsets_take(buf, GfRowSets{nullptr, 0, batch, N, 0, v.device, v.stream, v.cus}, width, who, r);
    w.d_rows = r->d_rows;
    return rc != GF_OK ? rc : rw_run(s, rw, w, who);
}

// a reducer (gf_rowsets_reduce: marginals or intervals, by the spec's type) over rw_row_sets' rows
template <class Spec, class Out>
int rw_reduce(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int with_fr, const Spec* spec, const Out* out, const char* who)
{
    GfScratch buf(GF_MEM_CACHED); GfRowSets r;
    const int rc = rw_row_sets(s, rw, nrows, with_fr, [&](int nsets, int64_t n, int width) { return gf_rowsets_check(nsets, n, width, spec); }, buf, who, &r);
    return rc != GF_OK ? rc : gf_rowsets_reduce(r, spec, out);
}

}  // namespace

extern "C" {

int gf_sampler_reweight(gf_sampler* s, const gf_reweight_spec* spec, const gf_reweight_out* out)
{
    if (!s || !spec || !out) return GF_ERR_INVALID_ARG;
    RwWant w;
    w.out = out;
    return rw_run(s, spec, w, "gf_sampler_reweight");
}

int gf_sampler_reweight_lnw(gf_sampler* s, const gf_reweight_spec* spec, int chain, double* lnw)
{
    if (!s || !spec || chain < 0 || !lnw) return GF_ERR_INVALID_ARG;
    RwWant w;
    w.lnw_chain = chain;
    w.lnw = lnw;
    return rw_run(s, spec, w, "gf_sampler_reweight_lnw");
}

int gf_sampler_reweight_rows_device(gf_sampler* s, const gf_reweight_spec* spec, int64_t nrows, int with_fr, double* d_rows)
{
    if (!s || !spec || nrows < 1 || !d_rows) return GF_ERR_INVALID_ARG;
    RwWant w;
    w.N = nrows; w.with_fr = with_fr; w.d_rows = d_rows;
    return rw_run(s, spec, w, "gf_sampler_reweight_rows_device");
}

int gf_sampler_reweight_rows(gf_sampler* s, const gf_reweight_spec* spec, int64_t nrows, int with_fr, double* rows, int64_t* index)
{
    const char* who = "gf_sampler_reweight_rows";
    GfChainView v;
    if (!rw_view(s, spec, nrows, &v) || !rows) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    const size_t RN = (size_t)v.nchains * spec->ntargets * nrows, width = (with_fr ? 3 : 0) + (size_t)v.ndim;
    GfScratch buf(GF_MEM_CACHED); RwWant w; w.N = nrows; w.with_fr = with_fr;
    buf.take(&w.d_rows, sizeof(double) * RN * width, who);
    int rc = buf.take(&w.d_index, sizeof(int64_t) * RN, who);
    if (rc == GF_OK) rc = rw_run(s, spec, w, who);
    if (rc == GF_OK) rc = gf_internal_d2h(v.device, v.stream, rows, w.d_rows, sizeof(double) * RN * width);
    if (rc == GF_OK && index) {
        GF_HIP(hipMemcpyAsync(index, w.d_index, sizeof(int64_t) * RN, hipMemcpyDeviceToHost, v.stream));
        GF_HIP(hipStreamSynchronize(v.stream));
    }
    return rc;
}

int gf_sampler_reweight_marginals(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int with_fr, const gf_marginal_spec* spec,
                                  const gf_marginal_out* out)
{
    return out ? rw_reduce(s, rw, nrows, with_fr, spec, out, "gf_sampler_reweight_marginals") : GF_ERR_INVALID_ARG;
}

int gf_sampler_reweight_intervals(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int with_fr, const gf_interval_spec* spec,
                                  const gf_interval_out* out)
{
    return spec && out ? rw_reduce(s, rw, nrows, with_fr, spec, out, "gf_sampler_reweight_intervals") : GF_ERR_INVALID_ARG;
}

// the rows with their compositions, the compositions alone, a histogram per (chain, target), the regions of all of them at once
int gf_sampler_reweight_regions(gf_sampler* s, const gf_reweight_spec* rw, int64_t nrows, int nbins, int radius, const double* weights,
                                const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in,
                                double* level_out, double* mass, int32_t* cells, double* density)
{
    const char* who = "gf_sampler_reweight_regions";
    GfScratch buf(GF_MEM_CACHED); GfRowSets r;
    int rc = rw_row_sets(s, rw, nrows, 1, [&](int nsets, int64_t, int) { return gf_region_check_args(nsets, nbins, radius, weights, coverage, ncov, cap); },
                         buf, who, &r);
    if (rc != GF_OK) return rc;
    double* d_fr3 = nullptr; GfRegionSets sets;
    buf.take(&d_fr3, sizeof(double) * 3 * (size_t)r.nsets * nrows, who);
    rc = sets.begin(buf, r.nsets, nbins, r.cus, r.stream, who);
    if (rc != GF_OK) return rc;
    hipLaunchKernelGGL(k_rw_fr3, dim3(rw_blocks((int64_t)r.nsets * nrows * 3)), dim3(RW_BLOCK), 0, r.stream, r.d_rows, (int64_t)r.nsets * nrows, r.width, d_fr3);
    hipError_t e = hipGetLastError();
    for (int k = 0; k < r.nsets && e == hipSuccess; ++k) e = sets.add(k, d_fr3 + (size_t)k * nrows * 3, nullptr, nrows);
    if (e != hipSuccess) { (void)hipStreamSynchronize(r.stream); return gf_hip_fail(e, who); }
    return sets.run(radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density);
}

}  // extern "C"
