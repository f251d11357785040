// gf_temper.hip -- the kernels of the tempered ensemble sampler: chains that sample prior * L^beta, their replica
// exchange, and the reduction of their lnl that the stepping-stone evidence starts from.  One instance per likelihood of a BSM model: the
// flux-averaged Gaussian, the energy-resolved Gaussian and the tabulated flavour-plane likelihood.
//
//   k_lnprior_lnl       lnprior and lnl of a row apart, one model per row block: where the status is OK their rounded sum is lnprob bit
//                       for bit.  The pieces are proposal_lnprob's (gf_propose.hpp); the exact verdict of a row the in-kernel tiers
//                       cannot settle is taken by k_stretch_settle's maximiser variant, then k_pt_finish ends the call.
//   k_stretch_tempered  the stretch half-step of gf_sampler.hip's grid shape (the move itself: gf_stretch.hpp) on the walker's scalar
//                       T = lp + beta lnl (gf_temper.hpp), one model and one beta per chain.  Parking and k_stretch_settle behind it
//                       are the untempered sampler's: the parked row's lnprob slot holds T.
//   k_pt_swap           one replica-exchange round on (lp, lnl) of the current walkers.
//   k_pt_series         lnl of every stored sample, reduced over the walkers of a step in gf_temper.hpp's order.
//
// Kernels and launchers only (gf_temper.h): the tempered sampler's host side and the bulk entry point gf_model_lnprior_lnl[_device] are
// gf_temper_host.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_host.h"
#include "gf_temper.h"
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_propose.hpp"
#include "gf_stretch.hpp"
#include "gf_temper.hpp"

namespace {
using namespace gfdev;

// lnprior and lnl of the row in LDS `row`, and the walker's scalar at `beta`: proposal_lnprob's (gf_propose.hpp) BSM bodies with the sum
// taken apart -- its pieces, its verdict lines, its `pending`; the likelihood stays where each body has it (behind the verdict lines,
// but for the binned one, whose bin loop carries the verdict's tiers).  st is what the bulk kernel gives the row (ST_NAN: lp + lnl is
// NaN).  MODE_BSM_BINNED (one lane per walker only): `ltab` is the model's binned measurement, staged in LDS by the caller.
// MODE_BSM_TABLE: `ltab` is the model's table in global memory and `tside` its side; a hole (lnl = -inf) is a legal point of the box:
// T = -inf at every beta > 0 and T = lp at beta = 0.
template <int NDIM, int MODE, int LPW>
__device__ __forceinline__ double tempered_eval(const GfCommon& c, const GfBsm* tb, const double* ctab, const double* ttab, const double* row,
                                                int ndim, double beta, int& st, int sub, double* fgrp, unsigned long long& pending, double& lp_out,
                                                double& lnl_out, const double* ltab = nullptr, int tside = 0)
{
    static_assert(MODE == MODE_BSM_GAUSS || MODE == MODE_BSM_BINNED || MODE == MODE_BSM_TABLE, "a tempered chain samples a BSM likelihood");
    static_assert(MODE != MODE_BSM_BINNED || LPW == 1, "the binned likelihood runs one lane per point");
    pending = 0ull;
    double lp, fr[3];
    const bool inbox = lnprior_tab<NDIM>(ctab, row, ndim, c.prior_const, lp);
    asm volatile("" : "+v"(lp));       // keeps the prior sum ahead of the bin loop (see k_bsm, gf_bsm.hip)
    double val = -gf_inf();
    st = ST_OUT_OF_PRIOR;
    lp_out = -gf_inf();
    lnl_out = -gf_inf();
    if (inbox) {
        UniAcc acc = {0.0, 0.0, 0ull, 2.0};
        double lnl = 0.0;
        if constexpr (MODE == MODE_BSM_BINNED) lnl = binned_llh<UNI_INLINE>(c, tb, ttab, ltab, row, acc) + c.offset;
        else flux_average<UNI_INLINE, LPW>(c, tb, ttab, row, fr, acc, sub, fgrp);
        st = (acc.clear_max < tb->uni_hi) ? ST_OK : ST_NON_UNITARY;       // tiers 1 and 2 (gf_bsm_device.hpp)
        pending = st == ST_OK ? uni_arbitration_mask(acc.amb, tb) : 0ull;
        if constexpr (MODE == MODE_BSM_GAUSS) lnl = gauss_llh(c, fr);
        if constexpr (MODE == MODE_BSM_TABLE) lnl = gftab::lookup(ltab, tside, fr[0], fr[1]);
        val = gftp::temper(lp, lnl, beta);
        if (lnl != lnl && st == ST_OK) st = ST_NAN;                        // lp is finite in the box: lp + lnl is NaN iff lnl is
        lp_out = lp;
        lnl_out = lnl;
    }
    return val;
}

// the likelihood table of chain / model r as tempered_eval takes it: the binned measurement staged in LDS (the caller syncs), the table's
// address in global memory and its side, or nothing.  The LDS array exists in the binned instances alone: declared in the kernels, even
// at one double, it moves the flux-averaged instances' register figures.
// (The arrays are handed over one by one: the kernels' argument structs taken by reference move the flux-averaged instances' figures too.)
struct LlhTable {
    const double* tab;
    int side;
};
template <int MODE>
__device__ __forceinline__ LlhTable stage_llh_table(const double* const* btabs, const double* const* ttabs, const int32_t* tsides, int r,
                                                    const GfBsm* tb)
{
    if constexpr (MODE == MODE_BSM_BINNED) {
        __shared__ __attribute__((aligned(16))) double btab[GF_BINNED_DOUBLES];
        load_binned_table(btab, btabs[r], tb->nbins);
        return {btab, 0};
    } else if constexpr (MODE == MODE_BSM_TABLE) {
        return {ttabs[r], tsides[r]};
    } else {
        return {nullptr, 0};
    }
}

template <int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK) void k_lnprior_lnl(const GfSplitArgs a)
{
    const int r = blockIdx.y;
    extern __shared__ __attribute__((aligned(16))) double fdyn[];
    double* fgrp = LPW > 1 ? fdyn + (threadIdx.x / LPW) * GF_FGRP_DOUBLES(a.nbins_max, LPW) : nullptr;
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * GF_MAX_DIM];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    const GfCommon& c = a.commons[r];
    const GfBsm* tb = a.tbs[r];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, a.ptabs[r], tb, true);
    const LlhTable lt = stage_llh_table<MODE>(a.btabs, a.ttabs, a.tsides, r, tb);
    __syncthreads();
    const int t = blockIdx.x * GF_BLOCK + threadIdx.x;
    const int k = t / LPW, sub = t % LPW;
    if (k >= a.rows) return;
    const int64_t i = (int64_t)r * a.rows + k;
    const int lane = threadIdx.x & (GF_WAVE - 1);
    double* row = tiles[threadIdx.x / GF_WAVE] + lane * GF_MAX_DIM;
    const double* src = a.theta + i * a.ndim;
    for (int d = 0; d < a.ndim; ++d) row[d] = src[d];
    int st;
    unsigned long long pending;
    double lp, lnl;
    (void)tempered_eval<0, MODE, LPW>(c, tb, ctab, ttab, row, a.ndim, 1.0, st, sub, fgrp, pending, lp, lnl, lt.tab, lt.side);
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    a.lp[i] = lp;
    a.lnl[i] = lnl;
    a.status[i] = st;
    // undecided unitarity: park; k_stretch_settle<Team9, false, true> writes the verdict over the status
    if (pending != 0ull) park_proposal(a.pq, a.pend_rows, i, row, a.ndim, lnl, pending);
}

// the end of a split evaluation: lnl is NaN where the reference would have raised (as lnprob is), and T, where asked for, is the walker's
// scalar at its model's beta -- NaN there too, which k_fix_start turns into -inf and counts
__global__ void k_pt_finish(const GfSplitArgs a, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool bad = a.status[i] == ST_NON_UNITARY;
        if (bad) a.lnl[i] = gf_nan();
        if (a.T) a.T[i] = bad ? gf_nan() : gftp::temper(a.lp[i], a.lnl[i], a.betas[i / a.rows]);
    }
}

// stretch_body (gf_sampler.hip) for the tempered chains: blockIdx.y = chain, so that the chain's constants and its beta are
// block-uniform and come from scalar loads.  flags[2] counts the parked proposals (one count per lane group).
#ifndef GF_STRETCH_WAVES
#define GF_STRETCH_WAVES 2
#endif
template <int NDIM, int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK, GF_STRETCH_WAVES) void k_stretch_tempered(const StretchArgs s, const double* __restrict__ betas)
{
    const int chain = blockIdx.y;
    const int t = blockIdx.x * GF_BLOCK + threadIdx.x;
    const int k = t / LPW, sub = t % LPW;
    const bool valid = k < s.nwalkers / 2;
    const GfCommon& c = s.commons[chain];
    const GfBsm* __restrict__ tb = s.tbs[chain];
    const double beta = betas[chain];
    extern __shared__ __attribute__((aligned(16))) double fdyn[];    // LPW > 1: per lane group [nbins_max][3] + [LPW]
    double* fgrp = LPW > 1 ? fdyn + (threadIdx.x / LPW) * GF_FGRP_DOUBLES(s.nbins_max, LPW) : nullptr;
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * ND];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, s.ptabs[chain], tb, true);
    const LlhTable lt = stage_llh_table<MODE>(s.btabs, s.ttabs, s.tsides, chain, tb);
    __syncthreads();

    const int ndim = NDIM ? NDIM : c.ndim;
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int wave = threadIdx.x / GF_WAVE;
    double* row = tiles[wave] + lane * ndim;
    const uint64_t iteration = s.state->iteration_base + (uint64_t)s.step_offset;
    const int64_t run_step = s.state->run_step_base + s.step_offset;
    const int thin = s.state->thin;
    const bool store_now = s.state->store != 0 && s.chain != nullptr && (run_step % thin) == 0;
    const int64_t store_index = s.state->store_base + (run_step + thin - 1) / thin;   // stored steps before this one
    const int nhalf = s.nwalkers / 2;
    const uint64_t sid = s.stream_ids ? s.stream_ids[chain] : (uint64_t)chain;
    const uint64_t g = sid * (uint64_t)nhalf + (uint64_t)k;  // walker slot of the chain's random stream: the Philox counter
    if (!valid) return;
    const int w = s.half * nhalf + k;                        // this walker, in the active half
    const int cbase = (1 - s.half) * nhalf;                  // complementary half

    double z, u3;
    int j;
    stretch_draw(s.seed, g, 2 * iteration + s.half, nhalf, s.a, z, j, u3);
    const double* sk = s.pos + ((int64_t)chain * s.nwalkers + w) * ndim;
    const double* cj = s.pos + ((int64_t)chain * s.nwalkers + cbase + j) * ndim;
    stretch_row<NDIM>(row, cj, sk, z, ndim);
    int st;
    unsigned long long pending;
    double lp, lnl;
    const double lnq = tempered_eval<NDIM, MODE, LPW>(c, tb, ctab, ttab, row, ndim, beta, st, sub, fgrp, pending, lp, lnl, lt.tab, lt.side);
    const int64_t wi = (int64_t)chain * s.nwalkers + w;
    const double lnk = s.lnp[wi];
    const double lhs = stretch_lhs(z, u3, ndim);
    if (pending != 0ull) {
        // undecided unitarity, at every beta: park the proposal; k_stretch_settle completes this walker's half-step
        if (sub == 0) {
            park_proposal<true>(s.pq, s.pend_rows, (int64_t)chain * nhalf + k, row, ndim, lnq, pending, lhs);
            atomicAdd(s.flags + 2, 1u);
        }
        return;
    }
    bool accept = lhs > lnk - lnq;                           // false for NaN and for lnq = -inf
    if (st == ST_NON_UNITARY) {                              // the reference raises inside ln_prob here
        accept = false;
        if (sub == 0) atomicAdd(s.flags, 1u);
    }
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    if (accept) {
        double* dst = s.pos + wi * ndim;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            if (!NDIM && d >= ndim) break;
            dst[d] = row[d];
        }
        s.lnp[wi] = lnq;
        s.naccept[wi] += 1u;
    }
    if (store_now) {
        double* dst = s.chain + (((int64_t)chain * s.nstore_cap + store_index) * s.nwalkers + w) * ndim;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            if (!NDIM && d >= ndim) break;
            dst[d] = accept ? row[d] : sk[d];
        }
        if (s.lnp_chain)
            s.lnp_chain[((int64_t)chain * s.nstore_cap + store_index) * s.nwalkers + w] = accept ? lnq : lnk;
    }
}

// one thread per (group, pair of the round, walker)
__global__ __launch_bounds__(GF_BLOCK) void k_pt_swap(const GfSwapArgs a)
{
    const int par = (int)(a.round & 1ull);
    const int npairs = (a.ntemps - par) / 2;                 // t = par, par + 2, ... with t + 1 < ntemps
    const int64_t total = (int64_t)a.ngroups * npairs * a.nwalkers;
    for (int64_t i = (int64_t)blockIdx.x * GF_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * GF_BLOCK) {
        const int w = (int)(i % a.nwalkers);
        const int p = (int)((i / a.nwalkers) % npairs);
        const int g = (int)(i / ((int64_t)a.nwalkers * npairs));
        const int t = 2 * p + par;
        const int ca = g * a.ntemps + t, cb = ca + 1;
        const int64_t ia = (int64_t)ca * a.nwalkers + w, ib = (int64_t)cb * a.nwalkers + w;
        if (!gftp::swap_live(a.T[ia]) || !gftp::swap_live(a.T[ib])) continue;
        const uint64_t gsid = a.stream_ids ? a.stream_ids[g * a.ntemps] : (uint64_t)(g * a.ntemps);
        const double u = gftp::swap_uniform(a.seed, gftp::swap_walker_word(gsid, a.nwalkers, w), gftp::swap_step_word(a.round, t));
        const double ba = a.betas[ca], bb = a.betas[cb];
        atomicAdd(a.counts + 2 * ca, 1u);
        if (!(log(u) < gftp::swap_log_ratio(ba, bb, a.lnl[ia], a.lnl[ib]))) continue;
        atomicAdd(a.counts + 2 * ca + 1, 1u);
        double* pa = a.pos + ia * a.ndim;
        double* pb = a.pos + ib * a.ndim;
        for (int d = 0; d < a.ndim; ++d) { const double x = pa[d]; pa[d] = pb[d]; pb[d] = x; }
        a.T[ia] = gftp::temper(a.lp[ib], a.lnl[ib], ba);
        a.T[ib] = gftp::temper(a.lp[ia], a.lnl[ia], bb);
    }
}

// the fold of 256 lane values in LDS, gfnp::fold_lanes' order; every thread returns the result
__device__ __forceinline__ double fold256(double* s, double v)
{
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if ((t & 63) < o) s[t] = gfnp::add(s[t], s[t + o]);
        __syncthreads();
    }
    return gfnp::add(gfnp::add(gfnp::add(s[0], s[64]), s[128]), s[192]);
}

// one workgroup per (stored step, chain).  Static LDS: 32 KiB of tiles, ctab, the fold's 2 KiB and, in the binned instance, the chain's
// measurement (GF_BINNED_DOUBLES doubles = 2.5 KiB): 37.5 KiB of a workgroup's 64.
template <int MODE>
__global__ __launch_bounds__(GF_BLOCK) void k_pt_series(const GfSeriesArgs a)
{
    static_assert(GF_BLOCK == gfnp::LANES, "the walker sum's lanes are the workgroup's");
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * GF_MAX_DIM];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    __shared__ double red[GF_BLOCK];
    __shared__ unsigned int cnt;
    const int chain = blockIdx.y;
    const int64_t step = blockIdx.x;
    const GfCommon& c = a.commons[chain];
    const GfBsm* tb = a.tbs[chain];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, a.ptabs[chain], tb, true);
    const LlhTable lt = stage_llh_table<MODE>(a.btabs, a.ttabs, a.tsides, chain, tb);
    if (threadIdx.x == 0) cnt = 0u;
    __syncthreads();
    const int lane = threadIdx.x & (GF_WAVE - 1);
    double* row = tiles[threadIdx.x / GF_WAVE] + lane * GF_MAX_DIM;
    const double* src = a.chain + (((int64_t)chain * a.cap + step) * a.nwalkers) * a.ndim;
    const double* tsrc = a.lnp_chain + ((int64_t)chain * a.cap + step) * a.nwalkers;
    double* lnl_out = a.lnl + ((int64_t)chain * a.nstored + step) * a.nwalkers;
    double m = -gf_inf();
    unsigned int mine = 0u;
    for (int w = threadIdx.x; w < a.nwalkers; w += GF_BLOCK) {
        double lnl = -gf_inf();
        if (gftp::swap_live(tsrc[w])) {                      // else: a start position that never moved, outside the support
            for (int d = 0; d < a.ndim; ++d) row[d] = src[(int64_t)w * a.ndim + d];
            int st;
            unsigned long long pending;
            double lp;
            (void)tempered_eval<0, MODE, 1>(c, tb, ctab, ttab, row, a.ndim, 1.0, st, 0, nullptr, pending, lp, lnl, lt.tab, lt.side);
        }
        lnl_out[w] = lnl;
        if (gftp::finite(lnl)) { ++mine; m = lnl > m ? lnl : m; }
    }
    if (mine) atomicAdd(&cnt, mine);
    // the largest finite lnl: exact in any order
    __syncthreads();
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = GF_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + o] ? red[threadIdx.x] : red[threadIdx.x + o];
        __syncthreads();
    }
    m = red[0];
    const double dup = a.d_up[chain], ddn = a.d_dn[chain];
    double sum = 0.0, up = 0.0, dn = 0.0;
    for (int w = threadIdx.x; w < a.nwalkers; w += GF_BLOCK) {
        const double lnl = lnl_out[w];                       // this thread's own store
        sum = gfnp::add(sum, gftp::finite(lnl) ? lnl : 0.0);
        up = gfnp::add(up, gftp::series_term(lnl, m, dup));
        dn = gfnp::add(dn, gftp::series_term(lnl, m, ddn));
    }
    sum = fold256(red, sum);
    up = fold256(red, up);
    dn = fold256(red, dn);
    if (threadIdx.x == 0) {
        double* o = a.out + ((int64_t)chain * a.nstored + step) * gftp::SERIES;
        o[0] = (double)cnt; o[1] = sum; o[2] = m; o[3] = up; o[4] = dn;
    }
}

template <int NDIM, int MODE>
hipError_t launch_tempered_nm(const StretchArgs& a, const double* d_betas, hipStream_t st)
{
    auto go = [&](auto l) {
        constexpr int LPW = decltype(l)::value;
        const size_t lds = LPW > 1 ? (size_t)(GF_BLOCK / LPW) * GF_FGRP_DOUBLES(a.nbins_max, LPW) * sizeof(double) : 0;
        const dim3 grid((unsigned)(((int64_t)(a.nwalkers / 2) * LPW + GF_BLOCK - 1) / GF_BLOCK), a.nchains);
        hipLaunchKernelGGL((k_stretch_tempered<NDIM, MODE, LPW>), grid, dim3(GF_BLOCK), lds, st, a, d_betas);
        return hipGetLastError();
    };
    if constexpr (MODE != MODE_BSM_BINNED) {
        switch (a.lpw) {
        case 2: return go(std::integral_constant<int, 2>());
        case 4: return go(std::integral_constant<int, 4>());
        case 16: return go(std::integral_constant<int, 16>());
        default: break;
        }
    }
    return go(std::integral_constant<int, 1>());
}

// the instance of the likelihood the arguments carry a table for, as gf_launch_stretch: the tabulated one's where ttabs is set, the
// energy-resolved one's where btabs is, else the flux-averaged one's
template <int NDIM>
hipError_t launch_tempered_n(const StretchArgs& a, const double* d_betas, hipStream_t st)
{
    if (a.ttabs) return launch_tempered_nm<NDIM, MODE_BSM_TABLE>(a, d_betas, st);
    if (a.btabs) return launch_tempered_nm<NDIM, MODE_BSM_BINNED>(a, d_betas, st);
    return launch_tempered_nm<NDIM, MODE_BSM_GAUSS>(a, d_betas, st);
}

// the lanes of a split evaluation: the nested sampler's and the maximiser's choices, forced by GF_TEMPER_LPW
const GfLpwRule SPLIT_RULE = {false, 32 * 1024, "GF_TEMPER_LPW"};

template <int MODE>
hipError_t launch_split_m(const GfSplitArgs& a, int nmodels, int lpw, hipStream_t st)
{
    const size_t lds = lpw > 1 ? (size_t)(GF_BLOCK / lpw) * GF_FGRP_DOUBLES(a.nbins_max, lpw) * sizeof(double) : 0;
    const dim3 grid((unsigned)(((int64_t)a.rows * lpw + GF_BLOCK - 1) / GF_BLOCK), nmodels);
    if constexpr (MODE != MODE_BSM_BINNED) {
        switch (lpw) {
        case 4: hipLaunchKernelGGL((k_lnprior_lnl<MODE, 4>), grid, dim3(GF_BLOCK), lds, st, a); return hipGetLastError();
        case 16: hipLaunchKernelGGL((k_lnprior_lnl<MODE, 16>), grid, dim3(GF_BLOCK), lds, st, a); return hipGetLastError();
        default: break;
        }
    }
    hipLaunchKernelGGL((k_lnprior_lnl<MODE, 1>), grid, dim3(GF_BLOCK), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t gf_launch_stretch_tempered(const StretchArgs& a, const double* d_betas, int ndim, hipStream_t st)
{
    switch (ndim) {
    case 7: return launch_tempered_n<7>(a, d_betas, st);
    case 12: return launch_tempered_n<12>(a, d_betas, st);
    default: return launch_tempered_n<0>(a, d_betas, st);
    }
}

hipError_t gf_launch_lnprior_lnl(const GfSplitArgs& a, int nmodels, unsigned int* ctl, const GfStepState* state, int cus, hipStream_t st)
{
    const int64_t n = (int64_t)nmodels * a.rows;
    if (n == 0) return hipSuccess;
    // the energy-resolved likelihood: one lane per row; the tabulated one: the flux-averaged rule, whose bins it splits
    const int lpw = a.btabs ? 1 : lanes_per_walker(MODE_BSM_GAUSS, n, a.nbins_max, cus, SPLIT_RULE);
    hipError_t e = a.ttabs ? launch_split_m<MODE_BSM_TABLE>(a, nmodels, lpw, st)
                 : a.btabs ? launch_split_m<MODE_BSM_BINNED>(a, nmodels, lpw, st)
                           : launch_split_m<MODE_BSM_GAUSS>(a, nmodels, lpw, st);
    if (e != hipSuccess) return e;
    // the parked rows' exact verdict: row t of model t / rows, as the maximiser's candidates (gf_simplex.hip)
    GfSettleArgs sa = {};
    sa.state = state; sa.pq = a.pq; sa.pend_rows = a.pend_rows; sa.ctl = ctl;
    sa.nchains = nmodels; sa.nwalkers = 2 * a.rows; sa.ndim = a.ndim; sa.commons = a.commons; sa.tbs = a.tbs; sa.multi = 1;
    sa.sx_lnq = a.lnl; sa.sx_status = a.status;
    e = gf_launch_simplex_settle(sa, cus, st);
    if (e != hipSuccess) return e;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_pt_finish, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, a, n);
    return hipGetLastError();
}

hipError_t gf_launch_pt_swap(const GfSwapArgs& a, hipStream_t st)
{
    const int64_t total = (int64_t)a.ngroups * (a.ntemps / 2) * a.nwalkers;
    if (total == 0) return hipSuccess;
    const int64_t blocks = (total + GF_BLOCK - 1) / GF_BLOCK;
    hipLaunchKernelGGL(k_pt_swap, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(GF_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t gf_launch_pt_series(const GfSeriesArgs& a, int nchains, hipStream_t st)
{
    if (a.nstored == 0) return hipSuccess;
    const dim3 grid((unsigned)a.nstored, (unsigned)nchains);
    if (a.ttabs) hipLaunchKernelGGL(k_pt_series<MODE_BSM_TABLE>, grid, dim3(GF_BLOCK), 0, st, a);
    else if (a.btabs) hipLaunchKernelGGL(k_pt_series<MODE_BSM_BINNED>, grid, dim3(GF_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(k_pt_series<MODE_BSM_GAUSS>, grid, dim3(GF_BLOCK), 0, st, a);
    return hipGetLastError();
}
