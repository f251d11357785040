// Device pieces shared by the ensemble sampler (gf_sampler.hip), the nested sampler (gf_nested.hip) and the maximiser
// (gf_simplex.hip): the Philox4x32-10 block behind the random streams, the evaluation of one proposal with its unitarity verdict,
// the parking of an undecided one, and the lanes-per-walker rule of their evaluation kernels (host code: gf_sampler_host.hip takes
// it from here too).
#pragma once
#include <cstdlib>

#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_launch.h"
#include "gf_table.hpp"

namespace {
using namespace gfdev;

__device__ __forceinline__ void philox_block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                             uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(m1 >> 32), c1, k0, 0x96);     // xor of three, one instruction
        const uint32_t n1 = (uint32_t)m1;
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(m0 >> 32), c3, k1, 0x96);
        const uint32_t n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// lnprob of the proposal held in LDS row `row`
// `pending` (out): the energy bins whose unitarity verdict the in-kernel tiers (gf_bsm_device.hpp) cannot settle, 0 = none.
// Such a proposal is not decided here: the half-step kernel parks it and k_stretch_settle (gf_unitarity.hip), next in stream
// order, takes the exact (emulated x87) verdict and completes the walker's update -- so that no sample enters the chain
// that the reference would have died on.
// MODE_BSM_BINNED (a model with a measurement per energy bin; one lane per point only): the same body around
// binned_llh<UNI_INLINE>, which reads the model's table from `btab` (LDS).  The other instances do not see it.
// MODE_BSM_TABLE (a model with a tabulated flavour-plane likelihood): the MODE_BSM_GAUSS body with gf_table.hpp's lookup
// in place of gauss_llh; `btab` is then the model's table in global memory and `tside` its side.  The table is looked up at the
// flux-averaged composition, so the instance splits a point's bins over LPW lanes as the flux-averaged one does: every lane of the
// group holds the group's identical `fr` behind flux_average and makes the same lookup.
template <int NDIM, int MODE, int LPW>
__device__ __forceinline__ double proposal_lnprob(const GfCommon& c, const GfBsm* tb, const double* ctab,
                                                  const double* ttab, const double* row, int ndim, int& st, int sub,
                                                  double* fgrp, unsigned long long& pending, const double* btab = nullptr,
                                                  int tside = 0)
{
    pending = 0ull;
    double val, fr[3];
    if constexpr (MODE == MODE_BSM_TABLE) {
        double lp;
        const bool inbox = lnprior_tab<NDIM>(ctab, row, ndim, c.prior_const, lp);
        asm volatile("" : "+v"(lp));       // keeps the prior sum ahead of the bin loop (see k_bsm, gf_bsm.hip)
        val = -gf_inf();
        st = ST_OUT_OF_PRIOR;
        if (inbox) {
            UniAcc acc = {0.0, 0.0, 0ull, 2.0};
            flux_average<UNI_INLINE, LPW>(c, tb, ttab, row, fr, acc, sub, fgrp);
            st = (acc.clear_max < tb->uni_hi) ? ST_OK : ST_NON_UNITARY;       // tiers 1 and 2 (gf_bsm_device.hpp)
            pending = st == ST_OK ? uni_arbitration_mask(acc.amb, tb) : 0ull;
            val = lp + gftab::lookup(btab, tside, fr[0], fr[1]);
            if (val != val && st == ST_OK) st = ST_NAN;
        }
    } else if constexpr (MODE == MODE_BSM_BINNED || MODE == MODE_BSM_GAUSS) {
        static_assert(MODE != MODE_BSM_BINNED || LPW == 1, "the binned likelihood runs one lane per point");
        double lp;
        const bool inbox = lnprior_tab<NDIM>(ctab, row, ndim, c.prior_const, lp);
        asm volatile("" : "+v"(lp));       // keeps the prior sum ahead of the bin loop (see k_bsm, gf_bsm.hip)
        val = -gf_inf();
        st = ST_OUT_OF_PRIOR;
        if (inbox) {
            UniAcc acc = {0.0, 0.0, 0ull, 2.0};
            // the two BSM instances differ in the likelihood alone; gauss_llh stays behind the verdict lines, where the flux-averaged
            // instance has always had it (moved ahead of them it changes the instances' code)
            double lnl = 0.0;
            if constexpr (MODE == MODE_BSM_BINNED) lnl = binned_llh<UNI_INLINE>(c, tb, ttab, btab, row, acc) + c.offset;
            else flux_average<UNI_INLINE, LPW>(c, tb, ttab, row, fr, acc, sub, fgrp);
            st = (acc.clear_max < tb->uni_hi) ? ST_OK : ST_NON_UNITARY;       // tiers 1 and 2 (gf_bsm_device.hpp)
            pending = st == ST_OK ? uni_arbitration_mask(acc.amb, tb) : 0ull;
            if constexpr (MODE != MODE_BSM_BINNED) lnl = gauss_llh(c, fr);
            val = lp + lnl;
            if (val != val && st == ST_OK) st = ST_NAN;
        }
    } else {
        eval_walker<NDIM, MODE, 0, false>(c, ctab, row, ndim, val, fr, st);
    }
    return val;
}

// A parked proposal's row: theta [GF_MAX_DIM] | lnprob | ln(z^(ndim-1) / u3) (GF_PEND_STRIDE, gf_launch.h).  Writes theta.
__device__ __forceinline__ void park_row(double* dst, const double* row, int ndim)
{
    for (int d = 0; d < ndim; ++d) dst[d] = row[d];
}

// Parks a proposal whose unitarity verdict the in-kernel tiers cannot settle: theta, its lnprob and -- the stretch move, whose settle
// step takes the accept test -- the test's left side `lhs` go to row t of `pend_rows`, {t, undecided bins} onto `pq`, for the
// settle kernel next in stream order
template <bool WITH_LHS = false>
__device__ __forceinline__ void park_proposal(GfArbQueue* pq, double* pend_rows, int64_t t, const double* row, int ndim, double lnq,
                                              unsigned long long pending, double lhs = 0.0)
{
    double* dst = pend_rows + (size_t)t * GF_PEND_STRIDE;
    park_row(dst, row, ndim);
    dst[GF_MAX_DIM] = lnq;
    if (WITH_LHS) dst[GF_MAX_DIM + 1] = lhs;
    const unsigned int at = atomicAdd(&pq->count, 1u);
    if (at < pq->cap) {
        GfArbItem it;
        it.walker = (unsigned long long)t;
        it.mask = pending;
        pq->items[at] = it;
    } else {
        pq->overflow = 1u;                                   // capacity = every proposal of a step: cannot happen
    }
}

// Lanes per walker for a BSM step of `walkers` proposals.  Splitting a walker's bins over L lanes shortens its critical path from
// nbins to nbins / L bin evaluations but repeats the per-walker prologue on every lane and multiplies the waves: small ensembles (a
// latency: one walker's chain on a GPU that is mostly idle) want the widest split, large ones the narrowest that still keeps more
// than one wave on a SIMD.  A cost model instead of a table (round 4; tools/c5_lpw_ab.py, tools/lpw_model_check.py): a lane runs
// P + ceil(nbins / L) B instructions (P ~ 2000: prologue + the tier-2 terms of the chains that need them, B ~ 400 per bin), a SIMD
// with w resident waves gives each an issue slot every max(7, 4 w) cycles, and waves beyond what is resident (three per SIMD by
// registers; two at L = 2, whose 128 group buffers per block take more LDS) queue for another round.  C5's half-step of 65 536
// proposals: L = 2 (one round of two waves per SIMD) -- measured 79 us per half-step against 84 at L = 4, 94 at L = 1, 122 at
// L = 16; ensembles of a few thousand proposals keep 16.  Any choice gives the same bits.
// What a caller's kernels allow: L from {1, 2, 4, 16} (`with2`: the ensemble sampler) or {1, 4, 16}, the LDS its lane-group buffers
// may take beside the tiles, and the environment variable that forces a choice (diagnostics / A-B, read per call)
struct GfLpwRule {
    bool with2;
    size_t lds_cap;
    const char* force_env;
};
inline int lanes_per_walker(int mode, int64_t walkers, int nbins_max, int cus, const GfLpwRule& rule)
{
    if (mode != MODE_BSM_GAUSS || nbins_max < 2) return 1;
    const char* force = gf_internal_env(rule.force_env, 0);
    if (force) { const int f = std::atoi(force); if (f == 1 || (f == 2 && rule.with2) || f == 4 || f == 16) return f; }
    const int64_t simds = (int64_t)(cus > 0 ? cus : 256) * 4;
    int best = 1;
    double best_cost = 0.0;
    for (int lpw : {1, 2, 4, 16}) {
        if (lpw == 2 && !rule.with2) continue;
        const size_t lds = (size_t)(GF_BLOCK / lpw) * GF_FGRP_DOUBLES(nbins_max, lpw) * sizeof(double);
        if (lpw > 1 && lds > rule.lds_cap) continue;                         // group buffers no longer fit beside the tiles
        const int64_t waves = (walkers * lpw + GF_WAVE - 1) / GF_WAVE;
        const int64_t wmax = lpw == 2 ? 2 : 3;
        const int64_t per_simd = (waves + simds - 1) / simds;
        const int64_t w = per_simd < wmax ? per_simd : wmax;
        const int64_t rounds = (waves + simds * wmax - 1) / (simds * wmax);
        const double interval = 4.0 * (double)w > 7.0 ? 4.0 * (double)w : 7.0;
        const double cost = (double)rounds * (2000.0 + 400.0 * (double)((nbins_max + lpw - 1) / lpw)) * interval;
        if (lpw == 1 || cost < best_cost) { best = lpw; best_cost = cost; }
    }
    return best;
}

}  // namespace
