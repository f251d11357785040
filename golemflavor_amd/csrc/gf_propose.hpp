// Device pieces shared by the ensemble sampler (gf_sampler.hip) and the nested sampler (gf_nested.hip): the Philox4x32-10
// block behind both samplers' random streams and the evaluation of one proposal with its unitarity verdict.
#pragma once
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"

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
template <int NDIM, int MODE, int LPW>
__device__ __forceinline__ double proposal_lnprob(const GfCommon& c, const GfBsm* tb, const double* ctab,
                                                  const double* ttab, const double* row, int ndim, int& st, int sub,
                                                  double* fgrp, unsigned long long& pending)
{
    pending = 0ull;
    double val, fr[3];
    if (MODE == MODE_BSM_GAUSS) {
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
            val = lp + gauss_llh(c, fr);
            if (val != val && st == ST_OK) st = ST_NAN;
        }
    } else {
        eval_walker<NDIM, MODE, 0, false>(c, ctab, row, ndim, val, fr, st);
    }
    return val;
}

}  // namespace
