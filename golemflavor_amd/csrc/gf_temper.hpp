// gf_temper.hpp -- the arithmetic of the tempered ensemble sampler that a test restates or a host build
// repeats: the walker's scalar T = lp + beta lnl, the draw and the log-ratio of a replica-exchange round, and the per-step reduction
// of a chain's lnl that the stepping-stone and thermodynamic estimators start from.
//
// Compiles for the device (hipcc: gf_temper.hip) and for the host (tests/temper/temper_host.cpp, g++ with contraction off).  As in
// gf_nested_post.hpp, whose operators, exp and lane fold this header uses, every product and sum is rounded once and every sum has ONE
// order, so the two builds give the same bits.  The library never evaluates the reduction on the host.
//
// The orders, over the walkers w = 0 .. nwalkers - 1 of one stored step of one chain:
//   walker sum  lane t (0 <= t < 256) adds its walkers t, t + 256, ... in order from 0.0; the 256 lane sums are folded in groups of 64
//               lanes by the halving tree s[l] += s[l + o], o = 32, 16, ..., 1, and the four group sums are added in order
//               (gfnp::fold_lanes).
//   max         the largest finite lnl, -inf where there is none: exact in any order.
#pragma once
#include "gf_nested_post.hpp"

namespace gftp {

constexpr int MAX_TEMPS = 64;         // rungs of a ladder at most: the rung index has six bits of the swap draw's counter word
constexpr int SERIES = 5;             // doubles per (chain, stored step): count, sum, max, S_up, S_dn

// The walker's scalar under prior * L^beta: lp + beta * lnl, the product rounded, then the sum.  beta == 0 is the prior itself, with NO
// product: a point whose lnl is -inf is a legal sample of the prior chain (0 * -inf would be NaN).  At beta == 1 the product is exact and
// T is the one rounded add of lnprob.  (The operators are gf_nested_post.hpp's, whose bodies switch contraction off: HIP's __dmul_rn and
// __dadd_rn are plain operators that the compiler fuses into one fma once they are inlined.)
GFNP_HD double temper(double lp, double lnl, double beta)
{
    if (beta == 0.0) return lp;
    return gfnp::add(lp, gfnp::mul(beta, lnl));
}

// ---- a replica-exchange round ------------------------------------------------------------------------------------------------------
// Round r pairs walker w of rung t with walker w of rung t + 1 for the t with t % 2 == r % 2.  Its uniform comes from one Philox4x32-10
// block keyed by the sampler's seed, as a stretch draw's, at
//   counter words (0, 1) = walker word  = gsid * nwalkers + w,   gsid = the stream id of the group's rung-0 chain
//   counter words (2, 3) = step word    = 2^63 | t << 56 | (r mod 2^56)
// A stretch draw's step word is 2 * iteration + half (gf_stretch.hpp): below 2^63 for every iteration < 2^62, so the two kinds of draw
// never share a counter whatever their walker words are.  u = (out[0] + 0.5) / 2^32, in (0, 1).
constexpr uint64_t SWAP_BIT = 1ull << 63;
constexpr int SWAP_RUNG_SHIFT = 56;
GFNP_HD uint64_t swap_step_word(uint64_t round, int t) { return SWAP_BIT | ((uint64_t)t << SWAP_RUNG_SHIFT) | (round & ((1ull << SWAP_RUNG_SHIFT) - 1ull)); }
GFNP_HD uint64_t swap_walker_word(uint64_t gsid, int nwalkers, int w) { return gsid * (uint64_t)nwalkers + (uint64_t)w; }
GFNP_HD uint64_t stretch_step_word(uint64_t iteration, int half) { return 2ull * iteration + (uint64_t)half; }
GFNP_HD double swap_uniform(uint64_t seed, uint64_t walker_word, uint64_t step_word)
{
    uint32_t q[4];
    gfnp::philox((uint32_t)walker_word, (uint32_t)(walker_word >> 32), (uint32_t)step_word, (uint32_t)(step_word >> 32), (uint32_t)seed,
                 (uint32_t)(seed >> 32), q);
    return gfnp::mul(gfnp::add((double)q[0], 0.5), 1.0 / 4294967296.0);
}
// the pair is exchanged iff ln u < (beta_t - beta_t1) (lnl_t1 - lnl_t); a NaN on either side rejects
GFNP_HD double swap_log_ratio(double beta_t, double beta_t1, double lnl_t, double lnl_t1) { return gfnp::mul(gfnp::sub(beta_t, beta_t1), gfnp::sub(lnl_t1, lnl_t)); }
GFNP_HD bool swap_live(double T) { return T > gfnp::neg_inf(); }       // a walker at -inf (or NaN) takes no part and is not counted

// ---- the reduction of one stored step ------------------------------------------------------------------------------------------------
GFNP_HD bool finite(double x) { return x - x == 0.0; }
// a walker's term of S_d = sum_w exp(d (lnl_w - m)), d >= 0, m the step's largest finite lnl: 0 for a walker without a finite lnl
GFNP_HD double series_term(double lnl, double m, double d) { return finite(lnl) ? gfnp::exp_neg(gfnp::mul(d, gfnp::sub(lnl, m))) : 0.0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// the host form of what the device does with a workgroup: lnl [nwalkers] of one step -> out [SERIES]
inline void series_step(const double* lnl, int nwalkers, double d_up, double d_dn, double* out)
{
    double m = gfnp::neg_inf();
    int64_t count = 0;
    for (int w = 0; w < nwalkers; ++w)
        if (finite(lnl[w])) { ++count; m = lnl[w] > m ? lnl[w] : m; }
    double sum[gfnp::LANES], up[gfnp::LANES], dn[gfnp::LANES];
    for (int t = 0; t < gfnp::LANES; ++t) {
        sum[t] = up[t] = dn[t] = 0.0;
        for (int w = t; w < nwalkers; w += gfnp::LANES) {
            sum[t] = gfnp::add(sum[t], finite(lnl[w]) ? lnl[w] : 0.0);
            up[t] = gfnp::add(up[t], series_term(lnl[w], m, d_up));
            dn[t] = gfnp::add(dn[t], series_term(lnl[w], m, d_dn));
        }
    }
    out[0] = (double)count;
    out[1] = gfnp::fold_lanes(sum);
    out[2] = m;
    out[3] = gfnp::fold_lanes(up);
    out[4] = gfnp::fold_lanes(dn);
}
#endif

}  // namespace gftp
