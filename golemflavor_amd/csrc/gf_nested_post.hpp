// gf_nested_post.hpp -- the arithmetic of a nested-sampling run's posterior: the weights of its points from
// their log-weights, the Kish effective sample size, the weighted mean and covariance, the inclusive prefix of the weights and the
// systematic resampling that turns the weighted points into equal-weight rows.
//
// Compiles for the device (hipcc: gf_nested_post.hip) and for the host (tests/nested_post/nested_post_host.cpp, g++ with contraction
// off).  Every product, sum and quotient is rounded once -- the plain operators with contraction switched off, fma() where a fused
// operation is meant -- and every sum has ONE order, stated here, so the two builds give the same bits.  The library never evaluates
// this on the host.
//
// The orders, over the points i = 0 .. n - 1 of a run:
//   tree sum    leaves of LEAF = 4096 consecutive points.  In a leaf, lane t (0 <= t < 256) adds its points t, t + 256, ... in order
//               (16 at most); the 256 lane sums are folded in groups of 64 lanes by the halving tree s[l] += s[l + o], o = 32, 16,
//               ..., 1, and the four group sums are added in order.  The leaves of a run are summed the same way: lane t adds the
//               leaves t, t + 256, ... in order, then the same fold.          depth <= 16 + 6 + 3 + ceil(leaves / 256) + 6 + 3
//   prefix      blocks of SCAN_BLOCK = 64 consecutive points.  L_i = the running sum of p inside i's block, in order from the
//               block's first point; T_b = L at the block's last point; P_b = P_{b-1} + T_b in order of b, P_{-1} = 0;
//               C_i = P_{b-1} + L_i.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFNP_HD __host__ __device__ __forceinline__
#else
#define GFNP_HD inline
#endif

namespace gfnp {

constexpr int LANES = 256;            // lanes of a leaf
constexpr int LEAF = 4096;            // points per leaf of a tree sum: 16 per lane
constexpr int SCAN_BLOCK = 64;        // points per block of the prefix
constexpr int MAX_DIM = 16;           // GF_MAX_DIM
constexpr uint32_t RESAMPLE_ITER = 0xFFFFFFFEu;     // iteration word of the resampling offset: no run reaches it, the initial draws use 0xFFFFFFFF

// the operators, each in a function whose body switches contraction off (gf_diag.hpp has the reason)
#if defined(__clang__)
#define GFNP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GFNP_NO_CONTRACT
#endif
GFNP_HD double add(double a, double b)
{
    GFNP_NO_CONTRACT
    return a + b;
}
GFNP_HD double sub(double a, double b)
{
    GFNP_NO_CONTRACT
    return a - b;
}
GFNP_HD double mul(double a, double b)
{
    GFNP_NO_CONTRACT
    return a * b;
}
GFNP_HD double div(double a, double b)
{
    GFNP_NO_CONTRACT
    return a / b;
}
GFNP_HD double nan() { return __builtin_nan(""); }
GFNP_HD double neg_inf() { return -__builtin_inf(); }
GFNP_HD double from_bits(uint64_t u)
{
    double d;
    __builtin_memcpy(&d, &u, sizeof(d));
    return d;
}

// exp(x) for x <= 0, down to the subnormal results of x > -745.2: k = rint(x log2 e), r = x - k ln 2 in two fused steps (the
// published fdlibm split of ln 2: the first product is exact), the Taylor polynomial of degree 13 on |r| <= ln 2 / 2 by Horner's rule
// in fused steps (its remainder is below 5e-18), then the power of two: one exact product for k >= -1021, else an exact product by
// 2^(k + 1000) and ONE rounding product by 2^-1000 into the subnormal range.  -inf and x < -746 give 0, NaN gives NaN; x > 0 is not
// used (a weight is exp(lnw - max lnw)).  The largest error measured against mpmath is in DESIGN.md 6e.
GFNP_HD double exp_neg(double x)
{
    if (x != x) return x;
    if (x < -746.0) return 0.0;
    const double kf = rint(mul(x, 1.44269504088896338700e+00));
    double r = fma(-kf, 6.93147180369123816490e-01, x);
    r = fma(-kf, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;               // 1 / 13!
    p = fma(p, r, 2.08767569878681e-09);             // 1 / 12!
    p = fma(p, r, 2.505210838544172e-08);
    p = fma(p, r, 2.755731922398589e-07);
    p = fma(p, r, 2.7557319223985893e-06);
    p = fma(p, r, 2.48015873015873e-05);
    p = fma(p, r, 0.0001984126984126984);
    p = fma(p, r, 0.001388888888888889);
    p = fma(p, r, 0.008333333333333333);
    p = fma(p, r, 0.041666666666666664);
    p = fma(p, r, 0.16666666666666666);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const int k = (int)kf;
    if (k >= -1021) return mul(p, from_bits((uint64_t)(k + 1023) << 52));
    return mul(mul(p, from_bits((uint64_t)(k + 1000 + 1023) << 52)), from_bits((uint64_t)(1023 - 1000) << 52));
}

// Philox4x32-10 (Salmon et al. 2011), the block gf_propose.hpp's philox_block computes
GFNP_HD void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)m1;
        const uint32_t n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the resampling offset u_r in [0, 1) of the run with id `id` in the sampler seeded `seed`: the first 53-bit uniform (as
// gf_cube_runs.hpp's cube_uniform2) of counter (id, RESAMPLE_ITER, 0, 0)
GFNP_HD double resample_offset(uint64_t seed, uint64_t id)
{
    uint32_t q[4];
    philox((uint32_t)id, RESAMPLE_ITER, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(id >> 32), q);
    return mul(add(mul((double)(q[0] >> 5), 67108864.0), (double)(q[1] >> 6)), 1.0 / 9007199254740992.0);
}

// a scanned column of a point: (hi - lo) u + lo, the product and the sum each rounded (mn.py:35-36, k_cube_to_theta)
GFNP_HD double cube_theta(double lo, double hi, double u) { return add(mul(sub(hi, lo), u), lo); }
// the log-weight of a point of the final live set: (ln X_final - ln nlive) + lnL, as gf_nested_get_dead
GFNP_HD double live_lnw(double lnw0, double lnl) { return add(lnw0, lnl); }

// the terms of the tree sums
GFNP_HD double weight(double lnw, double m) { return lnw == neg_inf() ? 0.0 : exp_neg(sub(lnw, m)); }
GFNP_HD double square(double e) { return mul(e, e); }
GFNP_HD double term_mean(double p, double x) { return mul(p, x); }
GFNP_HD double term_cov(double p, double xa, double ma, double xb, double mb) { return mul(p, mul(sub(xa, ma), sub(xb, mb))); }    // symmetric in a, b

// what follows the sums
GFNP_HD double kish_ess(double S, double S2) { return div(mul(S, S), S2); }
GFNP_HD double cov_factor(double sp, double sp2) { return sub(sp, div(sp2, sp)); }       // np.cov's, aweights = p, ddof = 1

// resampling: t_k = (k + u) / N, the point of row k = the first i with C_i > t_k: np.searchsorted(C, t, side="right").  Where there is
// none (t_k >= C_{n-1}: only within the rounding of 1; (k + u) / N itself rounds to 1 for the largest u) the row takes the last point
// that carries weight, the first i with C_i >= C_{n-1} -- which is np.minimum(., n - 1) unless the run ends in points of zero weight,
// and those are never taken.
GFNP_HD double resample_t(int64_t k, double u, int64_t N) { return div(add((double)k, u), (double)N); }
GFNP_HD int64_t resample_index(const double* C, int64_t n, double t)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo < n) return lo;
    const double top = C[n - 1];
    lo = 0; hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] >= top) hi = mid; else lo = mid + 1;
    }
    return lo;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host form of what the device does with whole workgroups -------------------------------------------------------------------

// the fold of 256 lane sums
inline double fold_lanes(double* s)
{
    for (int g = 0; g < LANES; g += 64)
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) s[g + l] = add(s[g + l], s[g + l + o]);
    return add(add(add(s[0], s[64]), s[128]), s[192]);
}

// the tree sum of term(i), i < n
template <class Term>
inline double tree_sum(int64_t n, Term term)
{
    const int64_t leaves = n > 0 ? (n + LEAF - 1) / LEAF : 1;
    double top[LANES];
    for (int t = 0; t < LANES; ++t) top[t] = 0.0;
    for (int64_t q = 0; q < leaves; ++q) {
        double s[LANES];
        for (int t = 0; t < LANES; ++t) {
            s[t] = 0.0;
            for (int64_t i = q * LEAF + t; i < n && i < (q + 1) * LEAF; i += LANES) s[t] = add(s[t], term(i));
        }
        top[q % LANES] = add(top[q % LANES], fold_lanes(s));
    }
    return fold_lanes(top);
}

// the inclusive prefix C [n] of p [n]
inline void prefix(const double* p, int64_t n, double* C)
{
    double before = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += SCAN_BLOCK) {
        double run = 0.0;
        for (int64_t i = b0; i < n && i < b0 + SCAN_BLOCK; ++i) {
            run = i == b0 ? p[i] : add(run, p[i]);
            C[i] = b0 == 0 ? run : add(before, run);
        }
        before = b0 == 0 ? run : add(before, run);
    }
}

struct Summary {
    double m, S, S2, ess, sp, sp2;
};

// One run: lnw [n], theta [n][ndim], fixed [ndim] (a column every point holds the same value in: its mean is that value and its
// covariances are zero, exactly) -> e, p [n], C [n] (may be NULL), mean [ndim], cov [ndim][ndim].  n >= 1 with a finite lnw.
inline Summary posterior(const double* lnw, const double* theta, int64_t n, int ndim, const int32_t* fixed, double* e, double* p, double* C,
                         double* mean, double* cov)
{
    Summary r;
    r.m = neg_inf();
    for (int64_t i = 0; i < n; ++i) r.m = lnw[i] > r.m ? lnw[i] : r.m;
    for (int64_t i = 0; i < n; ++i) e[i] = weight(lnw[i], r.m);
    r.S = tree_sum(n, [&](int64_t i) { return e[i]; });
    r.S2 = tree_sum(n, [&](int64_t i) { return square(e[i]); });
    r.ess = kish_ess(r.S, r.S2);
    for (int64_t i = 0; i < n; ++i) p[i] = div(e[i], r.S);
    r.sp = tree_sum(n, [&](int64_t i) { return p[i]; });
    r.sp2 = tree_sum(n, [&](int64_t i) { return square(p[i]); });
    for (int c = 0; c < ndim; ++c)
        mean[c] = fixed[c] ? theta[c] : div(tree_sum(n, [&](int64_t i) { return term_mean(p[i], theta[i * ndim + c]); }), r.sp);
    const double fact = cov_factor(r.sp, r.sp2);
    for (int a = 0; a < ndim; ++a)
        for (int b = 0; b < ndim; ++b)
            cov[a * ndim + b] = (fixed[a] || fixed[b]) ? 0.0 : div(tree_sum(n, [&](int64_t i) {
                return term_cov(p[i], theta[i * ndim + a], mean[a], theta[i * ndim + b], mean[b]); }), fact);
    if (C) prefix(p, n, C);
    return r;
}
#endif

}  // namespace gfnp
