// gf_diag.hpp -- the arithmetic of the convergence diagnostics: a series' mean, its centred form and half
// sums, the autocovariance of one lag, the walker average of a lag, the running sum with Sokal's window, split R-hat.
//
// Compiles for the device (hipcc: gf_diag.hip) and for the host (tests/diag/diag_host.cpp, g++ with contraction off).  Every product
// and every sum is rounded once -- the plain operators with contraction switched off, on both sides --
// and every sum has ONE order, stated here, so the two builds give the same bits.  The library never evaluates this on the host.
//
// The orders:
//   series sum     over i in [lo, hi): partial p (0 <= p < 256) takes i = lo + p, lo + p + 256, ... in order; the 256 partials are
//                  folded by the halving tree part[p] += part[p + s], s = 128, 64, ..., 1.   depth <= ceil(n / 256) + 8
//   autocovariance A(t) = sum_b S_b in order of b, S_b = the products i = 256 b .. 256 b + 255 (i <= n - 1 - t) in order.
//                                                                                             depth <= 256 + ceil(n / 256)
//   walker average the included walkers' values in blocks of 32 walkers (by walker index, excluded ones skipped): a block in
//                  order, then the blocks in order; divided by the number included.           depth <= 32 + ceil(nwalkers / 32)
//   running sum    np.cumsum's: t = 0, 1, 2, ...
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFDG_HD __host__ __device__ __forceinline__
#else
#define GFDG_HD inline
#endif

namespace gfdg {

constexpr int PARTS = 256;        // partials of a series sum
constexpr int LAG_BLOCK = 256;    // products per block of an autocovariance
constexpr int WALKER_BLOCK = 32;  // walkers per block of the walker average
constexpr int MAX_STEPS = 16384;  // a series stays resident in LDS: 128 KiB of the 160

// The device compiler contracts a product and a sum into an fma wherever both carry its `contract` flag, across inlined functions as
// well -- and the __dmul_rn / __dadd_rn of the HIP headers are plain operators that carry it.  So the operators are written here, each
// in a function whose body switches contraction off; division and square root are IEEE-correct on both sides.
#if defined(__clang__)
#define GFDG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GFDG_NO_CONTRACT
#endif
GFDG_HD double add(double a, double b)
{
    GFDG_NO_CONTRACT
    return a + b;
}
GFDG_HD double sub(double a, double b)
{
    GFDG_NO_CONTRACT
    return a - b;
}
GFDG_HD double mul(double a, double b)
{
    GFDG_NO_CONTRACT
    return a * b;
}
GFDG_HD double div(double a, double b)
{
    GFDG_NO_CONTRACT
    return a / b;
}
GFDG_HD double root(double a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}
GFDG_HD double nan() { return __builtin_nan(""); }
GFDG_HD bool finite(double x) { return x - x == 0.0; }

// what a series sum adds up
enum { TERM_VALUE = 0, TERM_CENTRED = 1, TERM_SQUARE = 2 };   // x[i] | x[i] - c | (x[i] - c)^2
template <int TERM>
GFDG_HD double term(double x, double c)
{
    if (TERM == TERM_VALUE) return x;
    const double d = sub(x, c);
    return TERM == TERM_CENTRED ? d : mul(d, d);
}

// partial p of the series sum over i in [lo, hi) of x[i * stride]
template <int TERM>
GFDG_HD double series_partial(const double* x, int64_t stride, int lo, int hi, int p, double c)
{
    double s = 0.0;
    for (int i = lo + p; i < hi; i += PARTS) s = add(s, term<TERM>(x[(int64_t)i * stride], c));
    return s;
}

// A(t) of the centred series y[0 .. n)
GFDG_HD double acov_lag(const double* y, int n, int t)
{
    const int m = n - t;                                   // products i = 0 .. m - 1
    double total = 0.0;
    int b = 0;
    for (; b + 4 * LAG_BLOCK <= m; b += 4 * LAG_BLOCK) {   // four blocks side by side: the order of each, and of the blocks, is unchanged
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        const double* a = y + b;
        for (int j = 0; j < LAG_BLOCK; ++j) {
            s0 = add(s0, mul(a[j], a[j + t]));
            s1 = add(s1, mul(a[j + LAG_BLOCK], a[j + LAG_BLOCK + t]));
            s2 = add(s2, mul(a[j + 2 * LAG_BLOCK], a[j + 2 * LAG_BLOCK + t]));
            s3 = add(s3, mul(a[j + 3 * LAG_BLOCK], a[j + 3 * LAG_BLOCK + t]));
        }
        total = add(add(add(add(total, s0), s1), s2), s3);
    }
    for (; b < m; b += LAG_BLOCK) {
        const int e = m - b < LAG_BLOCK ? m - b : LAG_BLOCK;
        double s = 0.0;
        for (int j = 0; j < e; ++j) s = add(s, mul(y[b + j], y[b + j + t]));
        total = add(total, s);
    }
    return total;
}

// a series is left out of the walker average: a non-finite sample, or A(0) zero (a stuck walker) or not finite
GFDG_HD bool excluded(bool nonfinite, double a0) { return nonfinite || !(a0 > 0.0) || !finite(a0); }

// mean over the included walkers of r[w * stride]; *nincl their number; NaN if there is none
GFDG_HD double walker_average(const double* r, int64_t stride, const int32_t* excl, int64_t excl_stride, int nwalkers, int* nincl)
{
    double total = 0.0;
    int k = 0;
    for (int w0 = 0; w0 < nwalkers; w0 += WALKER_BLOCK) {
        const int w1 = w0 + WALKER_BLOCK < nwalkers ? w0 + WALKER_BLOCK : nwalkers;
        double s = 0.0;
        for (int w = w0; w < w1; ++w)
            if (!excl[(int64_t)w * excl_stride]) { s = add(s, r[(int64_t)w * stride]); ++k; }
        total = add(total, s);
    }
    if (nincl) *nincl = k;
    return k ? div(total, (double)k) : nan();
}

// taus(M) = 2 sum_{t <= M} rho(t) - 1 in np.cumsum's order; the window of mcmc.integrated_time: the first M that is not below
// c taus(M), else the last lag; returns taus(window)
GFDG_HD double sokal_tau(const double* rho, int64_t nlags, double c, int64_t* window)
{
    double cs = 0.0, taus = nan();
    int64_t m = 0;
    for (; m < nlags; ++m) {
        cs = m == 0 ? rho[0] : add(cs, rho[m]);
        taus = sub(mul(2.0, cs), 1.0);
        if (!((double)m < mul(c, taus))) break;
    }
    if (m == nlags) m = nlags - 1;
    *window = m;
    return taus;
}

// The per-series numbers split R-hat is made of, [4]: the first and second half's mean and variance (ddof 1), h = n div 2 samples each
// (odd n: the middle step belongs to neither).  mean_k = m + s_k / h with s_k the half's sum of the centred series, var_k = the
// half's sum of (y - s_k / h)^2 over h - 1.
constexpr int HALF_FIELDS = 4;

// split R-hat of one (chain, column) from its walkers' halves [w * stride + 0 .. 3], excluded walkers skipped, in walker order
GFDG_HD double split_rhat(const double* halves, int64_t stride, const int32_t* excl, int64_t excl_stride, int nwalkers, int n)
{
    const int h = n / 2;
    double sm = 0.0, sv = 0.0;
    int k = 0;
    for (int w = 0; w < nwalkers; ++w) {
        if (excl[(int64_t)w * excl_stride]) continue;
        const double* q = halves + (int64_t)w * stride;
        sm = add(add(sm, q[0]), q[2]);
        sv = add(add(sv, q[1]), q[3]);
        k += 2;
    }
    if (k == 0 || h < 2) return nan();
    const double grand = div(sm, (double)k), W = div(sv, (double)k);
    double sb = 0.0;
    for (int w = 0; w < nwalkers; ++w) {
        if (excl[(int64_t)w * excl_stride]) continue;
        const double* q = halves + (int64_t)w * stride;
        const double d0 = sub(q[0], grand), d1 = sub(q[2], grand);
        sb = add(add(sb, mul(d0, d0)), mul(d1, d1));
    }
    const double b_over_h = div(sb, (double)(k - 1));
    const double num = add(mul(div((double)(h - 1), (double)h), W), b_over_h);
    return root(div(num, W));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host form of what the device does with a whole workgroup -------------------------------------------------------------

// the halving tree over the 256 partials
inline double fold_parts(double* part)
{
    for (int s = PARTS / 2; s > 0; s >>= 1)
        for (int p = 0; p < s; ++p) part[p] = add(part[p], part[p + s]);
    return part[0];
}

template <int TERM>
inline double series_sum(const double* x, int64_t stride, int lo, int hi, double c)
{
    double part[PARTS];
    for (int p = 0; p < PARTS; ++p) part[p] = series_partial<TERM>(x, stride, lo, hi, p, c);
    return fold_parts(part);
}

// One series x[i * stride], i < n: y [n] the centred series, racf [nlags] = A(t) / A(0) (untouched if excluded), halves
// [HALF_FIELDS] (may be NULL); returns excluded
inline bool series_acf(const double* x, int64_t stride, int n, int nlags, double* y, double* racf, double* halves)
{
    bool nonfinite = false;
    for (int i = 0; i < n; ++i) nonfinite = nonfinite || !finite(x[(int64_t)i * stride]);
    const double m = div(series_sum<TERM_VALUE>(x, stride, 0, n, 0.0), (double)n);
    for (int i = 0; i < n; ++i) y[i] = sub(x[(int64_t)i * stride], m);
    if (halves) {
        const int h = n / 2;
        for (int k = 0; k < 2; ++k) {
            const int lo = k ? n - h : 0;
            const double mu = div(series_sum<TERM_VALUE>(y, 1, lo, lo + h, 0.0), (double)h);
            halves[2 * k] = add(m, mu);
            halves[2 * k + 1] = div(series_sum<TERM_SQUARE>(y, 1, lo, lo + h, mu), (double)(h - 1));
        }
    }
    const double a0 = acov_lag(y, n, 0);
    if (excluded(nonfinite, a0)) return true;
    for (int t = 0; t < nlags; ++t) racf[t] = div(acov_lag(y, n, t), a0);
    return false;
}

// One step of the ensemble mean, k_walker_mean's arithmetic (gf_sampler.hip): `stride` = the largest multiple of ndim <= 256 running
// sums over the step's nwalkers x ndim block, folded per column in order, over nwalkers
inline void walker_mean_step(const double* step, int nwalkers, int ndim, double* mean)
{
    const int stride = (256 / ndim) * ndim, n = nwalkers * ndim;
    double part[256];
    for (int t = 0; t < stride; ++t) {
        double acc = 0.0;
        for (int i = t; i < n; i += stride) acc += step[i];
        part[t] = acc;
    }
    for (int d = 0; d < ndim; ++d) {
        double sum = 0.0;
        for (int t = d; t < stride; t += ndim) sum += part[t];
        mean[d] = sum / (double)nwalkers;
    }
}
#endif

}  // namespace gfdg
