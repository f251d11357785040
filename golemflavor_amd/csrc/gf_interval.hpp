// gf_interval.hpp -- the reference's one 1-D credible interval, "the *percentile* shortest interval around the mode"
// (golemflavor/misc.py:174-213: calc_nbins, calc_bins, most_likely, interval), stated for ONE SORTED column s[0 .. n-1] of finite
// values.
//
// Compiles for the device (hipcc: gf_interval.hip) and for the host (tests/interval/interval_host.cpp, g++ with contraction off).
// Every product, sum and difference is rounded once -- the plain operators in functions whose bodies switch contraction off (the
// __dmul_rn / __dadd_rn of the HIP headers are plain operators that carry the `contract` flag, gf_diag.hpp) -- so both builds give
// the same numbers.  The library never evaluates this on the host.
//
//   percentiles  p25, p75 = np.percentile's default `linear`: virtual index (n - 1) * (q / 100), its floor and the next index (both
//                the last one at the top), gamma = the difference, numpy's _lerp with its t >= 0.5 branch
//   bin count    nbins = floor((s[n-1] - s[0]) / (2 * n**(-1/3) * (p75 - p25))), n**(-1/3) = std::pow((double)n, -1./3) passed in
//   edges        np.linspace(s[0], s[n-1] + 2, nbins + 1): step = delta / nbins, e_b = b * step + start, e_nbins = stop; where the
//                step is zero, (b / nbins) * delta + start
//   counts       np.histogram(arr, edges): searchsorted(s, e_b, 'left') for every edge but the last, 'right' for the last;
//                differences of positions
//   centre       (e_b + e_{b+1}) * 0.5 of the FIRST bin of maximal count
//   start        the first index minimising fl(|s_i - centre|) (np.argmin)
//   walk         misc.py:199-212 step for step, while up - low < fl(fl(p / 100.) * n)
//   unique       1 + the number of i with s[i] != s[i-1]
// Status per (column, percentile): 0 ok; 1 a NaN or an infinity in the column (this library's rule: outputs NaN, nunique -1);
// 2 nbins NaN, infinite or below 1 (the reference raises before the walk); 3 the walk would index s[n] (the reference raises
// IndexError); 4 nbins above MAX_BINS, unsupported.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFIV_HD __host__ __device__ __forceinline__
#else
#define GFIV_HD inline
#endif

namespace gfiv {

constexpr int64_t MAX_BINS = (int64_t)1 << 20;
constexpr int MAX_PERCENTILES = 8;
enum { ST_OK = 0, ST_NONFINITE = 1, ST_NBINS = 2, ST_INDEX = 3, ST_TOO_MANY_BINS = 4 };

#if defined(__clang__)
#define GFIV_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GFIV_NO_CONTRACT
#endif
GFIV_HD double add(double a, double b)
{
    GFIV_NO_CONTRACT
    return a + b;
}
GFIV_HD double sub(double a, double b)
{
    GFIV_NO_CONTRACT
    return a - b;
}
GFIV_HD double mul(double a, double b)
{
    GFIV_NO_CONTRACT
    return a * b;
}
GFIV_HD double div(double a, double b)
{
    GFIV_NO_CONTRACT
    return a / b;
}
GFIV_HD double nan() { return __builtin_nan(""); }
GFIV_HD bool finite(double x) { return x - x == 0.0; }

// np.percentile(s, q) of the sorted column, method `linear` (numpy 2.x _quantile, _get_indexes, _get_gamma, _lerp)
GFIV_HD double percentile(const double* s, int64_t n, double q)
{
    const double vi = mul((double)(n - 1), div(q, 100.0));
    int64_t prev = (int64_t)std::floor(vi), next = prev + 1;
    if (vi >= (double)(n - 1)) prev = next = -1;                     // numpy's index of the last value
    else if (vi < 0.0) prev = next = 0;
    const double t = sub(vi, (double)prev);
    const double a = s[prev < 0 ? n - 1 : prev], b = s[next < 0 ? n - 1 : next];
    const double d = sub(b, a);
    return t >= 0.5 ? sub(b, mul(d, sub(1.0, t))) : add(a, mul(d, t));
}

// calc_nbins' value before anything is asked of it: may be NaN, infinite or below 1.  pw = n**(-1/3)
GFIV_HD double nbins_value(const double* s, int64_t n, double pw)
{
    const double iqr = sub(percentile(s, n, 75.0), percentile(s, n, 25.0));
    return std::floor(div(sub(s[n - 1], s[0]), mul(mul(2.0, pw), iqr)));
}
GFIV_HD int nbins_status(double nb) { return !(nb >= 1.0) || !finite(nb) ? ST_NBINS : nb > (double)MAX_BINS ? ST_TOO_MANY_BINS : ST_OK; }
// the integer reported: -1 for NaN, INT64_MAX for what does not fit
GFIV_HD int64_t nbins_reported(double nb) { return !(nb == nb) ? -1 : nb >= 9.2e18 ? INT64_MAX : nb <= -9.2e18 ? INT64_MIN : (int64_t)nb; }

// np.linspace(s[0], s[n-1] + 2, nbins + 1)
struct Edges {
    double start, stop, delta, step;
    int64_t nb;
};
GFIV_HD Edges edges(const double* s, int64_t n, int64_t nb)
{
    Edges e;
    e.start = s[0];
    e.stop = add(s[n - 1], 2.0);
    e.delta = sub(e.stop, e.start);
    e.step = div(e.delta, (double)nb);
    e.nb = nb;
    return e;
}
GFIV_HD double edge(const Edges& e, int64_t b)
{
    if (b >= e.nb) return e.stop;
    const double y = e.step == 0.0 ? mul(div((double)b, (double)e.nb), e.delta) : mul((double)b, e.step);
    return add(y, e.start);
}

// np.searchsorted(s, v, 'left') / 'right'
GFIV_HD int64_t lower_bound(const double* s, int64_t n, double v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
GFIV_HD int64_t upper_bound(const double* s, int64_t n, double v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (!(v < s[mid])) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// np.histogram's cumulative count at edge b (_search_sorted_inclusive): bin b holds position(b + 1) - position(b) values
GFIV_HD int64_t position(const double* s, int64_t n, const Edges& e, int64_t b)
{
    return b < e.nb ? lower_bound(s, n, edge(e, b)) : upper_bound(s, n, e.stop);
}
GFIV_HD double bin_center(const Edges& e, int64_t b) { return mul(add(edge(e, b), edge(e, b + 1)), 0.5); }

// the first bin of maximal count, bin after bin (the device streams 63 bins per wave round and keeps the first maximum: integers)
GFIV_HD int64_t mode_bin(const double* s, int64_t n, const Edges& e)
{
    int64_t best = 0, best_count = -1, prev = position(s, n, e, 0);
    for (int64_t b = 0; b < e.nb; ++b) {
        const int64_t next = position(s, n, e, b + 1);
        if (next - prev > best_count) { best_count = next - prev; best = b; }
        prev = next;
    }
    return best;
}

// np.argmin(np.abs(s - center)): fl(|s_i - center|) does not increase up to the first s_i >= center and does not decrease from
// there on (rounding is monotone), so the minimum is at that index or the one before, and its first occurrence is found by
// bisection of the falling part
GFIV_HD double distance(const double* s, int64_t i, double center) { return std::fabs(sub(s[i], center)); }
GFIV_HD int64_t start_index(const double* s, int64_t n, double center)
{
    const int64_t i = lower_bound(s, n, center);
    double dmin = i < n ? distance(s, i, center) : distance(s, i - 1, center);
    if (i > 0 && i < n) {
        const double dl = distance(s, i - 1, center);
        if (dl < dmin) dmin = dl;
    }
    int64_t lo = 0, hi = i < n ? i : n;                               // the first j < i with distance <= dmin, else i
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (distance(s, mid, center) <= dmin) hi = mid; else lo = mid + 1;
    }
    return lo < n ? lo : n - 1;
}

// the loop bound of misc.py:199 and its test
GFIV_HD double threshold(double p, int64_t n) { return mul(div(p, 100.0), (double)n); }
GFIV_HD bool reached(int64_t low, int64_t up, double thr) { return !((double)(up - low) < thr); }

// one step of misc.py:200-212: -1 = curr_low -= 1, +1 = curr_up += 1.  s_lm1 = s[low - 1] (unused at low == 0), s_up1 = s[up + 1]
// (unused at up == n - 1).  At low == 0 and up == n - 1 the reference steps to up == n and raises at its return: the caller stops.
GFIV_HD int walk_dir(int64_t low, int64_t up, int64_t n, double s_lm1, double s_low, double s_up, double s_up1)
{
    if (low == 0) return +1;
    if (up == n - 1) return -1;
    const double a = sub(s_up, s_lm1), b = sub(s_up1, s_low);
    if (a < b) return -1;
    if (a > b) return +1;
    return ((up - low) % 2) ? -1 : +1;
}

// ONE walk for thresholds thr[0] <= thr[1] <= ...: (low, up) recorded as each is reached; status ST_INDEX from the first one the walk
// cannot reach without indexing s[n]
GFIV_HD void walk(const double* s, int64_t n, int64_t start, const double* thr, int nthr, int64_t* low_at, int64_t* up_at, int32_t* status)
{
    int64_t low = start, up = start;
    int k = 0;
    for (;;) {
        while (k < nthr && reached(low, up, thr[k])) { low_at[k] = low; up_at[k] = up; status[k] = ST_OK; ++k; }
        if (k == nthr) return;
        if (low == 0 && up == n - 1) break;
        const int d = walk_dir(low, up, n, low > 0 ? s[low - 1] : 0.0, s[low], s[up], up < n - 1 ? s[up + 1] : 0.0);
        if (d < 0) --low; else ++up;
    }
    for (; k < nthr; ++k) { low_at[k] = up_at[k] = -1; status[k] = ST_INDEX; }
}

GFIV_HD int64_t count_unique(const double* s, int64_t n)
{
    int64_t u = 1;
    for (int64_t i = 1; i < n; ++i) u += s[i] != s[i - 1];
    return u;
}

// Everything for one sorted column, sequentially: the host build's entry.  pct [npct] in any order; low, up, status [npct] in the
// same order.  Returns the column's base status (ST_OK, ST_NBINS, ST_TOO_MANY_BINS).
inline int column(const double* s, int64_t n, double pw, const double* pct, int npct, double* low, double* up, int32_t* status, double* center,
                  int64_t* nbins, int64_t* nunique)
{
    *nunique = count_unique(s, n);
    *center = nan();
    for (int k = 0; k < npct; ++k) { low[k] = up[k] = nan(); }
    const double nb = nbins_value(s, n, pw);
    *nbins = nbins_reported(nb);
    const int base = nbins_status(nb);
    if (base != ST_OK) {
        for (int k = 0; k < npct; ++k) status[k] = base;
        return base;
    }
    const Edges e = edges(s, n, (int64_t)nb);
    *center = bin_center(e, mode_bin(s, n, e));
    const int64_t start = start_index(s, n, *center);
    int order[MAX_PERCENTILES];
    double thr[MAX_PERCENTILES];
    int64_t lo[MAX_PERCENTILES], hi[MAX_PERCENTILES];
    int32_t st[MAX_PERCENTILES];
    for (int k = 0; k < npct; ++k) order[k] = k;
    for (int a = 1; a < npct; ++a)                                     // by threshold, stable
        for (int b = a; b > 0 && threshold(pct[order[b]], n) < threshold(pct[order[b - 1]], n); --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
    for (int k = 0; k < npct; ++k) thr[k] = threshold(pct[order[k]], n);
    walk(s, n, start, thr, npct, lo, hi, st);
    for (int k = 0; k < npct; ++k) {
        status[order[k]] = st[k];
        if (st[k] == ST_OK) { low[order[k]] = s[lo[k]]; up[order[k]] = s[hi[k]]; }
    }
    return base;
}

}  // namespace gfiv
