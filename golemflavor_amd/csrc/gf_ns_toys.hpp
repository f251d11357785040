// gf_ns_toys.hpp -- the evidence of a nested-sampling run under other Gaussian measurements: the run's dead
// points and final live set, kept with their log-weights lnw_i = lnL_i + ln dX_i, reweighted to every realisation of an ensemble.
//
// Point i of a run carries lnw_i, its composition fr_i and its unitarity verdict st_i (one propagation under the run's own model);
// none of them depends on the measurement.  With l0_i the Gaussian of the run's own measurement at fr_i and lt_i the same function
// on realisation t's constants (gftoy::gauss, gf_toys.hpp: gauss_llh's operations in its order, log(exp(.)) from the caller),
//   x(t, i) = lnw_i + (lt_i - l0_i)       the difference first, then the sum: a realisation equal to the run's measurement has x = lnw
// and x = -inf for a point that carries no weight: lnw_i = -inf, or one of gf_reweight.hpp's rules (gfrw::classify: l0 not finite,
// status GF_ST_NON_UNITARY, lt NaN or -inf).  Then, over the points i = 0 .. n - 1 in dead(r)'s order,
//   M_t = max_i x(t, i)    e(t, i) = gfnp::weight(x(t, i), M_t)    S_t = sum e    S2_t = sum e e    ess_t = S_t S_t / S2_t
//   kept_t = the points with a finite x
// the sums along gf_nested_post.hpp's tree (leaves of 4096 consecutive points, 256 lanes, its fold), so that a realisation whose
// constants are the run's own reproduces gf_nested_posterior's M, S, S2 and ess bit for bit.  A (run, realisation) without a kept
// point has M = -inf, S = S2 = 0, ess = 0.  ln Z_t = M_t + log(S_t) is formed by the caller with the C library's log.
//
// Compiles for the device (hipcc: gf_ns_toys.hip) and for the host (tests/ns_toys/ns_toys_host.cpp, g++ with contraction off).  The
// library never evaluates the host form.
#pragma once
#include <stdint.h>

#include "gf_nested_post.hpp"
#include "gf_reweight.hpp"
#include "gf_toys.hpp"

#if defined(__HIPCC__)
#define GFNT_HD __host__ __device__ __forceinline__
#else
#define GFNT_HD inline
#endif

namespace gfnt {

// a measurement's constants: GfCommon's bf, gauss_mh and gauss_k (gf_internal_gauss_consts of its smearing).  The likelihood offset
// is the run's model's for its own measurement and for every realisation.
struct Consts { double m[3], mh, k; };

template <class LogOfExp>
GFNT_HD double gauss(const Consts& c, double offset, double f0, double f1, double f2, LogOfExp log_of_exp)
{
    const gftoy::Meas g = {{c.m[0], c.m[1], c.m[2]}, c.mh, c.k, offset};
    return gftoy::gauss(g, f0, f1, f2, log_of_exp);
}

// what of a point's log-weight every realisation sees: -inf where no realisation keeps the point (the rules that do not read lt)
GFNT_HD double base_lnw(double lnw, double l0, int32_t status)
{
    return gfrw::classify(0.0, l0, status) == gfrw::RW_KEPT ? lnw : gfrw::neg_inf();
}

// x(t, i) from base_lnw's value; l0 is finite wherever that is not -inf
GFNT_HD double x_term(double blnw, double l0, double lt)
{
    const int kind = gfrw::classify(lt, l0, 0);
    if (blnw == gfrw::neg_inf() || kind != gfrw::RW_KEPT) return gfrw::neg_inf();
    return gfnp::add(blnw, gfrw::lnw(lt, l0, kind));
}

GFNT_HD bool kept(double x) { return gfrw::finite(x); }

// what follows the sums
GFNT_HD double ess(double S, double S2, int64_t nkept) { return nkept > 0 ? gfnp::kish_ess(S, S2) : 0.0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host form of what the device does with whole workgroups -------------------------------------------------------------------

struct Result { double m, s, s2, ess; int64_t kept; };

// One run under one realisation: lnw [n], fr [n][3], status [n]; `own` the run's measurement, `t` the realisation's.  x [n] (may be
// NULL) receives x(t, i).  n = 0 (a run without points): NaN, ess = 0, kept = 0.
template <class LogOfExp>
inline Result evidence(const double* lnw, const double* fr, const int32_t* status, int64_t n, const Consts& own, const Consts& t, double offset,
                       LogOfExp log_of_exp, double* x_out)
{
    Result r;
    if (n < 1) { r.m = r.s = r.s2 = gfnp::nan(); r.ess = 0.0; r.kept = 0; return r; }
    double* x = x_out ? x_out : new double[n];
    r.m = gfnp::neg_inf();
    r.kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double l0 = gauss(own, offset, fr[3 * i], fr[3 * i + 1], fr[3 * i + 2], log_of_exp);
        const double lt = gauss(t, offset, fr[3 * i], fr[3 * i + 1], fr[3 * i + 2], log_of_exp);
        x[i] = x_term(base_lnw(lnw[i], l0, status[i]), l0, lt);
        r.m = x[i] > r.m ? x[i] : r.m;
        r.kept += kept(x[i]);
    }
    r.s = gfnp::tree_sum(n, [&](int64_t i) { return gfnp::weight(x[i], r.m); });
    r.s2 = gfnp::tree_sum(n, [&](int64_t i) { return gfnp::square(gfnp::weight(x[i], r.m)); });
    r.ess = ess(r.s, r.s2, r.kept);
    if (!x_out) delete[] x;
    return r;
}
#endif

}  // namespace gfnt
