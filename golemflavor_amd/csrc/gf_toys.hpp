// gf_toys.hpp -- the shared seeding of a realisation ensemble: the value of a seed point under a mock
// measurement, the order the best seeds are taken in, and the list that keeps the best of a stream of seeds.
//
// A realisation t of a Gaussian measurement is (m_t, smearing_t); seed i of a scale carries its prior sum lp_i (-inf outside the box),
// its composition fr_i and its unitarity verdict, none of which depend on the measurement.  Its value under realisation t is
//   score(t, i) = lp_i + gauss(m_t, fr_i)        the two operations of `val = lp + lnl` (gf_propose.hpp), gauss as gauss_llh forms it
//                                                (gf_device.hpp; restated for a target's constants as rw_mg is in gf_reweight.hip)
// -inf for a seed the reference would have raised on (status GF_ST_NON_UNITARY) and for NaN.  The starts of (scale, t) are the K best
// seeds with a finite score in the total order (score descending, seed index ascending), k_sx_pick's rule (gf_simplex.hip).
//
// Compiles for the device (hipcc: gf_toys.hip) and for the host (tests/toys/toys_host.cpp, g++ with contraction off).  The Gaussian
// takes its log(exp(.)) from the caller: gfdev::log_of_exp on the device, the same steps with the host's exp and log in the host
// build -- the two libraries may differ in the last place inside the subnormal band (logpdf in (-745.14, -708.39)); outside it the
// function is the identity or -inf on both.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFTOY_HD __host__ __device__ __forceinline__
#else
#define GFTOY_HD inline
#endif

namespace gftoy {

constexpr int MAX_STARTS = 16;           // GF_TOY_MAX_STARTS
constexpr int STATUS_NON_UNITARY = 2;    // GF_ST_NON_UNITARY
constexpr int32_t NO_SEED = 0x7fffffff;  // the index of an empty entry: behind every seed in the order

// a realisation's constants: GfCommon's bf, gauss_mh, gauss_k (gf_internal_gauss_consts of its smearing) and offset
struct Meas { double m[3], mh, k, offset; };

GFTOY_HD double neg_inf() { return -__builtin_inf(); }

// gauss_llh (gf_device.hpp) on a realisation's constants: the same operations in the same order
template <class LogOfExp>
GFTOY_HD double gauss(const Meas& g, double f0, double f1, double f2, LogOfExp log_of_exp)
{
    const double d0 = f0 - g.m[0];
    const double d1 = f1 - g.m[1];
    const double d2 = f2 - g.m[2];
    const double r2 = __builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0));
    const double logpdf = __builtin_fma(g.mh, r2, g.k);
    return log_of_exp(logpdf) + g.offset;
}

// the prior sum as the selection reads it: a seed the reference would have raised on has no value under any measurement
GFTOY_HD double seed_lp(double lp, int32_t status) { return status == STATUS_NON_UNITARY ? neg_inf() : lp; }

// lp from seed_lp
template <class LogOfExp>
GFTOY_HD double score(double lp, double f0, double f1, double f2, const Meas& g, LogOfExp log_of_exp)
{
    const double v = lp + gauss(g, f0, f1, f2, log_of_exp);
    return v != v ? neg_inf() : v;
}

// (sa, ia) is ahead of (sb, ib): score descending, then seed index ascending
GFTOY_HD bool ahead(double sa, int32_t ia, double sb, int32_t ib) { return sa > sb || (sa == sb && ia < ib); }

// The KM best of the entries offered so far, in order; empty entries are (-inf, NO_SEED).  KM is a compile-time constant and every
// loop is unrolled, so that on the device the list lives in registers.
template <int KM>
struct Best {
    double s[KM];
    int32_t i[KM];

    GFTOY_HD void clear()
    {
#pragma unroll
        for (int j = 0; j < KM; ++j) { s[j] = neg_inf(); i[j] = NO_SEED; }
    }

    // an entry with a finite (or +inf) score; -inf never enters
    GFTOY_HD void offer(double v, int32_t idx)
    {
        if (!(v > neg_inf()) || !ahead(v, idx, s[KM - 1], i[KM - 1])) return;
        // from the last place up: an entry moves down one place while the new one is ahead of its upper neighbour
#pragma unroll
        for (int j = KM - 1; j >= 0; --j) {
            bool up = false;
            if (j > 0) up = ahead(v, idx, s[j > 0 ? j - 1 : 0], i[j > 0 ? j - 1 : 0]);
            if (up) { s[j] = s[j > 0 ? j - 1 : 0]; i[j] = i[j > 0 ? j - 1 : 0]; }
            else if (ahead(v, idx, s[j], i[j])) { s[j] = v; i[j] = idx; }
        }
    }
};

// seeds per part of the seed range (blockIdx.y of k_toy_select); the parts' lists are merged under the same order, so no result
// depends on it
constexpr int CHUNK = 1024;

}  // namespace gftoy
