// gf_toys_binned.hpp -- the shared seeding of a realisation ensemble under the energy-resolved likelihood: the
// value of a seed point under a mock measurement of every energy bin.
//
// A realisation t of a binned measurement is (m_{t,k}, sigma_{t,k}), k < nb; seed i of a scale carries its prior sum lp_i, its composition
// at every energy bin fr_{i,k} (what k_bsm_bins stores) and its unitarity verdict, none of which depend on the measurement.  Its value is
//   score(t, i) = lp_i + (L + offset),   L = sum_k log_of_exp(fma(mh_{t,k}, r2_k, k_{t,k})),   r2_k = |fr_{i,k} - m_{t,k}|^2
// the operations of binned_llh (gf_bsm_device.hpp) and of k_bsm_binned's `val = lp + (sum + c.offset)` in their order: the sum ascends in
// k from 0.0 with one rounding per add, and a bin at -inf makes it -inf.  -inf for a seed the reference would have raised on and for
// NaN.  The order, the list of the best and the parts of the seed range are gf_toys.hpp's.
//
// Compiles for the device (hipcc: gf_toys_binned.hip) and for the host (tests/toys/toys_binned_host.cpp, g++ with contraction off);
// log_of_exp comes from the caller as in gf_toys.hpp.
#pragma once
#include "gf_toys.hpp"

namespace gftoyb {

using gftoy::ahead;
using gftoy::Best;
using gftoy::CHUNK;
using gftoy::MAX_STARTS;
using gftoy::neg_inf;
using gftoy::NO_SEED;
using gftoy::seed_lp;

constexpr int NCONST = 5;                // GF_BINNED_STRIDE: {m[3], mh, k} of one bin of one realisation

// The realisations' constants are one table [nb][NCONST][T]: a lane that owns realisation t reads bin k's five with loads that are
// contiguous across the lanes.  Element (k, c) of realisation t:
GFTOY_HD int64_t const_at(int k, int c, int64_t T, int64_t t) { return ((int64_t)k * NCONST + c) * T + t; }

// one bin's Gaussian term: gauss_llh's operations on the bin's constants, without the offset
template <class LogOfExp>
GFTOY_HD double bin_term(double f0, double f1, double f2, double m0, double m1, double m2, double mh, double k, LogOfExp log_of_exp)
{
    const double d0 = f0 - m0;
    const double d1 = f1 - m1;
    const double d2 = f2 - m2;
    const double r2 = __builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0));
    return log_of_exp(__builtin_fma(mh, r2, k));
}

// the running sum, one rounding per add: `sum` starts at 0.0 and takes the bins in ascending k
GFTOY_HD double add_term(double sum, double term) { return sum + term; }

// lp from seed_lp, sum over every bin
GFTOY_HD double finish(double lp, double sum, double offset)
{
    const double v = lp + (sum + offset);
    return v != v ? neg_inf() : v;
}

// The whole score of one seed: fr [nb][3] its compositions, `tab` the table of T realisations, t the realisation.
template <class LogOfExp>
GFTOY_HD double score(double lp, const double* fr, int nb, const double* tab, int64_t T, int64_t t, double offset, LogOfExp log_of_exp)
{
    double sum = 0.0;
    for (int k = 0; k < nb; ++k)
        sum = add_term(sum, bin_term(fr[3 * k], fr[3 * k + 1], fr[3 * k + 2], tab[const_at(k, 0, T, t)], tab[const_at(k, 1, T, t)],
                                     tab[const_at(k, 2, T, t)], tab[const_at(k, 3, T, t)], tab[const_at(k, 4, T, t)], log_of_exp));
    return finish(lp, sum, offset);
}

}  // namespace gftoyb
