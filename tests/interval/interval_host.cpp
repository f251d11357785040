// interval_host.cpp -- TEST INFRASTRUCTURE: the column interval of golemflavor_amd/csrc/gf_interval.hpp compiled for the host, so that
// every operation can be pinned to the reference's goldens and to the numpy restatement without a device.  Built by
// tests/interval_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../golemflavor_amd/csrc/gf_interval.hpp"

extern "C" {

// one column x[n] in any order; pct [npct]; low, up, status [npct]; center, nbins, nunique scalars.  -1: invalid arguments.
// Returns the column's base status (1: a NaN or an infinity, nothing evaluated).
int ivh_column(const double* x, int64_t n, const double* pct, int npct, double* low, double* up, int32_t* status, double* center, int64_t* nbins,
               int64_t* nunique)
{
    if (!x || n < 1 || !pct || npct < 1 || npct > gfiv::MAX_PERCENTILES || !low || !up || !status || !center || !nbins || !nunique) return -1;
    for (int k = 0; k < npct; ++k)
        if (!(pct[k] > 0.0 && pct[k] <= 100.0)) return -1;
    std::vector<double> s(x, x + n);
    bool ok = true;
    for (double v : s) ok = ok && gfiv::finite(v);
    if (!ok) {
        for (int k = 0; k < npct; ++k) { low[k] = up[k] = gfiv::nan(); status[k] = gfiv::ST_NONFINITE; }
        *center = gfiv::nan();
        *nbins = *nunique = -1;
        return gfiv::ST_NONFINITE;
    }
    std::sort(s.begin(), s.end());
    return gfiv::column(s.data(), n, std::pow((double)n, -1. / 3), pct, npct, low, up, status, center, nbins, nunique);
}

}  // extern "C"

#ifdef INTERVAL_HOST_MAIN
// a stand-alone run for host sanitizers: seeded columns through ivh_column; prints the results
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    const int64_t nmax = argc > 1 ? std::atoll(argv[1]) : 5000;
    uint64_t state = 88172645463325252ull;
    auto uniform = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    const double pct[3] = {90., 68., 100.};
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)257, nmax}) {
        std::vector<double> x((size_t)n);
        for (auto& v : x) v = std::floor(40.0 * (uniform() + uniform() + uniform() - 1.5)) / 10.0;
        double low[3], up[3], center;
        int32_t st[3];
        int64_t nb, nu;
        const int rc = ivh_column(x.data(), n, pct, 3, low, up, st, &center, &nb, &nu);
        std::printf("n %lld rc %d nbins %lld nunique %lld center %.17g [%.17g, %.17g] status %d %d %d\n", (long long)n, rc, (long long)nb, (long long)nu,
                    center, low[1], up[1], st[0], st[1], st[2]);
        if (rc < 0) return 1;
    }
    return 0;
}
#endif
