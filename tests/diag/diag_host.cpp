// diag_host.cpp -- TEST INFRASTRUCTURE: the chain diagnostics of golemflavor_amd/csrc/gf_diag.hpp compiled for the host, so that the
// arithmetic and the order of every sum can be pinned and bounded without a device.  Built by tests/diag_harness.py with g++
// (contraction off); nothing in the product links it.
#include <stdint.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../golemflavor_amd/csrc/gf_diag.hpp"

extern "C" {

// one chain [n][nwalkers][ndim]; outputs [ndim] and rho, rho_mean [ndim][maxlag + 1] (maxlag < 0: n - 1), any may be NULL;
// -1: invalid arguments, -2: n above the device's limit.  The series are shared out over `nthreads` threads (results do not depend on it).
int dgh_chain(const double* chain, int64_t n64, int nwalkers, int ndim, double c, int64_t maxlag, double* tau, double* tau_mean, double* rhat,
              int64_t* window, int64_t* window_mean, int32_t* nexcluded, double* rho, double* rho_mean, int nthreads)
{
    if (!chain || n64 < 2 || nwalkers < 1 || ndim < 1 || ndim > 16 || !(c > 0.0) || maxlag >= n64) return -1;
    if (n64 > gfdg::MAX_STEPS) return -2;
    const int n = (int)n64, nlags = (int)(maxlag < 0 ? n64 - 1 : maxlag) + 1;
    const int64_t K = (int64_t)nwalkers * ndim;
    std::vector<double> racf((size_t)K * nlags), halves((size_t)K * gfdg::HALF_FIELDS), mean((size_t)n * ndim);
    std::vector<double> r((size_t)ndim * nlags), rm((size_t)ndim * nlags);
    std::vector<int32_t> excl((size_t)K), excl_mean((size_t)ndim);
    for (int i = 0; i < n; ++i) gfdg::walker_mean_step(chain + (int64_t)i * K, nwalkers, ndim, mean.data() + (size_t)i * ndim);
    std::atomic<int64_t> next(0);
    auto work = [&]() {
        std::vector<double> y((size_t)n);
        for (int64_t s; (s = next.fetch_add(1)) < K + ndim;) {
            if (s < K) {
                excl[s] = gfdg::series_acf(chain + s, K, n, nlags, y.data(), racf.data() + s * nlags, halves.data() + s * gfdg::HALF_FIELDS);
            } else {
                const int d = (int)(s - K);
                excl_mean[d] = gfdg::series_acf(mean.data() + d, ndim, n, nlags, y.data(), rm.data() + (size_t)d * nlags, nullptr);
                if (excl_mean[d])
                    for (int t = 0; t < nlags; ++t) rm[(size_t)d * nlags + t] = gfdg::nan();
            }
        }
    };
    std::vector<std::thread> pool;
    for (int k = 1; k < nthreads; ++k) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    for (int d = 0; d < ndim; ++d) {
        for (int t = 0; t < nlags; ++t)
            r[(size_t)d * nlags + t] = gfdg::walker_average(racf.data() + (size_t)d * nlags + t, (int64_t)ndim * nlags, excl.data() + d, ndim, nwalkers, nullptr);
        int64_t w = 0;
        const double tw = gfdg::sokal_tau(r.data() + (size_t)d * nlags, nlags, c, &w);
        if (tau) tau[d] = tw;
        if (window) window[d] = w;
        const double tm = gfdg::sokal_tau(rm.data() + (size_t)d * nlags, nlags, c, &w);
        if (tau_mean) tau_mean[d] = tm;
        if (window_mean) window_mean[d] = w;
        int nex = 0;
        for (int k = 0; k < nwalkers; ++k) nex += excl[(size_t)k * ndim + d] != 0;
        if (nexcluded) nexcluded[d] = nex;
        if (rhat) rhat[d] = gfdg::split_rhat(halves.data() + (size_t)d * gfdg::HALF_FIELDS, (int64_t)ndim * gfdg::HALF_FIELDS, excl.data() + d, ndim, nwalkers, n);
    }
    if (rho) for (size_t i = 0; i < r.size(); ++i) rho[i] = r[i];
    if (rho_mean) for (size_t i = 0; i < rm.size(); ++i) rho_mean[i] = rm[i];
    return 0;
}

}  // extern "C"

#ifdef DIAG_HOST_MAIN
// a stand-alone run for host sanitizers: a seeded AR(1) chain through dgh_chain; prints the first column's results
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 193, nw = argc > 2 ? std::atoi(argv[2]) : 14, nd = argc > 3 ? std::atoi(argv[3]) : 4;
    std::vector<double> chain((size_t)n * nw * nd), tau(nd), taum(nd), rh(nd), rho((size_t)nd * n), rhom((size_t)nd * n);
    std::vector<int64_t> win(nd), winm(nd);
    std::vector<int32_t> nex(nd);
    uint64_t state = 88172645463325252ull;
    auto uniform = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0 - 0.5; };
    const double phis[4] = {0.0, 0.5, 0.9, 0.7};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < nw * nd; ++k) {
            const double phi = phis[(k % nd) % 4], e = uniform();
            chain[(size_t)i * nw * nd + k] = i ? phi * chain[(size_t)(i - 1) * nw * nd + k] + std::sqrt(1 - phi * phi) * e : e;
        }
    for (int64_t maxlag : {(int64_t)-1, (int64_t)63}) {
        const int rc = dgh_chain(chain.data(), n, nw, nd, 5.0, maxlag, tau.data(), taum.data(), rh.data(), win.data(), winm.data(), nex.data(), rho.data(),
                                 rhom.data(), 3);
        std::printf("maxlag %lld rc %d tau %.17g window %lld tau_mean %.17g window_mean %lld rhat %.17g nexcluded %d\n", (long long)maxlag, rc, tau[0],
                    (long long)win[0], taum[0], (long long)winm[0], rh[0], nex[0]);
        if (rc) return 1;
    }
    return 0;
}
#endif
