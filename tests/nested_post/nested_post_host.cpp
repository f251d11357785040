// nested_post_host.cpp -- TEST INFRASTRUCTURE: the posterior arithmetic of golemflavor_amd/csrc/gf_nested_post.hpp compiled for the
// host, so that its exp, the order of every sum, the prefix and the resampling can be pinned and bounded without a device.  Built by
// tests/nested_post_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include <vector>

#include "../../golemflavor_amd/csrc/gf_nested_post.hpp"

extern "C" {

void nph_exp(const double* x, int64_t n, double* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gfnp::exp_neg(x[i]);
}

void nph_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { gfnp::philox(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out); }

double nph_offset(uint64_t seed, uint64_t id) { return gfnp::resample_offset(seed, id); }

// one run: lnw [n], theta [n][ndim], fixed [ndim] -> stats [6] = m, S, S2, ess, sum p, sum p^2; e, p, C [n]; mean [ndim]; cov [ndim][ndim].
// -1: invalid arguments or no finite lnw
int nph_posterior(const double* lnw, const double* theta, int64_t n, int ndim, const int32_t* fixed, double* stats, double* e, double* p, double* C,
                  double* mean, double* cov)
{
    if (!lnw || !theta || n < 1 || ndim < 1 || ndim > gfnp::MAX_DIM || !fixed || !stats || !e || !p || !C || !mean || !cov) return -1;
    bool any = false;
    for (int64_t i = 0; i < n; ++i) any = any || lnw[i] > gfnp::neg_inf();
    if (!any) return -1;
    const gfnp::Summary r = gfnp::posterior(lnw, theta, n, ndim, fixed, e, p, C, mean, cov);
    stats[0] = r.m; stats[1] = r.S; stats[2] = r.S2; stats[3] = r.ess; stats[4] = r.sp; stats[5] = r.sp2;
    return 0;
}

// index [N] of the rows k = 0 .. N - 1 from the prefix C [n] and the offset u
int nph_resample(const double* C, int64_t n, int64_t N, double u, int64_t* index)
{
    if (!C || n < 1 || N < 1 || !index) return -1;
    for (int64_t k = 0; k < N; ++k) index[k] = gfnp::resample_index(C, n, gfnp::resample_t(k, u, N));
    return 0;
}

}  // extern "C"

#ifdef NESTED_POST_HOST_MAIN
// a stand-alone run for host sanitizers: seeded log-weights with a -inf head and 600 of span through every entry above, at sizes
// around the block and the leaf
#include <cstdio>
int main()
{
    uint64_t state = 88172645463325252ull;
    auto uniform = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    const int ndim = 5;
    const int32_t fixed[ndim] = {0, 0, 1, 0, 0};
    for (int64_t n : {1, 2, 63, 64, 65, 4095, 4096, 4097, 65537}) {
        std::vector<double> lnw(n), th(n * ndim), e(n), p(n), C(n), mean(ndim), cov(ndim * ndim), x(n), ex(n);
        for (int64_t i = 0; i < n; ++i) {
            lnw[i] = i < n / 8 ? gfnp::neg_inf() : -600.0 * uniform();
            for (int c = 0; c < ndim; ++c) th[i * ndim + c] = fixed[c] ? 0.25 : uniform();
            x[i] = -745.2 * uniform();
        }
        lnw[n - 1] = -1.0;
        double stats[6];
        int rc = nph_posterior(lnw.data(), th.data(), n, ndim, fixed, stats, e.data(), p.data(), C.data(), mean.data(), cov.data());
        nph_exp(x.data(), n, ex.data());
        for (int64_t N : {1, 64, 65, 4097}) {
            std::vector<int64_t> idx(N);
            rc |= nph_resample(C.data(), n, N, gfnp::resample_offset(25, (uint64_t)n), idx.data());
            for (int64_t k = 0; k < N; ++k) rc |= idx[k] < 0 || idx[k] >= n;
        }
        std::printf("n %lld rc %d ess %.17g C_last %.17g mean0 %.17g cov00 %.17g cov22 %.17g\n", (long long)n, rc, stats[3], C[n - 1], mean[0], cov[0],
                    cov[2 * ndim + 2]);
        if (rc) return 1;
    }
    return 0;
}
#endif
