// ns_toys_host.cpp -- TEST INFRASTRUCTURE: the reweighted evidence of golemflavor_amd/csrc/gf_ns_toys.hpp compiled for the host, so
// that the device kernels (gf_ns_toys.hip) can be held to it and it to Python.  Built by tests/ns_toys_harness.py with g++
// (contraction off); nothing in the product links it.
#include <stdint.h>

#include <cmath>

#include "../../golemflavor_amd/csrc/gf_ns_toys.hpp"

namespace {
// gfdev::log_of_exp (gf_device.hpp) with the host's exp and log: the identity above the underflow wall, the subnormal band's
// quantisation below it, -inf below the band
struct HostLogOfExp {
    double operator()(double x) const
    {
        if (x >= -708.3964185322641) return x;
        const double HI = 744.4400719213812, LO = 4.422444340918698e-14;
        const double t = x + HI;
        const double y = std::exp(t) * (1.0 + LO);
        const double k = std::rint(y);
        if (!(k >= 1.0)) return (x != x) ? x : -__builtin_inf();
        return (std::log(k) - HI) - LO;
    }
};
gfnt::Consts consts(const double* q) { return gfnt::Consts{{q[0], q[1], q[2]}, q[3], q[4]}; }
}  // namespace

extern "C" {

// One run: lnw [n], fr [n][3], status [n]; own [5] = {m[3], mh, k} the run's measurement, meas [ntoys][5] the realisations', offset the
// run's.  m, s, s2, ess, kept [ntoys]; x [ntoys][n] (NULL = skip)
void nth_evidence(const double* lnw, const double* fr, const int32_t* status, int64_t n, const double* own, double offset, const double* meas,
                  int ntoys, double* m, double* s, double* s2, double* ess, int64_t* kept, double* x)
{
    const gfnt::Consts o = consts(own);
    for (int t = 0; t < ntoys; ++t) {
        const gfnt::Result r = gfnt::evidence(lnw, fr, status, n, o, consts(meas + 5 * t), offset, HostLogOfExp(), x ? x + (int64_t)t * n : nullptr);
        m[t] = r.m; s[t] = r.s; s2[t] = r.s2; ess[t] = r.ess; kept[t] = r.kept;
    }
}

// the Gaussian exponent's value under a measurement: gauss [n]
void nth_gauss(const double* fr, int64_t n, const double* meas, double offset, double* out)
{
    const gfnt::Consts g = consts(meas);
    for (int64_t i = 0; i < n; ++i) out[i] = gfnt::gauss(g, offset, fr[3 * i], fr[3 * i + 1], fr[3 * i + 2], HostLogOfExp());
}

// x of one point from its four inputs: the classification rules
double nth_x(double lnw, double l0, double lt, int32_t status) { return gfnt::x_term(gfnt::base_lnw(lnw, l0, status), l0, lt); }

// the tree sum of e [n]
double nth_tree_sum(const double* e, int64_t n) { return gfnp::tree_sum(n, [&](int64_t i) { return e[i]; }); }

double nth_ess(double S, double S2, int64_t kept) { return gfnt::ess(S, S2, kept); }

}  // extern "C"

#ifdef NS_TOYS_HOST_MAIN
// a stand-alone run for host sanitizers
#include <cstdio>
int main()
{
    const int n = 5000;
    static double lnw[n], fr[3 * n], x[n];
    static int32_t st[n];
    for (int i = 0; i < n; ++i) {
        lnw[i] = i % 97 == 0 ? -__builtin_inf() : -1e-3 * (n - i);
        fr[3 * i] = 0.3 + 1e-5 * i; fr[3 * i + 1] = 0.35 - 1e-5 * i; fr[3 * i + 2] = 0.35;
        st[i] = i % 53 == 0 ? 2 : 0;
    }
    const double own[5] = {0.3, 0.35, 0.35, -200.0, 3.0}, meas[10] = {0.3, 0.35, 0.35, -200.0, 3.0, 0.32, 0.33, 0.35, -200.0, 3.0};
    double m[2], s[2], s2[2], ess[2];
    int64_t kept[2];
    nth_evidence(lnw, fr, st, n, own, -320.0, meas, 2, m, s, s2, ess, kept, nullptr);
    nth_evidence(lnw, fr, st, n, own, -320.0, meas, 1, m, s, s2, ess, kept, x);
    std::printf("%lld %.17g %.17g %.17g\n", (long long)kept[0], m[0], s[0], ess[0]);
    int want = 0;
    for (int i = 0; i < n; ++i) want += i % 97 != 0 && i % 53 != 0;
    return kept[0] == want && m[0] == -1e-3 ? 0 : 1;
}
#endif
