// table_host.cpp -- TEST INFRASTRUCTURE: the tabulated flavour-plane likelihood's lookup of golemflavor_amd/csrc/gf_table.hpp compiled for
// the host, so that the device kernels (gf_table.hip, gf_nested.hip, gf_simplex.hip) can be held to it and it to exact rationals.  Built by
// tests/table_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include "../../golemflavor_amd/csrc/gf_table.hpp"

extern "C" {

int tabh_nside_limit() { return GF_TABLE_NSIDE_LIMIT; }
int64_t tabh_node_count(int N) { return gftab::node_count(N); }
int64_t tabh_node_at(int N, int i, int j) { return gftab::node_at(N, i, j); }

// fr [n][3]; out: the cell of every composition (ok 0: a NaN composition, the rest is not written) and its three nodes
void tabh_locate(const double* fr, int64_t n, int N, int32_t* i, int32_t* j, double* fu, double* fv, int32_t* up, int32_t* ok, int64_t* at)
{
    for (int64_t k = 0; k < n; ++k) {
        gftab::Cell c;
        ok[k] = gftab::locate(fr[3 * k], fr[3 * k + 1], N, c) ? 1 : 0;
        if (!ok[k]) continue;
        i[k] = c.i; j[k] = c.j; fu[k] = c.fu; fv[k] = c.fv; up[k] = c.up;
        gftab::nodes(c, N, at + 3 * k);
    }
}

// ln L of every composition fr [n][3] under the table `tab` of side N
void tabh_lookup(const double* tab, int N, const double* fr, int64_t n, double* out)
{
    for (int64_t k = 0; k < n; ++k) out[k] = gftab::lookup(tab, N, fr[3 * k], fr[3 * k + 1]);
}

}  // extern "C"

#ifdef TABLE_HOST_MAIN
// a stand-alone run for host sanitizers: every side up to 9 and the largest, compositions on and beyond every edge
#include <cstdio>
#include <vector>
int main()
{
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double probe[] = {-inf, -1.0, -1e-17, 0.0, 1e-300, 0.25, 1.0 / 3.0, 0.5, 0.75, 1.0 - 1e-16, 1.0, 1.0 + 1e-16, 2.0, inf, nan};
    const int np = sizeof(probe) / sizeof(probe[0]);
    int bad = 0;
    for (int N : {1, 2, 3, 4, 5, 6, 7, 8, 9, 64, GF_TABLE_NSIDE_LIMIT}) {
        std::vector<double> tab((size_t)gftab::node_count(N));
        // linear in (i, j): the interpolation reproduces it
        for (int i = 0; i <= N; ++i)
            for (int j = 0; j <= N - i; ++j) tab[(size_t)gftab::node_at(N, i, j)] = 1.0 + 2.0 * i / N - 3.0 * j / N;
        for (int a = 0; a < np; ++a)
            for (int b = 0; b < np; ++b) {
                const double v = gftab::lookup(tab.data(), N, probe[a], probe[b]);
                const bool want_nan = probe[a] != probe[a] || probe[b] != probe[b];
                if (want_nan != (v != v)) ++bad;
                if (!want_nan && !(v >= -2.0 - 1e-9 && v <= 3.0 + 1e-9)) ++bad;
            }
        tab[0] = -inf;
        if (gftab::lookup(tab.data(), N, 0.0, 0.0) != -inf) ++bad;
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
#endif
