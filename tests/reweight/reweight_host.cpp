// reweight_host.cpp -- TEST INFRASTRUCTURE: the log-weight rules of golemflavor_amd/csrc/gf_reweight.hpp compiled for the host, so
// that they can be pinned against numpy without a device.  Built by tests/test_reweight_host.py with g++ (contraction off); nothing in
// the product links it.
#include <stdint.h>

#include "../../golemflavor_amd/csrc/gf_reweight.hpp"

extern "C" {

// lt, l0, status [n] -> lnw, kind [n]; counts [4] by kind (kept, bad base, non-unitary, outside)
void rwh_lnw(const double* lt, const double* l0, const int32_t* status, int64_t n, double* lnw, int32_t* kind, int64_t* counts)
{
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        kind[i] = gfrw::classify(lt[i], l0[i], status[i]);
        lnw[i] = gfrw::lnw(lt[i], l0[i], kind[i]);
        ++counts[kind[i]];
    }
}

uint64_t rwh_resample_id(uint64_t sid, int t) { return gfrw::resample_id(sid, t); }

}  // extern "C"

#ifdef REWEIGHT_HOST_MAIN
// a stand-alone run for host sanitizers
#include <cstdio>
int main()
{
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double v[6] = {-3.5, 0.0, 7.25, -inf, inf, nan};
    double lt[144], l0[144], lnw[144];
    int32_t st[144], kind[144];
    int64_t counts[4];
    int n = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b)
            for (int s = 0; s < 4; ++s) { lt[n] = v[a]; l0[n] = v[b]; st[n] = s; ++n; }
    rwh_lnw(lt, l0, st, n, lnw, kind, counts);
    std::printf("%lld %lld %lld %lld\n", (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3]);
    return counts[0] + counts[1] + counts[2] + counts[3] == n ? 0 : 1;
}
#endif
