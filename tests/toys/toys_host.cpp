// toys_host.cpp -- TEST INFRASTRUCTURE: the score, the order and the best-K list of golemflavor_amd/csrc/gf_toys.hpp compiled for the
// host, so that the device selection (gf_toys.hip) can be held to them and they to numpy.  Built by tests/toys_harness.py with g++
// (contraction off); nothing in the product links it.
#include <stdint.h>

#include <cmath>

#include "../../golemflavor_amd/csrc/gf_toys.hpp"

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

template <int KM>
void select_km(const double* lp, const double* fr, const int32_t* status, int nseed, const gftoy::Meas& g, int K, int32_t* index, double* score,
               int32_t* count)
{
    gftoy::Best<KM> best;
    best.clear();
    for (int i = 0; i < nseed; ++i)
        best.offer(gftoy::score(gftoy::seed_lp(lp[i], status[i]), fr[3 * i], fr[3 * i + 1], fr[3 * i + 2], g, HostLogOfExp()), i);
    *count = 0;
    for (int j = 0; j < K; ++j) {
        const bool have = best.i[j] != gftoy::NO_SEED;
        *count += have;
        index[j] = have ? best.i[j] : -1;
        score[j] = best.s[j];
    }
}
}  // namespace

extern "C" {

int toyh_max_starts() { return gftoy::MAX_STARTS; }
int toyh_chunk() { return gftoy::CHUNK; }

// meas [ntoys][6] = {m[3], mh, k, offset}; scores [ntoys][nseed]
void toyh_scores(const double* lp, const double* fr, const int32_t* status, int nseed, const double* meas, int ntoys, double* scores)
{
    for (int t = 0; t < ntoys; ++t) {
        const double* q = meas + 6 * t;
        const gftoy::Meas g = {{q[0], q[1], q[2]}, q[3], q[4], q[5]};
        for (int i = 0; i < nseed; ++i)
            scores[(int64_t)t * nseed + i] = gftoy::score(gftoy::seed_lp(lp[i], status[i]), fr[3 * i], fr[3 * i + 1], fr[3 * i + 2], g, HostLogOfExp());
    }
}

// out_index, out_score [ntoys][K], out_count [ntoys]; 0, or 1 for a K outside 1 .. MAX_STARTS
int toyh_select(const double* lp, const double* fr, const int32_t* status, int nseed, const double* meas, int ntoys, int K, int32_t* out_index,
                double* out_score, int32_t* out_count)
{
    if (K < 1 || K > gftoy::MAX_STARTS) return 1;
    for (int t = 0; t < ntoys; ++t) {
        const double* q = meas + 6 * t;
        const gftoy::Meas g = {{q[0], q[1], q[2]}, q[3], q[4], q[5]};
        int32_t* ix = out_index + (int64_t)t * K;
        double* sc = out_score + (int64_t)t * K;
        if (K <= 1) select_km<1>(lp, fr, status, nseed, g, K, ix, sc, out_count + t);
        else if (K <= 4) select_km<4>(lp, fr, status, nseed, g, K, ix, sc, out_count + t);
        else select_km<gftoy::MAX_STARTS>(lp, fr, status, nseed, g, K, ix, sc, out_count + t);
    }
    return 0;
}

}  // extern "C"

#ifdef TOYS_HOST_MAIN
// a stand-alone run for host sanitizers
#include <cstdio>
int main()
{
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double lp[8] = {-1.0, -2.0, -1.0, -inf, nan, -0.5, -0.5, -3.0};
    double fr[24];
    for (int i = 0; i < 8; ++i) { fr[3 * i] = 0.3; fr[3 * i + 1] = 0.3; fr[3 * i + 2] = 0.4; }
    const int32_t st[8] = {0, 0, 0, 1, 3, 2, 0, 0};
    const double meas[6] = {0.3, 0.3, 0.4, -50.0, 2.0, 0.0};
    int32_t index[16], count;
    double score[16];
    if (toyh_select(lp, fr, st, 8, meas, 1, 16, index, score, &count)) return 1;
    std::printf("%d:", count);
    for (int j = 0; j < 16; ++j) std::printf(" %d", index[j]);
    std::printf("\n");
    return count == 5 && index[0] == 6 && index[1] == 0 && index[2] == 2 && index[3] == 1 && index[4] == 7 && index[5] == -1 ? 0 : 1;
}
#endif
