// toys_binned_host.cpp -- TEST INFRASTRUCTURE: the binned score of golemflavor_amd/csrc/gf_toys_binned.hpp with gf_toys.hpp's order and
// best-K list compiled for the host, so that the device selection (gf_toys_binned.hip) can be held to them and they to numpy.  Built by
// tests/toys_binned_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include <cmath>

#include "../../golemflavor_amd/csrc/gf_toys_binned.hpp"

namespace {
// gfdev::log_of_exp (gf_device.hpp) with the host's exp and log, as in toys_host.cpp
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

double score_of(const double* lp, const double* frb, const int32_t* status, int nb, const double* tab, int ntoys, int t, double offset, int i)
{
    return gftoyb::score(gftoyb::seed_lp(lp[i], status[i]), frb + (int64_t)i * 3 * nb, nb, tab, ntoys, t, offset, HostLogOfExp());
}

template <int KM>
void select_km(const double* lp, const double* frb, const int32_t* status, int nseed, int nb, const double* tab, int ntoys, int t, double offset,
               int K, int32_t* index, double* score, int32_t* count)
{
    gftoyb::Best<KM> best;
    best.clear();
    for (int i = 0; i < nseed; ++i) best.offer(score_of(lp, frb, status, nb, tab, ntoys, t, offset, i), i);
    *count = 0;
    for (int j = 0; j < K; ++j) {
        const bool have = best.i[j] != gftoyb::NO_SEED;
        *count += have;
        index[j] = have ? best.i[j] : -1;
        score[j] = best.s[j];
    }
}
}  // namespace

extern "C" {

int toybh_max_starts() { return gftoyb::MAX_STARTS; }
int toybh_chunk() { return gftoyb::CHUNK; }
int toybh_nconst() { return gftoyb::NCONST; }

// lp [nseed], frb [nseed][nb][3], status [nseed]; tab [nb][5][ntoys] = {m[3], mh, k} per bin; scores [ntoys][nseed]
void toybh_scores(const double* lp, const double* frb, const int32_t* status, int nseed, int nb, const double* tab, int ntoys, double offset,
                  double* scores)
{
    for (int t = 0; t < ntoys; ++t)
        for (int i = 0; i < nseed; ++i) scores[(int64_t)t * nseed + i] = score_of(lp, frb, status, nb, tab, ntoys, t, offset, i);
}

// out_index, out_score [ntoys][K], out_count [ntoys]; 0, or 1 for a K outside 1 .. MAX_STARTS
int toybh_select(const double* lp, const double* frb, const int32_t* status, int nseed, int nb, const double* tab, int ntoys, double offset, int K,
                 int32_t* out_index, double* out_score, int32_t* out_count)
{
    if (K < 1 || K > gftoyb::MAX_STARTS) return 1;
    for (int t = 0; t < ntoys; ++t) {
        int32_t* ix = out_index + (int64_t)t * K;
        double* sc = out_score + (int64_t)t * K;
        if (K <= 1) select_km<1>(lp, frb, status, nseed, nb, tab, ntoys, t, offset, K, ix, sc, out_count + t);
        else if (K <= 4) select_km<4>(lp, frb, status, nseed, nb, tab, ntoys, t, offset, K, ix, sc, out_count + t);
        else select_km<gftoyb::MAX_STARTS>(lp, frb, status, nseed, nb, tab, ntoys, t, offset, K, ix, sc, out_count + t);
    }
    return 0;
}

}  // extern "C"

#ifdef TOYS_BINNED_HOST_MAIN
// a stand-alone run for host sanitizers
#include <cstdio>
int main()
{
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const int nseed = 8, nb = 2, ntoys = 2;
    const double lp[nseed] = {-1.0, -2.0, -1.0, -inf, nan, -0.5, -0.5, -3.0};
    double frb[nseed * nb * 3];
    for (int i = 0; i < nseed * nb; ++i) { frb[3 * i] = 0.3; frb[3 * i + 1] = 0.3; frb[3 * i + 2] = 0.4; }
    frb[3 * (7 * nb + 1)] = 9.0;                                           // seed 7, bin 1: below the wall
    const int32_t st[nseed] = {0, 0, 0, 1, 3, 2, 0, 0};
    double tab[nb * gftoyb::NCONST * ntoys];
    for (int k = 0; k < nb; ++k)
        for (int t = 0; t < ntoys; ++t) {
            const double c[gftoyb::NCONST] = {0.3, 0.3, 0.4, -50.0, 2.0};
            for (int j = 0; j < gftoyb::NCONST; ++j) tab[gftoyb::const_at(k, j, ntoys, t)] = c[j];
        }
    int32_t index[2 * 16], count[2];
    double score[2 * 16];
    if (toybh_select(lp, frb, st, nseed, nb, tab, ntoys, 0.0, 16, index, score, count)) return 1;
    std::printf("%d:", count[1]);
    for (int j = 0; j < 16; ++j) std::printf(" %d", index[16 + j]);
    std::printf("\n");
    return count[0] == 4 && count[1] == 4 && index[16] == 6 && index[17] == 0 && index[18] == 2 && index[19] == 1 && index[20] == -1 &&
                   score[16] == -0.5 + (2.0 + 2.0)
               ? 0
               : 1;
}
#endif
