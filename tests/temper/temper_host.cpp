// temper_host.cpp -- TEST INFRASTRUCTURE: the arithmetic of golemflavor_amd/csrc/gf_temper.hpp compiled for the host, so that the
// walker's scalar, the word layout of a replica-exchange draw and the per-step reduction of a chain's lnl can be pinned without a
// device.  Built by tests/temper_harness.py with g++ (contraction off); nothing in the product links it.
#include <stdint.h>

#include "../../golemflavor_amd/csrc/gf_temper.hpp"

extern "C" {

double tph_temper(double lp, double lnl, double beta) { return gftp::temper(lp, lnl, beta); }

uint64_t tph_swap_step_word(uint64_t round, int t) { return gftp::swap_step_word(round, t); }
uint64_t tph_swap_walker_word(uint64_t gsid, int nwalkers, int w) { return gftp::swap_walker_word(gsid, nwalkers, w); }
uint64_t tph_stretch_step_word(uint64_t iteration, int half) { return gftp::stretch_step_word(iteration, half); }
double tph_swap_uniform(uint64_t seed, uint64_t walker_word, uint64_t step_word) { return gftp::swap_uniform(seed, walker_word, step_word); }
double tph_swap_log_ratio(double bt, double bt1, double lt, double lt1) { return gftp::swap_log_ratio(bt, bt1, lt, lt1); }
int tph_max_temps(void) { return gftp::MAX_TEMPS; }

// lnl [nsteps][nwalkers] -> out [nsteps][5]
void tph_series(const double* lnl, int64_t nsteps, int nwalkers, double d_up, double d_dn, double* out)
{
    for (int64_t s = 0; s < nsteps; ++s) gftp::series_step(lnl + s * nwalkers, nwalkers, d_up, d_dn, out + s * gftp::SERIES);
}

}  // extern "C"
