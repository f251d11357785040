// gf_toys_prior.hpp -- the prior sum of a realisation ensemble's seed points (DESIGN.md sections 6j and 6l): one kernel, instantiated by
// the seeding both ensembles share (gf_toys_common.hip).
#pragma once
#include "gf_cube_runs.hpp"

namespace {

// lp [R][n]: the prior sum of every seed of every scale (blockIdx.y), -inf outside the box; nonunit [R] += the scale's seeds whose
// status is GF_ST_NON_UNITARY.  theta [R][n][ndim], status [R][n]
template <bool BSM>
__global__ __launch_bounds__(GF_BLOCK) void k_toy_prior(const GfCubeRuns a, int n, const double* __restrict__ theta,
                                                        const int32_t* __restrict__ status, double* __restrict__ lp, unsigned int* nonunit)
{
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    const int r = blockIdx.y;
    if (BSM) {
        load_eval_tables(ctab, a.ptabs[r], a.tbs[r], false);
        __syncthreads();
    }
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    bool nu = false;
    if (i < n) {
        const int64_t at = (int64_t)r * n + i;
        const double* row = theta + at * a.ndim;
        double s;
        bool inbox;
        if constexpr (BSM) inbox = lnprior_tab<0>(ctab, row, a.ndim, a.commons[r].prior_const, s);
        else inbox = lnprior<0>(a.commons[r], row, s);
        lp[at] = inbox ? s : -gf_inf();
        nu = status[at] == ST_NON_UNITARY;
    }
    const unsigned long long b = __ballot(nu);
    if ((threadIdx.x & (GF_WAVE - 1)) == 0 && b) atomicAdd(&nonunit[r], (unsigned int)__popcll(b));
}

}  // namespace
