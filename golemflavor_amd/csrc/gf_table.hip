// gf_table.hip -- the tabulated flavour-plane likelihood in bulk: for every row lnprior + the table's ln L at the row's
// flux-averaged composition, by gf_table.hpp's lookup.  The offset of the model is not added: the table is used as given.
// The verdict is not this kernel's: with a status array the existing propagate launch runs first on the same stream (gf_model.hip
// launch_lnprob), as for a binned model, and this kernel reads what it decided.  The composition it writes is the one it looked up.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_consts.h"
#include "gf_launch.h"
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_table.hpp"

namespace {
using namespace gfdev;

// One lane per row, one wave per tile of 64 rows staged through LDS, grid-stride over the tiles: k_bsm_binned's shape.  The table stays
// in global memory (up to 16 MB at the largest side; a few MB at the sides in use): a row's three nodes are three 8-byte vector loads,
// two of them neighbours, behind the row's bin loop, and the rows of a converged run read the same few cache lines of L2.
// `status` (may be NULL): in, the propagate launch's verdict for the row (OK / NON_UNITARY / NAN; it knows no prior box); out, the
// status the flux-averaged lnprob gives the same row.  `fr` (may be NULL): out, the composition that was looked up; NaN for the rows
// outside the box as the flux-averaged lnprob leaves them.
template <int NDIM>
__global__ __launch_bounds__(GF_BLOCK, NDIM == 0 ? 2 : 3) void k_bsm_table(const GfCommon* __restrict__ cp, const GfBsm* __restrict__ tb,
                                                                            const double* __restrict__ ptab, const double* __restrict__ table,
                                                                            int nside, const double* __restrict__ theta, int layout, int64_t n,
                                                                            double* __restrict__ lnprob, double* __restrict__ fr,
                                                                            int32_t* __restrict__ status)
{
    const GfCommon& c = *cp;                                             // by pointer: see k_bsm
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * (NDIM ? NDIM : GF_MAX_DIM)];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, ptab, tb, true);
    __syncthreads();
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GF_WAVE);
    const int ndim = NDIM ? NDIM : c.ndim;
    double* tile = tiles[wave];
    const int64_t ntiles = (n + GF_WAVE - 1) / GF_WAVE;
    const int64_t stride = (int64_t)gridDim.x * GF_WAVES_PER_BLOCK;
    for (int64_t t = (int64_t)blockIdx.x * GF_WAVES_PER_BLOCK + wave; t < ntiles; t += stride) {
        const int64_t w0 = t * GF_WAVE;
        stage_theta<NDIM>(theta, layout, n, w0, ndim, tile, lane);
        const int64_t i = w0 + lane;
        if (i < n) {
            const double* row = tile + lane * ndim;
            double lp;
            const bool inbox = lnprior_tab<NDIM>(ctab, row, ndim, c.prior_const, lp);
            asm volatile("" : "+v"(lp));       // keeps the prior sum ahead of the bin loop (see k_bsm, gf_bsm.hip)
            double val = -gf_inf();
            double f[3] = {gf_nan(), gf_nan(), gf_nan()};
            int st = ST_OUT_OF_PRIOR;
            if (inbox) {
                st = status ? status[i] : ST_OK;
                UniAcc acc = {0.0, 0.0, 0ull, 2.0};                       // untouched by UNI_NONE
                flux_average<UNI_NONE>(c, tb, ttab, row, f, acc);
                val = lp + gftab::lookup(table, nside, f[0], f[1]);
                if (val != val && st == ST_OK) st = ST_NAN;
                if (st == ST_NON_UNITARY) val = gf_nan();                 // the reference raises here
            }
            lnprob[i] = val;
            if (fr) { fr[3 * i] = f[0]; fr[3 * i + 1] = f[1]; fr[3 * i + 2] = f[2]; }
            if (status) status[i] = st;
        }
        // the next tile overwrites this wave's LDS rows
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int NDIM>
hipError_t launch_table(const GfCommon* d_common, const GfBsm* d_bsm, const double* ptab, const double* table, int nside, const double* theta,
                        int layout, int64_t n, double* lnprob, double* fr, int32_t* status, int cus, hipStream_t s)
{
    const int grid = gf_grid_for(n, GF_BLOCK, cus > 0 ? cus : 256);
    hipLaunchKernelGGL(k_bsm_table<NDIM>, dim3(grid), dim3(GF_BLOCK), 0, s, d_common, d_bsm, ptab, table, nside, theta, layout, n, lnprob, fr, status);
    return hipGetLastError();
}

}  // namespace

hipError_t gf_launch_bsm_table(const GfCommon& c, const GfCommon* d_common, const GfBsm* d_bsm, const double* ptab, const double* table, int nside,
                               const double* theta, int layout, int64_t n, double* lnprob, double* fr, int32_t* status, int cus, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (nside < 1 || nside > GF_TABLE_NSIDE_LIMIT || !d_common || !d_bsm || !ptab || !table || !theta || !lnprob) return hipErrorInvalidValue;
    switch (c.ndim) {
    case 7: return launch_table<7>(d_common, d_bsm, ptab, table, nside, theta, layout, n, lnprob, fr, status, cus, s);
    case 12: return launch_table<12>(d_common, d_bsm, ptab, table, nside, theta, layout, n, lnprob, fr, status, cus, s);
    default: return launch_table<0>(d_common, d_bsm, ptab, table, nside, theta, layout, n, lnprob, fr, status, cus, s);
    }
}
