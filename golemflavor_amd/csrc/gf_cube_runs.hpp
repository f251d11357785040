// The run set the nested sampler (gf_nested.hip) and the maximiser (gf_simplex.hip) share.  Run r is one posterior (one
// gf_model) over the unit cube of its scanned columns: theta_i = (hi_i - lo_i) u_i + lo_i there (mn.py:35-39, the product and
// the sum each rounded), the run's base value on every other column.  Random numbers: Philox4x32-10, key = seed, counter =
// (run id, iteration word, point, step): a run's result does not depend on the other runs of the launch or on the launch shape.
// The runs' models, their per-model device arrays and the likelihood they carry are a GfModelSet (gf_modelset.h), the layer the
// ensemble sampler builds on too; what is the cube runs' own -- slot map, bases, run ids, step state -- is here.
// This header: the two structs, what a kernel-bearing file needs inlined or instantiated (the device helpers, the launch templates)
// and the declarations of the host layer, which gf_cube_runs.hip defines once, with k_cube_draw.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstddef>
#include <new>
#include <type_traits>
#include <vector>

#include "gf_host.h"
#include "gf_modelset.h"
#include "gf_pool.h"                    // GF_LOCAL
#include "gf_propose.hpp"

// the kernels' view: NsArgs and SxArgs start with it
struct GfCubeRuns {
    const GfCommon* commons;        // [R]
    const GfBsm* const* tbs;        // [R]
    const double* const* ptabs;     // [R]
    const double* const* btabs;     // [R] the runs' binned measurements (gf_consts.h), NULL: the runs have none
    const double* const* ttabs;     // [R] the runs' tabulated likelihoods (gf_table.hpp), NULL: the runs have none
    const int32_t* tsides;          // [R] ... and their sides
    const uint64_t* run_ids;        // [R] Philox counter word 0
    const double* bases;            // [R][GF_MAX_DIM] values of the columns that are not scanned
    GfArbQueue* pq;                 // BSM: parked proposals, capacity = the proposals of one step
    double* pend_rows;              // BSM: [capacity][GF_PEND_STRIDE]
    uint64_t seed;
    int32_t slot[GF_MAX_DIM];       // column -> scanned slot, -1 = fixed
    int32_t nruns, nbins_max, ndim, nscan;     // last: a kernel loads nscan with the counters that follow it (k_sx_pick)
};

// the host's: the runs' models as a set (gf_modelset.h: model r is run r's; its stream carries every launch, its kind picks the
// kernels' instance), and the buffers behind the rest of GfCubeRuns and the settle kernel's arguments
struct GfCubeRunsHost {
    GfModelSet set;
    int initialised = 0;
    double* d_btab_runs = nullptr;      // cube_runs_set_binned_measurements: [nruns][nbins][GF_BINNED_STRIDE], the runs' own tables
    uint64_t* d_run_ids = nullptr;
    double* d_bases = nullptr;
    GfStepState* d_state = nullptr;     // the settle kernel's step state: zeros (no stored chain)
    unsigned int* d_ctl = nullptr;
};

namespace {
using namespace gfdev;

// iteration word of the seeding draws of the maximiser (gf_simplex.hip) and of a realisation ensemble's shared seeding (gf_toys_common.hip):
// the same points for the same run id; the nested sampler's initial draws take 0xFFFFFFFF
constexpr uint32_t SX_SEED_ITER = 0xFFFFFFFEu;

// two uniform doubles in [0, 1), 53 bits each, of counter (run id, it, point, step)
__device__ __forceinline__ void cube_uniform2(const GfCubeRuns& a, int r, uint32_t it, uint32_t point, uint32_t step, double out[2])
{
    uint32_t q[4];
    const uint64_t key = a.seed, id = a.run_ids[r];
    philox_block((uint32_t)id, it, point, step, (uint32_t)key, (uint32_t)(key >> 32) ^ (uint32_t)(id >> 32), q);
    out[0] = ((double)(q[0] >> 5) * 67108864.0 + (double)(q[1] >> 6)) * (1.0 / 9007199254740992.0);
    out[1] = ((double)(q[2] >> 5) * 67108864.0 + (double)(q[3] >> 6)) * (1.0 / 9007199254740992.0);
}

// (hi - lo) u + lo with the product and the sum each rounded, as mn.py:36, the host (NestedSampler.dead, SimplexMaximizer.cube_to_theta,
// gf_nested_post.hpp) and k_cube_to_theta (gf_kernels.hip) form it: plain operators under contract(off).  The HIP headers' __dmul_rn /
// __dadd_rn are operators that carry the contract flag of their own context, and such a pair is fused into one v_fma_f64.
__device__ __forceinline__ double cube_affine_unfused(double span, double u, double lo)
{
#pragma clang fp contract(off)
    const double prod = span * u;
    return prod + lo;
}

// theta of cube point u for run r: cube_affine_unfused on the scanned columns, the run's base value elsewhere.  Every instance of the
// walk and simplex kernels forms it so, and with it theta is the host's and k_cube_to_theta's bit for bit: a stored lnprob is the bulk
// kernel's at the theta the package reports for the same cube point.  (A fused map is one ulp off in a scanned coordinate on up to 40 per
// cent of the draws of a box that does not start at 0, and the stored lnprob then belongs to a neighbouring theta.)
__device__ __forceinline__ void cube_to_theta(const GfCubeRuns& a, const GfCommon& c, int r, const double* u, double* row)
{
    for (int d = 0; d < a.ndim; ++d) {
        const int sl = a.slot[d];
        row[d] = sl >= 0 ? cube_affine_unfused(c.hi[d] - c.lo[d], u[sl], c.lo[d]) : a.bases[r * GF_MAX_DIM + d];
    }
}

// An evaluation kernel's instances: PRIOR_ONLY, SM_GAUSS, BSM_BINNED and BSM_TABLE at one lane per point, BSM at 1, 4 or 16.  `launch` is called
// with std::integral_constant<int, MODE> and <int, LPW>.
template <class Launch>
hipError_t launch_mode_lpw(int mode, int lpw, Launch launch)
{
    using M = std::integral_constant<int, MODE_BSM_GAUSS>;
    switch (mode) {
    case MODE_PRIOR_ONLY: return launch(std::integral_constant<int, MODE_PRIOR_ONLY>(), std::integral_constant<int, 1>());
    case MODE_SM_GAUSS: return launch(std::integral_constant<int, MODE_SM_GAUSS>(), std::integral_constant<int, 1>());
    case MODE_BSM_BINNED: return launch(std::integral_constant<int, MODE_BSM_BINNED>(), std::integral_constant<int, 1>());
    case MODE_BSM_TABLE: return launch(std::integral_constant<int, MODE_BSM_TABLE>(), std::integral_constant<int, 1>());
    default:
        switch (lpw) {
        case 4: return launch(M(), std::integral_constant<int, 4>());
        case 16: return launch(M(), std::integral_constant<int, 16>());
        default: return launch(M(), std::integral_constant<int, 1>());
        }
    }
}

// Its launch: `points` per run (blockIdx.y = run), LPW lanes each, with the lane groups' LDS
template <class Kernel, class Args>
hipError_t launch_points(Kernel kernel, const Args& a, int lpw, int64_t points, hipStream_t st)
{
    const size_t lds = lpw > 1 ? (size_t)(GF_BLOCK / lpw) * GF_FGRP_DOUBLES(a.nbins_max, lpw) * sizeof(double) : 0;
    const dim3 grid((unsigned)((points * lpw + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(kernel, grid, dim3(GF_BLOCK), lds, st, a);
    return hipGetLastError();
}
}  // namespace

// The host layer (gf_cube_runs.hip), compiled once.  Its own device buffers and the arbitration queue come from the driver
// (GF_MEM_DRIVER; DESIGN.md 6, the device cache's table of allocators); the model set's arrays are gf_modelset.hip's.

// The runs' model set (every model shares device, ndim and mode with models[0], and all of them carry a binned measurement / a
// tabulated likelihood, or none; `who` names the call in the error), the slot map of `cols`, and every run's id, base and step
// state: fills `a` but pq and pend_rows.  On failure nothing stays allocated.
GF_LOCAL int cube_runs_create(GfCubeRunsHost& h, GfCubeRuns& a, gf_model* const* models, int nruns, int nscan, const int32_t* cols,
                              const double* bases, uint64_t seed, const char* who);
// the shared buffers and the model set; the stream is synchronised first
GF_LOCAL void cube_runs_free(GfCubeRunsHost& h, GfCubeRuns& a);
// What a run set owes to models whose likelihood can be set after the set exists, for every entry point that
// evaluates (`who`), before it launches or writes anything: the set's kind is fixed at creation -- a model that has since gained a
// table or a measurement is refused; the call that initialises takes the models' tables of now (a binned table's address never
// changes) and marks the models; a run that has begun is refused once a model's likelihood has been set again, in place included.
GF_LOCAL int cube_runs_begin(GfCubeRunsHost& h, const char* who);
// BSM: the arbitration queue for `w` proposals a step, their pend rows and the settle kernel's counters, all empty
GF_LOCAL hipError_t cube_runs_alloc_queue(GfCubeRunsHost& h, GfCubeRuns& a, size_t w);
// the settle kernel's arguments common to both variants: run r is its chain r, `nwalkers` / 2 proposals each
GF_LOCAL void cube_runs_settle_args(const GfCubeRunsHost& h, const GfCubeRuns& a, int nwalkers, GfSettleArgs& sa);
// the Philox streams of the runs; `late` is the error before the first run
GF_LOCAL int cube_runs_set_ids(GfCubeRunsHost& h, const GfCubeRuns& a, const uint64_t* ids, const char* late);
// A measurement of its own for every run: bf [R][3] and smearing [R] replace bf, inv_smear, gauss_c0, gauss_mh and
// gauss_k of d_commons[r], the constants by gf_internal_gauss_consts as gf_model_create derives them -- the run's kernels, which read
// the measurement from d_commons alone, then evaluate what a model compiled with that measurement evaluates.  The models themselves,
// and with them the bulk path of cube_runs_draw, keep theirs.  Flux-averaged Gaussian likelihoods only; `who` names the call.
GF_LOCAL int cube_runs_set_measurements(GfCubeRunsHost& h, const GfCubeRuns& a, const double* bf, const double* smearing, const char* who);
// A binned measurement of its own for every run: fr_bins [R][nbins][3] and sigma [R][nbins] become one device buffer
// [R][nbins][GF_BINNED_STRIDE], built the way gf_model_set_binned_measurement builds a model's table, and d_btabs[r] points into it --
// the run's kernels, which read the binned measurement from a.btabs[r] alone, then evaluate what a model given that measurement
// evaluates.  The models keep theirs.  Binned sets only; `who` names the call.
GF_LOCAL int cube_runs_set_binned_measurements(GfCubeRunsHost& h, const GfCubeRuns& a, int nbins, const double* fr_bins, const double* sigma,
                                               const char* who);
// n uniform cube points per run (k_cube_draw, iteration word `it`: counter (run id, it, point, pair of coordinates)) into u
// [R][n][nscan], mapped to theta [R][n][ndim]: the launch on the set's stream, whose error the caller reads
GF_LOCAL void cube_runs_draw_points(const GfCubeRunsHost& h, const GfCubeRuns& a, uint32_t it, int n, double* u, double* theta);
// ... then every run's lnprob by its model's bulk path with its own unitarity arbitration: lnl [R][n], status [R][n]
GF_LOCAL int cube_runs_draw(const GfCubeRunsHost& h, const GfCubeRuns& a, uint32_t it, int n, double* u, double* theta, double* lnl,
                            int32_t* status);
