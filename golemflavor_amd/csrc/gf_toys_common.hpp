// gf_toys_common.hpp -- the layer the realisation ensembles share (DESIGN.md sections 6j and 6l), between "the seed points of every
// scale" and "the K best seeds of every (scale, realisation)": the seed set behind both public handles, the tail of a selection and
// the stand-alone selection on host arrays; gf_toys_common.hip implements it.  Two likelihoods plug into it, gf_toys.hip (the
// flux-averaged Gaussian) and gf_toys_binned.hip (the energy-resolved one): each brings its scoring kernels (select, score) and the
// layout of its realisations' constants, nothing else.
#pragma once
#include "gf_cube_runs.hpp"
#include "gf_pool.h"
#include "gf_toys.hpp"

static_assert(gftoy::MAX_STARTS == GF_TOY_MAX_STARTS, "gf_toys.hpp states the public limit");
static_assert(gftoy::STATUS_NON_UNITARY == GF_ST_NON_UNITARY && gftoy::STATUS_NON_UNITARY == ST_NON_UNITARY, "gf_toys.hpp states the public status");

namespace {
// the scores' log(exp(.)) on the device (gf_toys.hpp takes it from the caller)
struct DevLogOfExp {
    __device__ __forceinline__ double operator()(double x) const { return gfdev::log_of_exp(x); }
};
}  // namespace

// The seeds of every scale (one run of a run set, gf_cube_runs.hpp / .hip, each).  Both public handles, gf_toys and gf_toys_binned, point to
// one: the public types stay incomplete, and their files convert with toy_set.
struct ToySeedSet {
    GfCubeRunsHost rs;
    GfCubeRuns a = {};
    int nseed = 0, seeded = 0;
    int nbins = 0;                      // an energy-resolved set's bins, else 0
    double offset = 0.0;                // the scale models' likelihood offset: one for all (checked at create)
    const char* seed_fn = "";           // the public function that draws this set's seeds, for "<who>: after <seed_fn>"
    double* d_u = nullptr;              // [S][M][N]
    double* d_theta = nullptr;          // [S][M][ndim]
    double* d_lnl = nullptr;            // [S][M] the scale models' own lnprob (under the models' measurement)
    double* d_fr = nullptr;             // [S][M][3] the flux-averaged compositions
    double* d_frb = nullptr;            // [S][M][nb][3], an energy-resolved set's (gf_model_bins_on), else NULL
    int32_t* d_st = nullptr;            // [S][M]
    double* d_lp = nullptr;             // [S][M]
    unsigned int* d_nonunit = nullptr;  // [S]
};
inline ToySeedSet* toy_set(void* handle) { return static_cast<ToySeedSet*>(handle); }

// The public functions of a seed set, for the one named `who`.  create: with `binned` the set is of models that carry a binned
// measurement and keeps the compositions at every energy bin.  set_ids: `late` are cube_runs_set_ids' words for a seeded set.  get:
// fr_bins is an energy-resolved set's (else NULL).  ready: GF_OK for a seeded set, its device made current.
GF_LOCAL int toy_seeds_create(void** out, gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed,
                              uint64_t seed, bool binned, const char* who, const char* seed_fn);
GF_LOCAL void toy_seeds_destroy(ToySeedSet* t);
GF_LOCAL int toy_seeds_set_ids(ToySeedSet* t, const uint64_t* ids, const char* late);
GF_LOCAL int toy_seeds_seed(ToySeedSet* t, uint32_t* nonunitary, const char* who);
GF_LOCAL int toy_seeds_get(ToySeedSet* t, int scale, double* cube, double* lnprob, double* lp, double* fr, double* fr_bins, int32_t* status,
                           const char* who);
GF_LOCAL int toy_seeds_ready(const ToySeedSet& t, const char* who);

// What the tail of a selection reads and writes.  A likelihood's argument struct derives from it and adds its own inputs.
struct ToyTail {
    double* part_s;                     // [S][T][nparts][KM]: the best of every part of the seed range, by the likelihood's select kernel
    int32_t* part_i;
    int32_t nparts, K, T, M, N;
    const double* seed_u;               // [S][M][N], NULL: no cube points
    int32_t* out_index;                 // [S][T][K], -1 behind the count
    double* out_score;                  // [S][T][K], -inf behind the count
    int32_t* out_count;                 // [S][T]
    double* out_cube;                   // [S][T][K][N], NaN behind the count (NULL without seed_u)
};
// the likelihood's select kernel <KM> over S scales on `st`, into a.part_s / a.part_i; `a` is the likelihood's own struct
typedef void (*ToySelectLaunch)(const ToyTail& a, int KM, int S, hipStream_t st);

// The selection of S scales' seeds under T realisations on `st`: M, T, K, N, seed_u and the likelihood's device inputs of `a` are the
// caller's; the parts' lists and the outputs are scratch of this call, copied to the host arrays (NULL = skip) before it returns.
GF_LOCAL int toy_select_run(ToyTail& a, int S, hipStream_t st, ToySelectLaunch select, int32_t* index, double* score, int32_t* count,
                            double* cube, const char* who);

// The selection alone, of one seed set on host arrays: a pool stream of `device` borrowed, every block copied into scratch and its
// device address stored in *dev (a pointer of the likelihood's struct `a`), toy_select_run, the stream returned idle.
struct ToyUpload { const void* host; size_t bytes; const void** dev; };
GF_LOCAL int toy_select_alone(int device, ToyTail& a, ToySelectLaunch select, const ToyUpload* blocks, int nblocks, int32_t* index, double* score,
                              int32_t* count, const char* who);
