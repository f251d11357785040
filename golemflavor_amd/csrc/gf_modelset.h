// gf_modelset.h -- a set of models on one device that share ndim and mode, as the ensemble sampler (gf_sampler_host.hip: one model for
// every chain, or one per chain) and the cube runs (gf_cube_runs.hip: one per run) hand them to their kernels: per-model device
// arrays of the constants, the BSM, prior, binned and likelihood tables, and the one likelihood every model of the set carries.
// Host code only (gf_modelset.hip).
#pragma once
#include <vector>

#include "gf_internal.h"
#include "gf_device.hpp"                // the kernels' MODE_*

struct GfModelSet {
    std::vector<gf_model*> models;      // the models outlive the set; models[0]'s stream carries the set's transfers and its user's launches
    hipStream_t stream = nullptr;
    int device = 0, cus = 256;
    int ndim = 0, mode = 0;             // of every model
    int nbins_max = 0;                  // largest nbins over the models (BSM); sizes the lane-group buffers
    int kind = GF_LLH_FLUX;             // the GfLikelihood every model carries: all of a set do, or none
    // model 0 as create found it (its stream never changes)
    const GfCommon* c = nullptr;        // its constants (host)
    const GfBsm* tb = nullptr;          // its BSM table (device)
    const double* ptab = nullptr;       // its prior table (device)
    // device arrays, one entry per model
    GfCommon* d_commons = nullptr;
    const GfBsm** d_tbs = nullptr;
    const double** d_ptabs = nullptr;
    const double** d_btabs = nullptr;   // GF_LLH_BINNED: the binned measurements (a table's address is its model's for good), else null
    const double** d_ttabs = nullptr;   // GF_LLH_TABLE: the tabulated likelihoods and their sides, else null ...
    int32_t* d_tsides = nullptr;
    std::vector<const double*> h_ttabs; // ... and what the two arrays hold (members: they outlive the asynchronous upload)
    std::vector<int32_t> h_tsides;
    // what create examined, for the refusals its callers word: the first model that is missing or differs from model 0 in device, ndim
    // or mode (-1: none), and the GfLikelihood of every model before it
    int differs = -1;
    std::vector<int> carries;
    // gf_modelset_mark: every model's gf_model_likelihood_sets when the set's user began a run that must not change likelihood
    std::vector<uint64_t> marked;
};

// Validates the models against models[0], takes what each carries and uploads the arrays on the set's stream, which is synchronised.
// GF_ERR_INVALID_ARG without a message where the set is refused: models[0] is unusable (ndim stays 0), a model differs (`differs`) or
// the models carry different likelihoods (kind GF_LLH_MIXED, `carries`); GF_ERR_HIP with `who` in the message.  On failure nothing
// stays allocated.
int gf_modelset_create(GfModelSet* set, gf_model* const* models, int nmodels, const char* who);
// A table set's arrays follow its models: a table set on a model since the arrays were written (gf_model_set_table_likelihood moves
// the table when it grows, and may change its side) is uploaded on the set's stream, ahead of what is enqueued next.  The arrays' own
// addresses never change, so a captured graph stays valid; an outgrown table is retired by its model, not freed.  Called with the
// stream idle; `who` names the caller where a model has lost its table.
int gf_modelset_refresh_tables(GfModelSet* set, const char* who);
// The contract every user of a set keeps with models whose likelihood can be set after the set exists.  The set
// reports, its users word the refusals.
// A set's kind is fixed at creation: the first model that now carries another GfLikelihood than the set's (-1: none), and in *now what
// it carries.  Host reads only.
int gf_modelset_kind_differs(const GfModelSet* set, int* now);
// a GfLikelihood as the refusals name it: "a tabulated likelihood", "a binned measurement", "the flux-averaged likelihood"
inline const char* gf_likelihood_name(int kind) { return kind == GF_LLH_TABLE ? "a tabulated likelihood" : kind == GF_LLH_BINNED ? "a binned measurement" : "the flux-averaged likelihood"; }
// A run that has begun does not change likelihood: _mark records every model's count of likelihoods set, _replaced is the first model
// whose count has moved since (-1: none, or never marked) -- a table or measurement written in place, which leaves address and side as
// they were, included.
void gf_modelset_mark(GfModelSet* set);
int gf_modelset_replaced(const GfModelSet* set);
// the device arrays, after the stream has drained
void gf_modelset_free(GfModelSet* set);
// the MODE of the evaluation kernels' instance: the models' mode, MODE_BSM_BINNED or MODE_BSM_TABLE for such a set
inline int gf_modelset_eval_mode(const GfModelSet* set) { return set->kind == GF_LLH_TABLE ? gfdev::MODE_BSM_TABLE : set->kind == GF_LLH_BINNED ? gfdev::MODE_BSM_BINNED : set->mode; }
