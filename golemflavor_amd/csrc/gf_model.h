// gf_model.h -- the model object behind the C ABI's gf_model handle, for the two files that work on its members: gf_model.hip (its
// constants, its stream, its launches) and gf_capi.hip (the host-buffer entry points' staging).  Everybody else goes through
// gf_model_internal, gf_model_constants and the *_on functions of gf_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "gf_consts.h"
#include "gf_pool.h"

struct gf_model {
    GfCommon c;
    GfBsm hb;
    void* d_block = nullptr;     // the model's constant block (from the per-device pool): d_ptab | d_bsm
    GfBsm* d_bsm = nullptr;
    GfCommon* d_common = nullptr;  // device copy of `c` (same block)
    double* d_ptab = nullptr;    // [GF_MAX_DIM][4] = {lo, hi, loc, 1/sigma}: the kernels' LDS constant table
    hipStream_t stream = nullptr;   // created on first use (ensure_stream)
    std::mutex mu;
    int device = 0;
    int cus = 256;
    // staging for the host-buffer entry points (grown on demand, reused across calls)
    int64_t cap = 0;             // rows the device buffers hold
    double* d_theta = nullptr;
    double* d_out = nullptr;     // lnprob [cap] then fr [3 cap]
    int32_t* d_status = nullptr;
    int64_t hcap = 0;            // rows the pinned mirror holds (large batches stream through it in chunks: run_host)
    void* h_pin = nullptr;       // pinned mirror: theta [hcap][ndim] | lnprob [hcap] | fr [hcap][3] | status [hcap]
    size_t h_pin_bytes = 0;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_down[2] = {nullptr, nullptr};   // the chunk pipeline's slot events
    double* d_cube = nullptr;    // gf_lnprob_cube_batch: the unit-cube rows on the device
    size_t cube_cap = 0;
    double* d_btab = nullptr;    // gf_model_set_binned_measurement: [GF_MAX_BINS][GF_BINNED_STRIDE], allocated by the first call and kept
    int binned = 0;              // ... and from then on lnprob is the energy-resolved likelihood; c.mode stays BSM_GAUSS
    double* d_table = nullptr;   // gf_model_set_table_likelihood: ln L at the nodes of a lattice of side table_nside (gf_table.hpp)
    int table_nside = 0;         // ... and while > 0 lnprob is lnprior + the table's value; c.mode stays BSM_GAUSS
    int64_t table_cap = 0;       // nodes d_table has room for: a replacement that fits is written in place
    std::vector<double*> tables_retired;   // tables a larger replacement outgrew, kept until the model goes: a run set created
                                           // before the replacement still reads its own (gf_cube_runs.hip)
    uint64_t likelihood_sets = 0;   // successful gf_model_set_table_likelihood / gf_model_set_binned_measurement calls: what tells a run
                                    // that has begun that its likelihood was replaced, in place included (gf_model_likelihood_sets)
    std::mutex call_mu;          // serialises the entry points that use the model's staging buffers / the stream's unitarity workspace
};

// Makes the model's device the current one and gives the model its stream, which is created (or taken from the pool) the first time
// one of its entry points needs it:
// creating a HIP stream costs milliseconds (tools/rtcost.hip: 3.8 ms), and the models of a stacked grid
// sampler only lend their constants -- their launches go to the sampler's stream.
GF_LOCAL int ensure_stream(gf_model* m);
#define GF_STREAM(m)                      \
    do {                                  \
        int rs_ = ensure_stream(m);       \
        if (rs_ != GF_OK) return rs_;     \
    } while (0)

// the model's kernels for n rows on `st`; d_fr (lnprob only) and d_status may be NULL.  The caller holds call_mu.
GF_LOCAL int launch_lnprob(gf_model* m, hipStream_t st, const double* d_theta, int layout, int64_t n, double* d_lnprob, double* d_fr,
                           int32_t* d_status);
GF_LOCAL int launch_propagate(gf_model* m, hipStream_t st, const double* d_theta, int layout, int64_t n, double* d_fr, int32_t* d_status);
