// gf_sampler_host.h -- the ensemble sampler's host state, for the two files that make up its host side: gf_sampler_host.hip (gf_sampler,
// its runs, the C ABI) and gf_temper_host.hip (the tempered sampler).  ONLY those two include it: everything else sees a
// sampler through gf_internal_sampler_chain_view and the other gf_internal_sampler_* accessors (gf_internal.h).  Nothing here is exported
// from the library.
#pragma once
#include "gf_host.h"
#include "gf_modelset.h"
#include "gf_sampler_launch.h"

#pragma GCC visibility push(hidden)

// what a captured graph froze in its kernel arguments: the graph is valid while these are the run's (the CONTENT of the stream-id buffer
// is read at replay)
struct GfGraphFrozen {
    const double* chain = nullptr;
    const double* lnp_chain = nullptr;
    int64_t cap = -1;
    int store = -1;
    const uint64_t* stream_ids = nullptr;
    bool operator==(const GfGraphFrozen& o) const
    {
        return chain == o.chain && lnp_chain == o.lnp_chain && cap == o.cap && store == o.store && stream_ids == o.stream_ids;
    }
};

struct gf_sampler {
    // the chains' models: one that every chain samples, or (`multi`, gf_sampler_create_multi: even for one chain) one per chain.
    // Model 0's stream carries the sampler's launches; the set's device arrays are what the kernels that take constants by pointer read
    GfModelSet set;
    bool multi = false;
    int last_lpw = 0;                   // lanes per walker of the last run's grid kernels, 0 before the first (gf_internal_sampler_lpw)
    int nchains = 0, nwalkers = 0, ndim = 0;
    uint64_t seed = 0, iteration = 0;
    double a = 2.0;
    double* d_pos = nullptr;
    double* d_lnp = nullptr;
    uint32_t* d_naccept = nullptr;
    uint32_t* d_flags = nullptr;
    GfArbQueue* d_pq = nullptr;         // BSM posteriors: proposals parked for k_stretch_settle (capacity: one half-step's proposals)
    double* d_pend_rows = nullptr;      // [nchains * nwalkers / 2][GF_PEND_STRIDE]
    unsigned int* d_pend_ctl = nullptr; // [nchains * nwalkers / 2][2]: k_stretch_settle's per-walker counters, zero between uses
    double* d_lazy_rows = nullptr;      // k_stretch_chain: [nchains][lazy_cap][GF_PEND_STRIDE], undecided proposals that are rejected either way
    unsigned long long* d_lazy_mask = nullptr;   // [nchains][lazy_cap]
    int lazy_cap = 0;
    unsigned long long* d_chain_stats = nullptr;   // [nchains][8]: k_stretch_chain's per-chain census (ChainArgs::stats), zeroed by gf_sampler_reset
    // what the probe of a BSM sampler on small ensembles last chose: 0 = nothing yet, 1 = one workgroup per chain (k_stretch_chain), 2 =
    // the per-half-step grid kernels + k_stretch_settle.  Taken at the start of every run of 128 steps or more, by timing a block of 16
    // steps of each on the sampler's own chains (run_per_chain); which shape a run takes: run_shape (gf_sampler_host.hip)
    int shape = 0;
    double probe_us[2] = {0.0, 0.0};               // what the decision was taken on: us per block of 16 steps, [0] per chain, [1] grid
    double* d_chain = nullptr;
    double* d_lnp_chain = nullptr;
    int64_t nstore_cap = 0, nstored = 0;
    int64_t steps_since_reset = 0;
    uint64_t* d_stream_ids = nullptr;   // per-chain random stream ids (gf_sampler_set_stream_ids), else null
    GfStepState* d_state = nullptr;
    GfStepState h_state = {};
    // captured graph of GRAPH_STEPS steps (2 nodes per step + one tick) and what it froze; capture_graph alone decides that it is stale
    hipGraphExec_t graph = nullptr;
    GfGraphFrozen graph_of;
    // Blocks of steps in flight.  An event is recorded behind every block a run enqueues (a graph replay of 16 steps, or up to 64
    // eager steps), in a ring of FLIGHT slots: block k is not enqueued before block k - FLIGHT has completed, so the host never runs
    // more than FLIGHT blocks (~2 000 AQL packets) ahead of the GPU however long the run is.  gf_sampler_run_to_host hangs its
    // read-back on the same events (`sink`): a completed block's stored steps are copied to the host before its slot is reused.
    static constexpr int FLIGHT = 8;
    hipEvent_t flight_ev[FLIGHT] = {};
    int64_t flight_nstored[FLIGHT] = {};     // stored steps of every chain that are final once the slot's event has passed
    int64_t flight_enq = 0, flight_done = 0; // blocks of the current run: enqueued / consumed (waited for and, with a sink, copied)
    struct HostSink* sink = nullptr;
    struct GfTempered* tp = nullptr;         // gf_sampler_create_tempered: the tempered sampler's own state (gf_temper_host.hip), else null
};

// One run: what it was asked for and the steps enqueued so far.  A shape enqueues the steps [done, nsteps); the per-chain shape
// may leave the rest of the run to the grid shape after its probe.
struct Run {
    gf_sampler* s;
    int64_t nsteps;
    int thin, store;
    int64_t done;
    bool graphs = false;                // grid_begin: blocks of GRAPH_STEPS steps are replays of s->graph where there is one
};

// The per-half-step grid kernels of a run: k_stretch (k_stretch_multi: one model per chain) over all chains, and for BSM
// posteriors k_stretch_settle behind every half-step.
struct GridSteps {
    gf_sampler* s;
    StretchArgs a;
    GfSettleArgs sa;
    const double* betas = nullptr;      // a tempered sampler: [nchains], and the half-step is k_stretch_tempered (gf_temper.hip)
    hipError_t enqueue(int count);      // `count` steps relative to the device-side base counters, then k_tick
};
GridSteps grid_steps(gf_sampler* s, int store, int lpw);

// gf_sampler_create (multi false: every chain samples models[0]) and gf_sampler_create_multi (multi true: chain ch samples
// models[ch]): the model set has one entry per model.  want: the likelihood the sampler evaluates -- GF_LLH_BINNED
// (gf_sampler_create_binned), GF_LLH_TABLE (gf_sampler_create_table) or the flux-averaged one; every model must carry exactly that.
int sampler_create(gf_model* const* models, bool multi, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out, int want = GF_LLH_FLUX);
// GF_OK, or the refusal -- code and message -- of a model that carries the GfLikelihood `has` where the sampler evaluates `want`; index:
// the model's, as the caller numbers its models (a tempered sampler: the group's, not the chain's)
int sampler_likelihood_refusal(int want, int has, int index);
// GF_OK, or the refusal of the entry point `who` for a sampler whose models' likelihood is no longer the one it was created for
int sampler_kind_refusal(const gf_sampler* s, const char* who);
// Once per run, before its first grid block and with `g` complete: whether the run replays a graph (GF_SAMPLER_NO_GRAPH unset, at least
// 2 GRAPH_STEPS steps), and the graph captured if the sampler's is stale
void grid_begin(Run& r, GridSteps& g);
// THE loop of the grid shape: the steps [r.done, end) of a run as graph replays of GRAPH_STEPS steps, then eager blocks of up to 64
int run_grid(Run& r, GridSteps& g, int64_t end);

#pragma GCC visibility pop
