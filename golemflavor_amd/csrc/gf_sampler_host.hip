// gf_sampler_host.hip -- the host side of the device-resident ensemble sampler: the creation of a gf_sampler (gf_sampler_host.h) over
// a model set (gf_modelset.h), the ring of blocks in flight, the launch shape of a run (run_shape) and the shapes themselves with the
// graph capture and the one loop of the grid shape, and the C ABI.  The kernels, their argument structs and their launchers are
// gf_sampler.hip's (gf_sampler_launch.h); a tempered sampler's own state and its run are gf_temper_host.hip's, reached through
// gf_temper.h's four functions.  No kernel here.
#include <chrono>
#include <new>

#include "gf_devcache.h"                // large device allocations are cached, not handed back to the driver
#include "gf_sampler_host.h"
#include "gf_propose.hpp"               // lanes_per_walker
#include "gf_temper.h"                  // the tempered half-step's launcher, and the tempered sampler's host side (gf_temper_host.hip)

// gf_sampler_run_to_host's destination
struct HostSink {
    double* chain; double* lnp; int64_t total;     // host arrays of `total` stored steps per chain
    void* copy_stream; int device;
    struct gf_d2h_pipe* pipe = nullptr;            // ONE read-back pipeline for the whole run (gf_readback.hip)
    int64_t copied = 0;                            // stored steps whose copy has been issued
    int rc = GF_OK;
    std::chrono::steady_clock::time_point last_event;   // when the newest consumed block was seen complete
    // where the host thread's time went (diagnostics: gf_internal_run_to_host_times): [0] total / [1] longest call issuing a block's
    // copy, [2] total / [3] longest wait for a block to complete, [4] blocks, [5] total / [6] longest enqueue of a block of steps,
    // [7] from the call's entry to the first block's mark (chain buffer, graph capture, the launch-shape probe)
    double t[8] = {};
    std::chrono::steady_clock::time_point t_entry;
};
double g_last_run_to_host_times[8] = {};
double g_last_run_prologue[4] = {};             // the last gf_sampler_run: [0] growing the chain buffers, [1] capturing + instantiating the graph (seconds)

namespace {
// a stopwatch from its construction on: the seconds it ran are added to *total when it stops -- at stop() or at the end of its scope --
// and kept in *longest if they exceed it; without a total it only reads
struct Stopwatch {
    using clock = std::chrono::steady_clock;
    double* total;
    double* longest;
    clock::time_point t0 = clock::now();
    explicit Stopwatch(double* total_ = nullptr, double* longest_ = nullptr) : total(total_), longest(longest_) {}
    static double since(clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); }
    double seconds() const { return since(t0); }
    void stop()
    {
        if (!total) return;
        const double d = seconds();
        *total += d;
        if (longest && d > *longest) *longest = d;
        total = nullptr;
    }
    ~Stopwatch() { stop(); }
};

// The stretch kernels evaluate ONE likelihood, the one the entry point asked for (`want`): never silently for a model whose lnprob is
// another.  The refusals, model by model in the order the set examined them.
int sampler_refusal(const GfModelSet& set, int want)
{
    for (int ch = 0; ch < (int)set.carries.size(); ++ch)
        if (const int rc = sampler_likelihood_refusal(want, set.carries[ch], ch)) return rc;
    if (set.differs >= 0)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_sampler_create_multi: model %d differs from model 0 in device, ndim or mode", set.differs);
    return GF_OK;
}

// slot i of the run's HostSink::t, null without a sink: where a Stopwatch of the run adds to
double* sink_t(gf_sampler* s, int i) { return s->sink ? &s->sink->t[i] : nullptr; }

// the stored steps [sink->copied, upto) of every chain -> host: their chunks are ISSUED into the sink's pipe (pinned ring, copy stream); the
// host threads empty them into the destination while the caller goes on
int sink_copy(gf_sampler* s, int64_t upto)
{
    HostSink* k = s->sink;
    if (!k || k->rc != GF_OK || upto <= k->copied) return k ? k->rc : GF_OK;
    if (upto > k->total) upto = k->total;
    const size_t row = sizeof(double) * (size_t)s->nwalkers * s->ndim, lrow = sizeof(double) * (size_t)s->nwalkers;
    const size_t prev = (size_t)k->copied, now = (size_t)(upto - k->copied);
    Stopwatch clock(&k->t[0], &k->t[1]);
    k->t[4] += 1.0;
    // these steps of one of the two arrays, rows of `width` bytes per step: through the pipe, or (GF_RUN_TO_HOST_NO_PIPE, A/B) in a
    // pipeline of its own per block, as before the pipe
    auto steps = [&](double* host, const double* dev, size_t width) {
        char* dst = reinterpret_cast<char*>(host) + width * prev;
        const char* src = reinterpret_cast<const char*>(dev) + width * prev;
        const size_t dpitch = width * (size_t)k->total, spitch = width * (size_t)s->nstore_cap;
        return k->pipe ? gf_internal_d2h_pipe_rows(k->pipe, dst, dpitch, src, spitch, width * now, (size_t)s->nchains)
                       : gf_internal_d2h_2d(k->device, k->copy_stream, dst, dpitch, src, spitch, width * now, (size_t)s->nchains);
    };
    int rc = steps(k->chain, s->d_chain, row);
    if (rc == GF_OK && k->lnp) rc = steps(k->lnp, s->d_lnp_chain, lrow);
    k->rc = rc;
    k->copied = upto;
    return rc;
}

// Block j of the current run: has it completed?  wait = true blocks until it has.  A completed block is consumed -- its stored
// steps go to the sink, if there is one -- and its slot is free again.  Blocks are consumed in order.
hipError_t flight_consume(gf_sampler* s, bool wait)
{
    const int slot = (int)(s->flight_done % gf_sampler::FLIGHT);
    Stopwatch waited(wait ? sink_t(s, 2) : nullptr, sink_t(s, 3));
    hipError_t e = wait ? hipEventSynchronize(s->flight_ev[slot]) : hipEventQuery(s->flight_ev[slot]);
    waited.stop();
    if (e != hipSuccess) return e;                                  // hipErrorNotReady: still running
    if (s->sink) { s->sink->last_event = Stopwatch::clock::now(); (void)sink_copy(s, s->flight_nstored[slot]); }
    ++s->flight_done;
    return hipSuccess;
}

// before block `flight_enq` is enqueued: at most FLIGHT - 1 earlier blocks may still be running; and whatever has completed
// meanwhile is consumed on the way (with a sink: copied while the GPU works on the blocks behind it)
hipError_t flight_admit(gf_sampler* s)
{
    while (s->flight_enq - s->flight_done >= gf_sampler::FLIGHT) {
        const hipError_t e = flight_consume(s, true);
        if (e != hipSuccess) return e;
    }
    while (s->sink && s->flight_done < s->flight_enq) {
        const hipError_t e = flight_consume(s, false);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// an event behind the block just enqueued; `nstored` stored steps of every chain are final once it has passed
hipError_t flight_mark(gf_sampler* s, hipStream_t st, int64_t nstored)
{
    const int slot = (int)(s->flight_enq % gf_sampler::FLIGHT);
    if (s->sink && s->sink->t[7] == 0.0) s->sink->t[7] = Stopwatch::since(s->sink->t_entry);
    hipEvent_t& e = s->flight_ev[slot];
    if (!e) { const hipError_t ec = hipEventCreateWithFlags(&e, hipEventDisableTiming); if (ec != hipSuccess) { e = nullptr; return ec; } }
    const hipError_t er = hipEventRecord(e, st);
    if (er != hipSuccess) return er;
    s->flight_nstored[slot] = nstored;
    ++s->flight_enq;
    return hipSuccess;
}

// ---- gf_sampler_run: a prologue, the launch shape run_shape names, an epilogue -------------------------------------------------
// One block of `count` steps from r.done on, enqueued by launch(): admitted into the ring of blocks in flight, then marked with
// the stored steps of every chain that are final once it has run.  `what` names a failed launch.
template <class Launch>
int run_block(Run& r, int64_t count, const char* what, Launch launch)
{
    gf_sampler* s = r.s;
    hipError_t e = flight_admit(s);
    if (e != hipSuccess) return gf_hip_fail(e, "block in flight");
    e = launch();
    if (e != hipSuccess) return gf_hip_fail(e, what);
    r.done += count;
    e = flight_mark(s, s->set.stream, r.store ? s->nstored + (r.done + r.thin - 1) / r.thin : s->nstored);
    if (e != hipSuccess) return gf_hip_fail(e, "hipEventRecord");
    return GF_OK;
}

// room for `need` stored steps of every chain: chains are [chain][slot][walker][dim], so a new capacity changes the chain stride
// and the stored prefix is repacked
int grow_chain(gf_sampler* s, int64_t need)
{
    const size_t nw = (size_t)s->nchains * s->nwalkers;
    hipStream_t st = s->set.stream;
    int64_t cap = s->nstore_cap ? s->nstore_cap : 64;
    while (cap < need) cap *= 2;
    double *nc = nullptr, *nl = nullptr;
    GF_HIP(hipStreamSynchronize(st));
    g_last_run_prologue[0] = 0.0;
    Stopwatch growing(&g_last_run_prologue[0]);
    GF_HIP(gf_cached_malloc((void**)&nc, sizeof(double) * nw * s->ndim * cap));
    {
        hipError_t e_ = gf_cached_malloc((void**)&nl, sizeof(double) * nw * cap);
        if (e_ != hipSuccess) { (void)gf_cached_free(nc); return gf_hip_fail(e_, "hipMalloc(lnprob chain)"); }
    }
    if (s->nstored > 0) {
        // every chain's stored prefix in one strided copy: row = chain, pitch = old / new chain stride
        const size_t row = sizeof(double) * s->nwalkers * s->ndim, lrow = sizeof(double) * s->nwalkers;
        hipError_t e_ = hipMemcpy2DAsync(nc, row * cap, s->d_chain, row * s->nstore_cap, row * s->nstored, s->nchains,
                                         hipMemcpyDeviceToDevice, st);
        if (e_ == hipSuccess)
            e_ = hipMemcpy2DAsync(nl, lrow * cap, s->d_lnp_chain, lrow * s->nstore_cap, lrow * s->nstored, s->nchains,
                                  hipMemcpyDeviceToDevice, st);
        if (e_ == hipSuccess) e_ = hipStreamSynchronize(st);                  // the old buffers are freed next
        if (e_ != hipSuccess) { (void)gf_cached_free(nc); (void)gf_cached_free(nl); return gf_hip_fail(e_, "chain repack"); }
    }
    if (s->d_chain) (void)gf_cached_free(s->d_chain);
    if (s->d_lnp_chain) (void)gf_cached_free(s->d_lnp_chain);
    s->d_chain = nc; s->d_lnp_chain = nl; s->nstore_cap = cap;         // (a captured graph froze the old ones: capture_graph sees it)
    return GF_OK;
}

// Small ensembles of a PRIOR_ONLY / SM_GAUSS posterior: one workgroup per ensemble (k_stretch_persist), the whole run in one
// launch per CHUNK steps.
int run_persistent(Run& r)
{
    gf_sampler* s = r.s;
    int threads = 0, workers = 0;
    size_t lds = 0;
    gf_persist_geometry(s->nwalkers, s->ndim, &threads, &lds, &workers, s->nchains, s->set.cus);
    PersistArgs pa = {};
    pa.commons = s->set.d_commons; pa.ptabs = s->set.d_ptabs; pa.nmodels = (int32_t)s->set.models.size();
    pa.nwalkers = s->nwalkers; pa.pos = s->d_pos; pa.lnp = s->d_lnp; pa.naccept = s->d_naccept;
    pa.chain = r.store ? s->d_chain : nullptr; pa.lnp_chain = r.store ? s->d_lnp_chain : nullptr;
    pa.nstore_cap = s->nstore_cap; pa.seed = s->seed; pa.thin = r.thin; pa.store = r.store; pa.a = s->a;
    pa.stream_ids = s->d_stream_ids;
    pa.workers = workers;
    constexpr int64_t CHUNK = 1 << 16;                          // steps per launch: bounds a kernel's run time
    while (r.done < r.nsteps) {
        // every launch but the last covers a whole multiple of `thin` steps, so that the kernel's
        // (step % thin) == 0 test, which counts from the launch's first step, stays aligned with the run
        const int64_t left = r.nsteps - r.done;
        int64_t count = left < CHUNK ? left : CHUNK;
        if (count < left) {
            const int64_t whole = (count / r.thin) * r.thin;
            count = whole > 0 ? whole : r.thin;
            if (count > left) count = left;                     // thin longer than what is left
        }
        pa.iteration_base = s->iteration + (uint64_t)r.done;
        pa.store_base = s->nstored + (r.done + r.thin - 1) / r.thin;
        pa.nsteps = count;
        hipError_t e = gf_launch_persist(s->set.mode, s->ndim, s->nchains, threads, lds, pa, s->set.stream);
        if (e != hipSuccess) return gf_hip_fail(e, "persistent stretch launch");
        r.done += count;
    }
    return GF_OK;
}

// `count` steps of the grid kernels, one block in flight
int grid_block(Run& r, GridSteps& g, int count)
{
    return run_block(r, count, "stretch launch", [&] { return g.enqueue(count); });
}

// k_stretch_chain's lists of the proposals whose verdict only the count waits for -- at least two passes' worth per chain, ~64 MB
// in all -- and its per-chain census (left out if it cannot be allocated), at the sampler's first per-chain run
int alloc_lazy_lists(gf_sampler* s)
{
    if (s->d_lazy_rows) return GF_OK;
    const int pass = s->nwalkers < CH_BLOCK ? s->nwalkers : CH_BLOCK;
    int64_t cap = ((int64_t)64 << 20) / ((int64_t)s->nchains * (int64_t)(sizeof(double) * GF_PEND_STRIDE + 8));
    if (cap > 1024) cap = 1024;
    if (cap < 2 * pass) cap = 2 * pass;
    GF_HIP(gf_cached_malloc((void**)&s->d_lazy_rows, sizeof(double) * GF_PEND_STRIDE * (size_t)cap * s->nchains));
    {
        hipError_t e_ = gf_cached_malloc((void**)&s->d_lazy_mask, sizeof(unsigned long long) * (size_t)cap * s->nchains);
        if (e_ != hipSuccess) { (void)gf_cached_free(s->d_lazy_rows); s->d_lazy_rows = nullptr; return gf_hip_fail(e_, "hipMalloc(lazy list)"); }
    }
    s->lazy_cap = (int)cap;
    if (gf_cached_malloc((void**)&s->d_chain_stats, sizeof(unsigned long long) * 8 * (size_t)s->nchains) == hipSuccess)
        (void)hipMemsetAsync(s->d_chain_stats, 0, sizeof(unsigned long long) * 8 * (size_t)s->nchains, s->set.stream);
    else { s->d_chain_stats = nullptr; (void)hipGetLastError(); }
    return GF_OK;
}

// BSM posteriors on ensembles of up to 1024 walkers have two launch shapes with the same chain, bit for bit:
//   per chain   one workgroup owns a chain for a block of 16 steps and settles its own parked proposals (k_stretch_chain): a chain that
//               parks nothing never waits for one that does -- 21 us per half-step where nothing is parked (C5: 256 x 512 walkers);
//   grid        one launch per half-step for all chains + k_stretch_settle on the whole GPU (round 3): every chain waits for the
//               slowest parked proposal, but a chain that parks TEN proposals per half-step (the top-scale grid points of C5) gets
//               3 584 teams for them instead of its workgroup's 56 -- 115 us per half-step against 150.
// Which is faster depends on where the chains live NOW (a burn-in that starts below the failing region and drifts into it parks
// nothing at first), so every run of 128 steps or more times one block of each shape on its own chains at its start (the second
// block of two, the first warms the kernel up; the blocks are the run's own steps, nothing is computed twice) and takes the faster
// for the rest of the run; shorter runs take the last decision (none yet: per chain).  GF_SAMPLER_CHAIN=1 / 0 forces a shape
// (run_shape).  The per-chain shape of a run, with the probe (`probe`) at its start: where that chose the grid kernels it returns
// with r.done < r.nsteps, and the rest of the run is the grid shape's.
constexpr int64_t CHAIN_STEPS = 16;                                      // steps per launch: the granule of the overlapped read-back
int run_per_chain(Run& r, GridSteps& g, bool probe)
{
    gf_sampler* s = r.s;
    hipStream_t st = s->set.stream;
    int rc = alloc_lazy_lists(s);
    if (rc != GF_OK) return rc;
    ChainArgs ca = {};
    ca.lazy_rows = s->d_lazy_rows; ca.lazy_mask = s->d_lazy_mask; ca.lazy_cap = s->lazy_cap;
    ca.stats = s->d_chain_stats;
    ca.commons = s->set.d_commons; ca.tbs = s->multi ? s->set.d_tbs : nullptr; ca.tb = s->set.tb; ca.ptabs = s->set.d_ptabs;
    ca.nmodels = (int32_t)s->set.models.size(); ca.nwalkers = s->nwalkers;
    ca.pos = s->d_pos; ca.lnp = s->d_lnp; ca.naccept = s->d_naccept; ca.flags = s->d_flags; ca.pend_rows = s->d_pend_rows;
    ca.chain = r.store ? s->d_chain : nullptr; ca.lnp_chain = r.store ? s->d_lnp_chain : nullptr;
    ca.nstore_cap = s->nstore_cap; ca.store_base = s->nstored; ca.seed = s->seed; ca.thin = r.thin; ca.store = r.store;
    ca.a = s->a; ca.stream_ids = s->d_stream_ids;
    auto chain_block = [&](int64_t count) {                              // `count` steps from r.done on, one launch
        return run_block(r, count, "chain launch", [&] {
            ca.iteration_base = s->iteration + (uint64_t)r.done;
            ca.run_step_base = r.done;
            ca.nsteps = (int32_t)count;
            return gf_launch_chain(s->ndim, s->nchains, ca, st);
        });
    };
    if (probe) {
        // two blocks per chain, two blocks on the grid, the second of each timed; k_tick after a per-chain block brings the grid
        // kernels' device-side counters along
        double us[2] = {0.0, 0.0};
        for (int which = 0; which < 2; ++which)
            for (int rep = 0; rep < 2; ++rep) {
                GF_HIP(hipStreamSynchronize(st));
                const Stopwatch block;
                if (which == 0) {
                    rc = chain_block(CHAIN_STEPS);
                    if (rc == GF_OK && gf_launch_tick(s->d_state, (int)CHAIN_STEPS, st) != hipSuccess) rc = GF_ERR_HIP;
                } else {
                    rc = grid_block(r, g, (int)CHAIN_STEPS);
                }
                if (rc != GF_OK) return rc;
                GF_HIP(hipStreamSynchronize(st));
                if (rep == 1) us[which] = 1e6 * block.seconds();
            }
        s->probe_us[0] = us[0]; s->probe_us[1] = us[1];
        s->shape = us[0] <= us[1] ? 1 : 2;
        if (s->shape == 2) return GF_OK;
    }
    while (r.done < r.nsteps) {
        rc = chain_block(r.nsteps - r.done < CHAIN_STEPS ? r.nsteps - r.done : CHAIN_STEPS);
        if (rc != GF_OK) return rc;
    }
    return GF_OK;
}

// s->graph: GRAPH_STEPS steps of `g` captured (2 nodes per step + one tick), recaptured when what it froze in its kernel arguments
// (GfGraphFrozen) is no longer the run's -- the one place that decides so: grown chain buffers and a first set of stream ids show
// here; null where capture fails (the run launches eagerly then)
constexpr int GRAPH_STEPS = 16;
void capture_graph(gf_sampler* s, GridSteps& g, int store)
{
    const GfGraphFrozen now = {g.a.chain, g.a.lnp_chain, g.a.nstore_cap, store, g.a.stream_ids};
    if (s->graph && s->graph_of == now) return;
    if (s->graph) { (void)hipGraphExecDestroy(s->graph); s->graph = nullptr; }
    hipGraph_t gr = nullptr;
    g_last_run_prologue[1] = 0.0;
    Stopwatch capturing(&g_last_run_prologue[1]);
    hipError_t e = hipStreamBeginCapture(s->set.stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        e = g.enqueue(GRAPH_STEPS);
        hipError_t e2 = hipStreamEndCapture(s->set.stream, &gr);
        if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&s->graph, gr, nullptr, nullptr, 0);
    if (gr) (void)hipGraphDestroy(gr);
    if (e != hipSuccess) {                      // graphs unavailable: eager launches
        (void)hipGetLastError();
        s->graph = nullptr;
    } else {
        s->graph_of = now;
    }
}

// A sampler with ONE launch shape, the per-half-step grid kernels: the energy-resolved, the tabulated and the tempered ones.
bool grid_only(const gf_sampler* s) { return s->set.kind != GF_LLH_FLUX || s->tp; }

// What a run of `nsteps` steps does -- the one place that decides it.  The overrides are read in this order, once per run, each only
// where it could change the outcome's branch: GF_SAMPLER_PERSIST ("0": never the persistent kernel), then GF_SAMPLER_CHAIN ("0": grid
// kernels; "1": per chain) for a flux-averaged BSM sampler of up to 1024 walkers.  Unforced, such a sampler probes at the start of a run
// of 128 steps or more and takes its last probe's choice (none yet: per chain) in a shorter one.
enum class Shape { PERSISTENT, PER_CHAIN, PER_CHAIN_PROBE, GRID, TEMPERED };
Shape run_shape(const gf_sampler* s, int64_t nsteps)
{
    int threads = 0;
    size_t lds = 0;                                                 // 0: the ensemble does not fit one workgroup
    gf_persist_geometry(s->nwalkers, s->ndim, &threads, &lds, nullptr, s->nchains, s->set.cus);
    const char* env = gf_internal_env("GF_SAMPLER_PERSIST", 0);
    const bool bsm = s->set.mode == MODE_BSM_GAUSS;
    if (s->tp) return Shape::TEMPERED;
    if (!bsm && lds > 0 && !(env && env[0] == '0')) return Shape::PERSISTENT;
    if (!bsm || grid_only(s) || s->nwalkers / 2 > 512) return Shape::GRID;
    env = gf_internal_env("GF_SAMPLER_CHAIN", 0);
    if (env && (env[0] == '0' || env[0] == '1')) return env[0] == '0' ? Shape::GRID : Shape::PER_CHAIN;
    if (nsteps >= 8 * CHAIN_STEPS) return Shape::PER_CHAIN_PROBE;
    return s->shape == 2 ? Shape::GRID : Shape::PER_CHAIN;
}

// gf_sampler_create_binned / _table: one model for every chain, or (nmodels == nchains) one per chain
int sampler_create_of(gf_model* const* models, int nmodels, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out, int want)
{
    if (!models || !out || nchains < 1 || nchains > 65535 || (nmodels != 1 && nmodels != nchains)) return GF_ERR_INVALID_ARG;
    *out = nullptr;
    for (int ch = 0; ch < nmodels; ++ch)
        if (!models[ch]) return GF_ERR_INVALID_ARG;
    return sampler_create(models, nmodels == nchains && nchains > 1, nchains, nwalkers, seed, a, out, want);
}
}  // namespace

// ---- what the tempered sampler's host side shares (gf_sampler_host.h) ----------------------------------------------------------
// The stretch kernels' likelihood stays the one the sampler was created for: a model that has since gained a table or a measurement is
// refused by every entry point that evaluates (`who`), before it launches or writes anything.  The stored chain and state stay as they are.
int sampler_kind_refusal(const gf_sampler* s, const char* who)
{
    int now = GF_LLH_FLUX;
    const int differs = gf_modelset_kind_differs(&s->set, &now);
    if (differs < 0) return GF_OK;
    return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: model %d now carries %s; the sampler's kernels evaluate the likelihood it was created for (%s)", who, differs,
                       gf_likelihood_name(now), gf_likelihood_name(s->set.kind));
}

int sampler_likelihood_refusal(int want, int has, int index)
{
    if (has == want) return GF_OK;
    if (want == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_sampler_create_table: model %d carries no tabulated likelihood; all of a sampler's models must", index);
    if (has == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_sampler_create: model %d carries a tabulated likelihood; sample the flux-averaged model and reweight the chain to this one", index);
    if (want == GF_LLH_BINNED)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_sampler_create_binned: model %d carries no binned measurement; all of a sampler's models must", index);
    return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_sampler_create: model %d carries a binned measurement; sample the flux-averaged model and reweight the chain to this one", index);
}

int sampler_create(gf_model* const* models, bool multi, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out, int want)
{
    if (!out || nchains < 1 || nwalkers < 2 || (nwalkers & 1) || !(a > 1.0)) return GF_ERR_INVALID_ARG;
    *out = nullptr;
    const char* who = want == GF_LLH_TABLE ? "gf_sampler_create_table" : want == GF_LLH_BINNED ? "gf_sampler_create_binned" : multi ? "gf_sampler_create_multi" : "gf_sampler_create";
    gf_sampler* s = new (std::nothrow) gf_sampler();
    if (!s) return GF_ERR_ALLOC;
    const GfModelSet& set = s->set;
    int rc = gf_modelset_create(&s->set, models, multi ? nchains : 1, who);
    if (set.ndim == 0 || nwalkers < 2 * set.ndim) rc = GF_ERR_INVALID_ARG;        // models[0] is unusable; emcee's own requirement
    else if (const int refused = sampler_refusal(set, want)) rc = refused;
    if (rc != GF_OK) { gf_sampler_destroy(s); return rc; }
    s->multi = multi;
    s->nchains = nchains; s->nwalkers = nwalkers; s->ndim = set.ndim; s->seed = seed; s->a = a;
    const size_t nw = (size_t)nchains * nwalkers;
    // every transfer of this file goes through the sampler's stream: a synchronous (null-stream) hipMemcpy / hipMemset
    // issued while ANOTHER host thread is capturing its sampler's graph fails and poisons that capture on this runtime
    hipStream_t st0 = set.stream;
    hipError_t e = hipSetDevice(set.device);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&s->d_pos, sizeof(double) * nw * s->ndim);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&s->d_lnp, sizeof(double) * nw);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&s->d_naccept, sizeof(uint32_t) * nw);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&s->d_flags, sizeof(uint32_t) * 4);
    if (e == hipSuccess && set.mode == MODE_BSM_GAUSS)
        e = gf_alloc_arb_queue(GF_MEM_CACHED, (size_t)nchains * (nwalkers / 2), st0, &s->d_pq, &s->d_pend_rows, &s->d_pend_ctl);
    if (e == hipSuccess) e = gf_cached_malloc((void**)&s->d_state, sizeof(GfStepState));
    if (e == hipSuccess) e = hipMemsetAsync(s->d_state, 0, sizeof(GfStepState), st0);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_naccept, 0, sizeof(uint32_t) * nw, st0);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_flags, 0, sizeof(uint32_t) * 4, st0);
    if (e == hipSuccess) e = hipStreamSynchronize(st0);
    if (e != hipSuccess) { gf_sampler_destroy(s); return gf_hip_fail(e, who); }
    *out = s;
    return GF_OK;
}

hipError_t GridSteps::enqueue(int count)
{
    for (int i = 0; i < count; ++i) {
        a.step_offset = i;
        for (int half = 0; half < 2; ++half) {
            a.half = half;
            hipError_t e = betas ? gf_launch_stretch_tempered(a, betas, s->ndim, s->set.stream)
                                 : gf_launch_stretch(*s->set.c, s->set.tb, s->set.ptab, a, s->set.stream);
            if (e != hipSuccess) return e;
            if (s->set.mode == MODE_BSM_GAUSS) {
                // the proposals whose unitarity the half-step could not settle: exact verdict, then their accept step
                sa.half = half; sa.step_offset = i;
                e = gf_launch_stretch_settle(sa, s->set.cus, s->set.stream);
                if (e != hipSuccess) return e;
            }
        }
    }
    return gf_launch_tick(s->d_state, count, s->set.stream);
}

GridSteps grid_steps(gf_sampler* s, int store, int lpw)
{
    GridSteps g;
    g.s = s;
    StretchArgs& a = g.a;
    a = {};
    a.state = s->d_state;
    a.pos = s->d_pos; a.lnp = s->d_lnp; a.naccept = s->d_naccept; a.flags = s->d_flags;
    a.pq = s->d_pq; a.pend_rows = s->d_pend_rows;
    a.chain = store ? s->d_chain : nullptr;
    a.lnp_chain = store ? s->d_lnp_chain : nullptr;
    a.nstore_cap = s->nstore_cap; a.seed = s->seed; a.nchains = s->nchains; a.nwalkers = s->nwalkers; a.a = s->a;
    a.commons = s->multi ? s->set.d_commons : nullptr; a.tbs = s->set.d_tbs; a.ptabs = s->set.d_ptabs;
    a.nbins_max = s->set.nbins_max;
    a.stream_ids = s->d_stream_ids;
    a.btabs = s->set.d_btabs;
    a.ttabs = s->set.d_ttabs; a.tsides = s->set.d_tsides;
    a.lpw = lpw;
    GfSettleArgs& sa = g.sa;
    sa = {};
    sa.state = s->d_state; sa.pq = s->d_pq; sa.pend_rows = s->d_pend_rows; sa.ctl = s->d_pend_ctl; sa.pos = s->d_pos; sa.lnp = s->d_lnp; sa.naccept = s->d_naccept;
    sa.flags = s->d_flags; sa.chain = a.chain; sa.lnp_chain = a.lnp_chain; sa.nstore_cap = s->nstore_cap; sa.nchains = s->nchains;
    sa.nwalkers = s->nwalkers; sa.half = 0; sa.step_offset = 0; sa.ndim = s->ndim; sa.commons = s->set.d_commons; sa.tbs = s->set.d_tbs; sa.tb = s->set.tb;
    sa.multi = s->multi ? 1 : 0;
    return g;
}

void grid_begin(Run& r, GridSteps& g)
{
    const bool no_graph = gf_internal_env("GF_SAMPLER_NO_GRAPH", 0) != nullptr;          // diagnostics, read per run
    r.graphs = !no_graph && r.nsteps >= 2 * GRAPH_STEPS;
    if (r.graphs) capture_graph(r.s, g, r.store);
}

// The launch-bound inner loop of every grid-shape run: a plain one (end = r.nsteps), what the per-chain shape leaves after its probe,
// and a tempered sampler's steps up to its next round.
int run_grid(Run& r, GridSteps& g, int64_t end)
{
    gf_sampler* s = r.s;
    while (r.graphs && s->graph && end - r.done >= GRAPH_STEPS) {
        const int rc = run_block(r, GRAPH_STEPS, "hipGraphLaunch", [&] {
            Stopwatch enqueue(sink_t(s, 5), sink_t(s, 6));
            return hipGraphLaunch(s->graph, s->set.stream);
        });
        if (rc != GF_OK) return rc;
    }
    while (r.done < end) {
        const int rc = grid_block(r, g, (int)(end - r.done < 64 ? end - r.done : 64));
        if (rc != GF_OK) return rc;
    }
    return GF_OK;
}

extern "C" {

int gf_sampler_create(gf_model* m, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out)
{
    if (!m) return GF_ERR_INVALID_ARG;
    return sampler_create(&m, false, nchains, nwalkers, seed, a, out);
}

// One ensemble per model: chain ch samples the posterior of models[ch].  All models must live on the same
// device and share ndim and mode (one kernel instance); everything else -- priors, fixed values, best fit,
// smearing, texture, dimension, binning -- may differ.  The models must outlive the sampler.
int gf_sampler_create_multi(gf_model* const* models, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out)
{
    if (!models || !out || nchains < 1 || nchains > 65535) return GF_ERR_INVALID_ARG;   // blockIdx.y = chain
    *out = nullptr;
    for (int ch = 0; ch < nchains; ++ch)
        if (!models[ch]) return GF_ERR_INVALID_ARG;
    return sampler_create(models, true, nchains, nwalkers, seed, a, out);
}

// A sampler of the energy-resolved likelihood: every model carries a binned measurement
// (gf_model_set_binned_measurement).  nmodels == 1: every chain samples models[0]; nmodels == nchains: chain ch samples
// models[ch], as gf_sampler_create_multi.  The tables' addresses are taken here and stay the models' own: a measurement set
// between two runs is the one the next run samples.
int gf_sampler_create_binned(gf_model* const* models, int nmodels, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out)
{
    return sampler_create_of(models, nmodels, nchains, nwalkers, seed, a, out, GF_LLH_BINNED);
}

// A sampler of the tabulated flavour-plane likelihood: every model carries a table (gf_model_set_table_likelihood).
// nmodels == 1: every chain samples models[0]; nmodels == nchains: chain ch samples models[ch], as gf_sampler_create_multi; the sides
// may differ from chain to chain.  The sampler keeps its models and takes each one's table again at the start of every run.
int gf_sampler_create_table(gf_model* const* models, int nmodels, int nchains, int nwalkers, uint64_t seed, double a, gf_sampler** out)
{
    return sampler_create_of(models, nmodels, nchains, nwalkers, seed, a, out, GF_LLH_TABLE);
}

// diagnostics (not part of the ABI): proposals since the last reset that the half-step kernel parked and k_stretch_settle completed;
// counted by the energy-resolved, the tabulated and the tempered instances alone, GF_ERR_UNSUPPORTED for every other sampler
int gf_internal_sampler_parked(gf_sampler* s, uint32_t* out)
{
    if (!s || !out) return GF_ERR_INVALID_ARG;
    if (s->set.kind == GF_LLH_FLUX && !s->tp) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(s->set.device));
    GF_HIP(hipMemcpyAsync(out, s->d_flags + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s->set.stream));
    GF_HIP(hipStreamSynchronize(s->set.stream));
    return GF_OK;
}

// internal (gf_reweight.hip): the GfLikelihood the sampler's chains were sampled under
int gf_internal_sampler_likelihood(const gf_sampler* s) { return s ? s->set.kind : GF_LLH_FLUX; }
// diagnostics: lanes per walker of the last run's grid kernels (0: no run yet, or the run took another launch shape)
int gf_internal_sampler_lpw(const gf_sampler* s) { return s ? s->last_lpw : 0; }

void gf_sampler_destroy(gf_sampler* s)
{
    if (!s) return;
    gf_modelset_free(&s->set);          // behind it the stream has drained
    void* ptrs[] = {s->d_pos, s->d_lnp, s->d_naccept, s->d_flags, s->d_pq, s->d_pend_rows, s->d_pend_ctl, s->d_lazy_rows, s->d_lazy_mask, s->d_chain_stats,
                    s->d_state, s->d_chain, s->d_lnp_chain, s->d_stream_ids};
    for (void* p : ptrs) if (p) (void)gf_cached_free(p);
    if (s->graph) (void)hipGraphExecDestroy(s->graph);
    for (int i = 0; i < gf_sampler::FLIGHT; ++i) if (s->flight_ev[i]) (void)hipEventDestroy(s->flight_ev[i]);
    gf_temper_free(s->tp);
    delete s;
}

// Random stream of every chain (default: the chain's index in this sampler).  ids [nchains]; call before the first run.
int gf_sampler_set_stream_ids(gf_sampler* s, const uint64_t* ids)
{
    if (!s || !ids) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    GF_HIP(hipStreamSynchronize(st));
    if (!s->d_stream_ids) GF_HIP(gf_cached_malloc((void**)&s->d_stream_ids, sizeof(uint64_t) * (size_t)s->nchains));
    GF_HIP(hipMemcpyAsync(s->d_stream_ids, ids, sizeof(uint64_t) * (size_t)s->nchains, hipMemcpyHostToDevice, st));
    GF_HIP(hipStreamSynchronize(st));               // (a graph captured without ids froze a null pointer: capture_graph sees it)
    return GF_OK;
}

// p0: [nchains][nwalkers][ndim] host; evaluates lnprob of the start positions on the device.
int gf_sampler_set_state(gf_sampler* s, const double* pos)
{
    if (!s || !pos) return GF_ERR_INVALID_ARG;
    if (const int rc = sampler_kind_refusal(s, "gf_sampler_set_state")) return rc;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    const size_t nw = (size_t)s->nchains * s->nwalkers;
    GF_HIP(hipMemcpyAsync(s->d_pos, pos, sizeof(double) * nw * s->ndim, hipMemcpyHostToDevice, st));
    if (s->tp) return gf_temper_start(s);           // a tempered sampler: the walkers' scalar at their chain's beta
    // BSM posteriors: with the unitarity status, so that a start position the reference would have raised on is treated as such
    int32_t* d_st = nullptr;
    if (s->set.mode == MODE_BSM_GAUSS) GF_HIP(gf_cached_malloc((void**)&d_st, sizeof(int32_t) * nw));
    int rc = GF_OK;
    if (!s->multi) {
        rc = gf_model_lnprob_on(s->set.models[0], st, s->d_pos, GF_LAYOUT_AOS, (int64_t)nw, s->d_lnp, nullptr, d_st);
    } else {
        for (int ch = 0; ch < s->nchains && rc == GF_OK; ++ch)         // every chain's own posterior, on the sampler's stream
            rc = gf_model_lnprob_on(s->set.models[ch], st, s->d_pos + (size_t)ch * s->nwalkers * s->ndim, GF_LAYOUT_AOS,
                                    s->nwalkers, s->d_lnp + (size_t)ch * s->nwalkers, nullptr, d_st ? d_st + (size_t)ch * s->nwalkers : nullptr);
    }
    hipError_t e = hipSuccess;
    if (rc == GF_OK && d_st) {
        e = gf_launch_fix_start(d_st, (int64_t)nw, s->d_lnp, s->d_flags, st);
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (d_st) (void)gf_cached_free(d_st);
    if (rc != GF_OK) return rc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_set_state");
    return gf_internal_check_overflow(s->set.device, st);
}

int gf_sampler_reset(gf_sampler* s)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    GF_HIP(hipStreamSynchronize(st));
    GF_HIP(hipMemsetAsync(s->d_naccept, 0, sizeof(uint32_t) * (size_t)s->nchains * s->nwalkers, st));
    GF_HIP(hipMemsetAsync(s->d_flags, 0, sizeof(uint32_t) * 4, st));
    if (s->d_chain_stats) GF_HIP(hipMemsetAsync(s->d_chain_stats, 0, sizeof(unsigned long long) * 8 * (size_t)s->nchains, st));
    if (s->tp) GF_HIP(gf_temper_clear_counts(s));
    GF_HIP(hipStreamSynchronize(st));
    s->nstored = 0;
    s->steps_since_reset = 0;
    return GF_OK;
}

// Advance every ensemble by nsteps stretch-move steps (2 launches each), asynchronously on the model's
// stream.  store != 0 appends every `thin`-th step to the device chain (capacity grows as needed).
int gf_sampler_run(gf_sampler* s, int64_t nsteps, int thin, int store)
{
    if (!s || nsteps < 0 || thin < 1) return GF_ERR_INVALID_ARG;
    if (const int rc = sampler_kind_refusal(s, "gf_sampler_run")) return rc;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    const int64_t nstore = store ? (nsteps + thin - 1) / thin : 0;     // steps this run stores
    if (s->nstored + nstore > s->nstore_cap) {
        const int rc = grow_chain(s, s->nstored + nstore);
        if (rc != GF_OK) return rc;
    }
    // device-side step counters for this run
    GfStepState& hs = s->h_state;                   // member: outlives the asynchronous upload
    hs.iteration_base = s->iteration; hs.run_step_base = 0; hs.store_base = s->nstored;
    hs.store = store ? 1 : 0; hs.thin = thin;
    GF_HIP(hipStreamSynchronize(st));          // earlier runs must be done with the counters
    s->flight_enq = s->flight_done = 0;         // (so nothing of an earlier run is in flight either)
    GF_HIP(hipMemcpyAsync(s->d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    if (const int rc = gf_modelset_refresh_tables(&s->set, "gf_sampler_run")) return rc;       // a table sampler: the models' tables of now

    // the launch shape; the overrides are read in this order, once per run: GF_SAMPLER_LPW, run_shape's, GF_SAMPLER_NO_GRAPH (grid_begin)
    Run r = {s, nsteps, thin, store ? 1 : 0, 0};
    // (a sampler of the energy-resolved likelihood has the grid kernels at one lane per walker: no override is read for that;
    // a sampler of the tabulated likelihood has them at the lanes per walker the flux-averaged rule gives)
    GridSteps g = grid_steps(s, r.store, s->set.kind == GF_LLH_BINNED ? 1 : lanes_per_walker(s->set.mode, (int64_t)s->nchains * (s->nwalkers / 2), s->set.nbins_max, s->set.cus,
                                                                               {true, 48 * 1024, "GF_SAMPLER_LPW"}));
    const Shape shape = run_shape(s, nsteps);
    int rc = GF_OK;
    switch (shape) {
    case Shape::TEMPERED:               // the grid kernels alone, one model and one beta per chain, and its rounds between their blocks
        s->last_lpw = g.a.lpw;
        rc = gf_temper_run(r, g);
        break;
    case Shape::PERSISTENT:
        rc = run_persistent(r);
        break;
    case Shape::PER_CHAIN:
    case Shape::PER_CHAIN_PROBE:
        s->last_lpw = 0;
        rc = run_per_chain(r, g, shape == Shape::PER_CHAIN_PROBE);
        if (rc != GF_OK || r.done == r.nsteps) break;
        [[fallthrough]];                // the probe chose the grid kernels for the rest of the run
    case Shape::GRID:
        s->last_lpw = g.a.lpw;
        grid_begin(r, g);
        rc = run_grid(r, g, r.nsteps);
        break;
    }
    if (rc != GF_OK) return rc;

    s->iteration += (uint64_t)nsteps;
    s->steps_since_reset += nsteps;
    s->nstored += nstore;
    return GF_OK;
}

int gf_sampler_sync(gf_sampler* s)
{
    if (!s) return GF_ERR_INVALID_ARG;
    return gf_model_sync(s->set.models[0]);
}

// gf_sampler_run(..., store = 1) with the read-back of the chain overlapped: the run is enqueued as usual (asynchronously, an
// event behind every block of 16 steps), and while the GPU works through it this thread copies every finished block of steps
// of all chains to the host on a second stream, through the library's pinned ring.  On return the run is complete and
// chain [nchains][nstored][nwalkers][ndim] / lnprob_chain [nchains][nstored][nwalkers] (may be NULL) hold the WHOLE stored chain
// (steps stored by earlier runs included).  What sampler.chain needs after run_mcmc (golemflavor/mcmc.py:41-43), without the
// wait for the read-back at the end.  *readback_tail_s (may be NULL): seconds between the end of the run on the GPU and the end of
// the last copy -- what of the read-back was NOT hidden behind the run.
int gf_sampler_run_to_host(gf_sampler* s, int64_t nsteps, int thin, double* chain, double* lnprob_chain, double* readback_tail_s)
{
    if (!s || !chain || nsteps < 0 || thin < 1) return GF_ERR_INVALID_ARG;
    if (const int refused = sampler_kind_refusal(s, "gf_sampler_run_to_host")) return refused;      // before the copy stream and the pipe
    GF_HIP(hipSetDevice(s->set.device));
    const int device = s->set.device;
    void* copy_stream = nullptr;
    int rc = gf_internal_borrow_copy_stream(device, &copy_stream);
    if (rc != GF_OK) return rc;
    // One thread, one pipeline: gf_sampler_run enqueues block after block and, between two blocks, hands every block the GPU has
    // finished meanwhile to the sink (flight_admit) -- at most FLIGHT blocks are ever enqueued ahead of the GPU, and the copies run
    // while the GPU works through them.  (Round 3 enqueued the whole run first and only then started to copy.)
    HostSink sink;
    sink.chain = chain; sink.lnp = lnprob_chain; sink.total = s->nstored + (nsteps + thin - 1) / thin;
    sink.copy_stream = copy_stream; sink.device = device;
    sink.last_event = sink.t_entry = Stopwatch::clock::now();
    if (gf_internal_env("GF_RUN_TO_HOST_NO_PIPE", 0) == nullptr) {       // diagnostics / A-B: else every block is a read-back of its own
        rc = gf_internal_d2h_pipe_open(device, copy_stream, &sink.pipe);
        if (rc != GF_OK) { gf_internal_return_copy_stream(device, copy_stream); return rc; }
    }
    const bool marks = gf_internal_env("GF_RUN_TO_HOST_NO_MARKS", 0) == nullptr;      // diagnostics: no sink during the run = one copy after it
    s->sink = marks ? &sink : nullptr;
    rc = gf_sampler_run(s, nsteps, thin, 1);
    hipError_t e = hipSuccess;
    while (rc == GF_OK && e == hipSuccess && s->flight_done < s->flight_enq) e = flight_consume(s, true);   // the blocks still in flight
    s->sink = nullptr;
    const hipError_t e2 = hipStreamSynchronize(s->set.stream);
    auto t_done = marks && s->flight_enq > 0 ? sink.last_event : Stopwatch::clock::now();        // when the run itself was complete on the GPU
    if (rc == GF_OK && e == hipSuccess && e2 == hipSuccess && sink.rc == GF_OK) {
        s->sink = &sink;                                            // whatever no block's event covered (one-launch runs; no marks)
        (void)sink_copy(s, s->nstored);
        s->sink = nullptr;
    }
    const int rc_pipe = gf_internal_d2h_pipe_close(sink.pipe);          // drains: every chunk is in the destination
    (void)hipStreamSynchronize((hipStream_t)copy_stream);
    gf_internal_return_copy_stream(device, copy_stream);
    if (rc == GF_OK && sink.rc == GF_OK) sink.rc = rc_pipe;
    if (readback_tail_s) *readback_tail_s = Stopwatch::since(t_done);
    for (int i = 0; i < 8; ++i) g_last_run_to_host_times[i] = sink.t[i];
    if (rc != GF_OK) return rc;
    if (sink.rc != GF_OK) return sink.rc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_run_to_host");
    return GF_OK;
}

// diagnostics (tools/, not part of the ABI): k_stretch_chain's per-chain census since the last reset, out [nchains][8] (ChainArgs::stats);
// GF_ERR_UNSUPPORTED where the sampler has not run that kernel
int gf_internal_sampler_chain_stats(gf_sampler* s, unsigned long long* out)
{
    if (!s || !out) return GF_ERR_INVALID_ARG;
    if (!s->d_chain_stats) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(s->set.device));
    GF_HIP(hipMemcpyAsync(out, s->d_chain_stats, sizeof(unsigned long long) * 8 * (size_t)s->nchains, hipMemcpyDeviceToHost, s->set.stream));
    GF_HIP(hipStreamSynchronize(s->set.stream));
    return GF_OK;
}

// diagnostics (not part of the ABI): the host thread's times of the process's LAST gf_sampler_run_to_host (HostSink::t), seconds / counts
int gf_internal_run_to_host_times(double out[8])
{
    if (!out) return GF_ERR_INVALID_ARG;
    for (int i = 0; i < 8; ++i) out[i] = g_last_run_to_host_times[i];
    return GF_OK;
}
int gf_internal_run_prologue_times(double out[4])
{
    if (!out) return GF_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = g_last_run_prologue[i];
    return GF_OK;
}

// diagnostics (not part of the ABI): out[0] = the launch shape of a small-ensemble BSM sampler (0 undecided, 1 per chain, 2 grid),
// out[1], out[2] = the probe's us per block of 16 steps, per chain / grid (0 when it has not run)
int gf_internal_sampler_shape(const gf_sampler* s, double out[3])
{
    if (!s || !out) return GF_ERR_INVALID_ARG;
    out[0] = grid_only(s) ? 2.0 : (double)s->shape; out[1] = s->probe_us[0]; out[2] = s->probe_us[1];
    return GF_OK;
}

int64_t gf_sampler_nstored(const gf_sampler* s) { return s ? s->nstored : -1; }
int64_t gf_sampler_iterations(const gf_sampler* s) { return s ? s->steps_since_reset : -1; }

// internal (gf_postprocess.hip): what chain post-processing needs of a sampler; gf_sampler itself stays private to this file
int gf_internal_sampler_chain_view(const gf_sampler* s, GfChainView* v)
{
    if (!s || !v) return GF_ERR_INVALID_ARG;
    *v = GfChainView{s->set.device, s->set.stream, s->set.cus, s->nchains, s->nwalkers, s->ndim, s->nstored, s->nstore_cap, s->d_chain, s->set.models[0], s->multi ? s->set.models.data() : nullptr,
                     s->d_lnp_chain, s->seed, s->d_stream_ids};
    return GF_OK;
}

// pos [nchains][nwalkers][ndim], lnprob [nchains][nwalkers] (either may be NULL)
int gf_sampler_get_state(gf_sampler* s, double* pos, double* lnprob)
{
    if (!s) return GF_ERR_INVALID_ARG;
    int rc = gf_model_sync(s->set.models[0]);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(s->set.device));
    const size_t nw = (size_t)s->nchains * s->nwalkers;
    hipStream_t st = s->set.stream;
    if (pos) GF_HIP(hipMemcpyAsync(pos, s->d_pos, sizeof(double) * nw * s->ndim, hipMemcpyDeviceToHost, st));
    if (lnprob) GF_HIP(hipMemcpyAsync(lnprob, s->d_lnp, sizeof(double) * nw, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

// chain [nchains][nstored][nwalkers][ndim], lnprob_chain [nchains][nstored][nwalkers],
// naccepted [nchains][nwalkers], nonunitary[1]; any may be NULL.
int gf_sampler_get_chain(gf_sampler* s, double* chain, double* lnprob_chain, uint32_t* naccepted, uint32_t* nonunitary)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;                           // in order behind the sampler's launches
    const size_t per = (size_t)s->nwalkers;
    if (s->nstored > 0) {
        // one strided copy per array: row = chain (stored prefix), device pitch = capacity stride
        const size_t row = sizeof(double) * per * s->ndim, lrow = sizeof(double) * per;
        // (gf_internal_d2h_2d: a plain strided copy below 16 MB, the pinned ring + host copy pool from there on)
        if (chain) {
            const int rc = gf_internal_d2h_2d(s->set.device, st, chain, row * s->nstored, s->d_chain, row * s->nstore_cap, row * s->nstored,
                                              (size_t)s->nchains);
            if (rc != GF_OK) return rc;
        }
        if (lnprob_chain) {
            const int rc = gf_internal_d2h_2d(s->set.device, st, lnprob_chain, lrow * s->nstored, s->d_lnp_chain, lrow * s->nstore_cap,
                                              lrow * s->nstored, (size_t)s->nchains);
            if (rc != GF_OK) return rc;
        }
    }
    if (naccepted)
        GF_HIP(hipMemcpyAsync(naccepted, s->d_naccept, sizeof(uint32_t) * (size_t)s->nchains * per, hipMemcpyDeviceToHost, st));
    if (nonunitary) GF_HIP(hipMemcpyAsync(nonunitary, s->d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

// The stored chain packed into caller-owned DEVICE buffers (the capacity padding of the sampler's own buffer removed):
// d_chain [nchains][nstored][nwalkers][ndim], d_lnprob_chain [nchains][nstored][nwalkers]; either may be NULL.
// Synchronous on return.  What a multi-GPU gather sends (gf_comm_allgather takes device pointers).
int gf_sampler_get_chain_device(gf_sampler* s, double* d_chain, double* d_lnprob_chain)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    if (s->nstored > 0) {
        const size_t row = sizeof(double) * (size_t)s->nwalkers * s->ndim, lrow = sizeof(double) * (size_t)s->nwalkers;
        if (d_chain)
            GF_HIP(hipMemcpy2DAsync(d_chain, row * s->nstored, s->d_chain, row * s->nstore_cap, row * s->nstored, s->nchains,
                                     hipMemcpyDeviceToDevice, st));
        if (d_lnprob_chain)
            GF_HIP(hipMemcpy2DAsync(d_lnprob_chain, lrow * s->nstored, s->d_lnp_chain, lrow * s->nstore_cap, lrow * s->nstored,
                                     s->nchains, hipMemcpyDeviceToDevice, st));
    }
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}


// mean [nchains][nstored][ndim]: the ensemble-averaged series whose integrated autocorrelation time the
// reference prints (golemflavor/mcmc.py:45-51 sampler.acor); reduced on the device, only the means cross PCIe.
int gf_sampler_walker_mean(gf_sampler* s, double* mean)
{
    if (!s || !mean) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->set.device));
    hipStream_t st = s->set.stream;
    if (s->nstored == 0) { GF_HIP(hipStreamSynchronize(st)); return GF_OK; }
    const size_t bytes = sizeof(double) * (size_t)s->nchains * s->nstored * s->ndim;
    double* d_mean = nullptr;
    GF_HIP(gf_cached_malloc((void**)&d_mean, bytes));
    hipError_t e = gf_launch_walker_mean(s->d_chain, s->nstore_cap, s->nstored, s->nchains, s->nwalkers, s->ndim, d_mean, st);
    if (e == hipSuccess) e = hipMemcpyAsync(mean, d_mean, bytes, hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipStreamSynchronize(st);
    (void)gf_cached_free(d_mean);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gf_hip_fail(e, "gf_sampler_walker_mean");
    return GF_OK;
}

}  // extern "C"
