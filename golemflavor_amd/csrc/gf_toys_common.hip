// gf_toys_common.hip -- the layer the realisation ensembles share (gf_toys_common.hpp; DESIGN.md sections 6j and 6l), for
// gf_toys.hip and gf_toys_binned.hip.
//
// The seed set: a seed point's prior sum, its unitarity verdict and its compositions do not depend on the measurement.  Per scale:
//   k_cube_draw     (gf_cube_runs.hip) nseed cube points of Philox counter (the scale's run id, SX_SEED_ITER, point, pair of coordinates): the points
//                   gf_simplex.hip's seeding draws for that run id
//   the bulk path   gf_model_lnprob_on with compositions and status: the verdicts with the bulk path's own arbitration
//   k_bsm_bins      an energy-resolved set only: gf_model_bins_on with that status, fr_bins [S][M][nb][3] (24 S M nb bytes), NaN for a
//                   row whose status is not OK
//   k_toy_prior     (gf_toys_prior.hpp) the prior sum lp_i of every seed by the evaluation kernels' own device function, -inf outside
//                   the box; counts the seeds the reference would have raised on, once per scale
// The tail of a selection, behind the likelihood's select kernel:
//   k_toy_merge     a lane per (scale, realisation) merges the parts' lists under gf_toys.hpp's total order, so the result does not
//                   depend on the split, and gathers the selected seeds' cube points: the starts of that realisation's polish
// No floating-point atomics, nothing order-dependent: the only atomic is the integer count of non-unitary seeds.
#include "gf_toys_common.hpp"

#include <vector>

#include "gf_toys_prior.hpp"

namespace {
using namespace gftoy;

// a lane per (scale, realisation): the parts' lists merged, the first K entries out
template <int KM>
__global__ __launch_bounds__(GF_BLOCK) void k_toy_merge(const ToyTail a, int64_t npairs)
{
    const int64_t p = (int64_t)blockIdx.x * GF_BLOCK + threadIdx.x;
    if (p >= npairs) return;
    Best<KM> best;
    best.clear();
    const int64_t at = p * a.nparts * KM;
    for (int e = 0; e < a.nparts * KM; ++e) best.offer(a.part_s[at + e], a.part_i[at + e]);
    const int64_t s = p / a.T;
    int count = 0;
#pragma unroll
    for (int j = 0; j < KM; ++j) {                                   // unrolled whole (no early exit): the list stays in registers
        if (j < a.K) {
            const int32_t idx = best.i[j];
            const bool have = idx != NO_SEED;
            count += have;
            a.out_index[p * a.K + j] = have ? idx : -1;
            a.out_score[p * a.K + j] = best.s[j];
            if (a.out_cube)
                for (int d = 0; d < a.N; ++d)
                    a.out_cube[(p * a.K + j) * a.N + d] = have ? a.seed_u[(s * a.M + idx) * a.N + d] : gf_nan();
        }
    }
    a.out_count[p] = count;
}

}  // namespace

int toy_seeds_create(void** out, gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed,
                     uint64_t seed, bool binned, const char* who, const char* seed_fn)
{
    if (!models || !cols || !bases || !out || nscales < 1 || nscales > 65535 || nscan < 1 || nscan > GF_MAX_DIM || nseed < 1 ||
        nseed > (1 << 22))
        return GF_ERR_INVALID_ARG;
    *out = nullptr;
    ToySeedSet* t = new (std::nothrow) ToySeedSet();
    if (!t) return GF_ERR_ALLOC;
    int rc = cube_runs_create(t->rs, t->a, models, nscales, nscan, cols, bases, seed, who);
    if (rc != GF_OK) { delete t; return rc; }
    if (t->rs.set.kind == GF_LLH_TABLE)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models carry a tabulated likelihood; a realisation of a table is not defined", who);
    else if (binned && t->rs.set.kind != GF_LLH_BINNED)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models carry no binned measurement; gf_toys_create seeds the flux-averaged Gaussian likelihood", who);
    else if (!binned && t->rs.set.kind == GF_LLH_BINNED)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models carry a binned measurement; realisations are of the flux-averaged Gaussian likelihood", who);
    else if (!binned && t->rs.set.mode != MODE_SM_GAUSS && t->rs.set.mode != MODE_BSM_GAUSS)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models have no Gaussian measurement (mode %d)", who, t->rs.set.mode);
    t->nseed = nseed;
    t->seed_fn = seed_fn;
    for (int r = 0; r < nscales && rc == GF_OK; ++r) {
        const GfCommon* c; const GfBsm* tb; const double* pt; int device, cus, nb;
        rc = gf_model_constants(models[r], &c, &tb, &pt, &device, &cus, &nb);
        if (rc != GF_OK) break;
        if (r == 0) { t->nbins = binned ? nb : 0; t->offset = c->offset; }
        // realisations shared by the scales are scored once per scale with one set of constants and one offset
        if (binned && (nb != t->nbins || nb < 1 || nb > GF_MAX_BINS))
            rc = gf_fail_msg(GF_ERR_INVALID_ARG, "%s: model %d has %d energy bins, model 0 has %d", who, r, nb, t->nbins);
        else if (!(c->offset == t->offset))
            rc = gf_fail_msg(GF_ERR_INVALID_ARG, "%s: model %d has another likelihood offset than model 0", who, r);
    }
    if (rc != GF_OK) { toy_seeds_destroy(t); return rc; }
    const size_t S = nscales, M = nseed;
    hipError_t e = hipSuccess;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    al((void**)&t->d_u, sizeof(double) * S * M * nscan);
    al((void**)&t->d_theta, sizeof(double) * S * M * t->a.ndim);
    al((void**)&t->d_lnl, sizeof(double) * S * M);
    al((void**)&t->d_fr, sizeof(double) * S * M * 3);
    if (binned) al((void**)&t->d_frb, sizeof(double) * S * M * 3 * t->nbins);
    al((void**)&t->d_st, sizeof(int32_t) * S * M);
    al((void**)&t->d_lp, sizeof(double) * S * M);
    al((void**)&t->d_nonunit, sizeof(unsigned int) * S);
    if (e != hipSuccess) { rc = gf_hip_fail(e, who); toy_seeds_destroy(t); return rc; }
    *out = t;
    return GF_OK;
}

void toy_seeds_destroy(ToySeedSet* t)
{
    if (!t) return;
    cube_runs_free(t->rs, t->a);
    void* ptrs[] = {t->d_u, t->d_theta, t->d_lnl, t->d_fr, t->d_frb, t->d_st, t->d_lp, t->d_nonunit};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete t;
}

int toy_seeds_set_ids(ToySeedSet* t, const uint64_t* ids, const char* late)
{
    if (!t || !ids) return GF_ERR_INVALID_ARG;
    return cube_runs_set_ids(t->rs, t->a, ids, late);
}

int toy_seeds_ready(const ToySeedSet& t, const char* who)
{
    if (!t.seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: after %s", who, t.seed_fn);
    GF_HIP(hipSetDevice(t.rs.set.device));
    return GF_OK;
}

int toy_seeds_seed(ToySeedSet* t, uint32_t* nonunitary, const char* who)
{
    if (!t) return GF_ERR_INVALID_ARG;
    if (t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the seeds have been drawn", who);
    GF_HIP(hipSetDevice(t->rs.set.device));
    if (const int rc = cube_runs_begin(t->rs, who)) return rc;
    const GfCubeRuns& a = t->a;
    const int n = t->nseed;
    hipStream_t st = t->rs.set.stream;
    const dim3 grid((unsigned)((n + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    cube_runs_draw_points(t->rs, a, SX_SEED_ITER, n, t->d_u, t->d_theta);
    GF_HIP(hipGetLastError());
    for (int r = 0; r < a.nruns; ++r) {
        const size_t at = (size_t)r * n;
        int rc = gf_model_lnprob_on(t->rs.set.models[r], st, t->d_theta + at * a.ndim, GF_LAYOUT_AOS, n, t->d_lnl + at, t->d_fr + at * 3, t->d_st + at);
        if (rc == GF_OK && t->d_frb)
            rc = gf_model_bins_on(t->rs.set.models[r], st, t->d_theta + at * a.ndim, GF_LAYOUT_AOS, n, t->d_frb + at * 3 * t->nbins, 0, t->d_st + at);
        if (rc != GF_OK) return rc;
    }
    GF_HIP(hipMemsetAsync(t->d_nonunit, 0, sizeof(unsigned int) * a.nruns, st));
    // an energy-resolved set's models are BSM models (gf_model_bins_on has refused any other)
    if (t->d_frb || t->rs.set.mode == MODE_BSM_GAUSS) hipLaunchKernelGGL(k_toy_prior<true>, grid, dim3(GF_BLOCK), 0, st, a, n, t->d_theta, t->d_st, t->d_lp, t->d_nonunit);
    else hipLaunchKernelGGL(k_toy_prior<false>, grid, dim3(GF_BLOCK), 0, st, a, n, t->d_theta, t->d_st, t->d_lp, t->d_nonunit);
    GF_HIP(hipGetLastError());
    std::vector<unsigned int> nu(a.nruns);
    GF_HIP(hipMemcpyAsync(nu.data(), t->d_nonunit, sizeof(unsigned int) * a.nruns, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    const int rc = gf_internal_check_overflow(t->rs.set.device, st);
    if (rc != GF_OK) return rc;
    if (nonunitary) for (int r = 0; r < a.nruns; ++r) nonunitary[r] = nu[r];
    t->seeded = 1;
    t->rs.initialised = 1;
    return GF_OK;
}

int toy_seeds_get(ToySeedSet* t, int scale, double* cube, double* lnprob, double* lp, double* fr, double* fr_bins, int32_t* status, const char* who)
{
    if (!t || scale < 0 || scale >= t->a.nruns) return GF_ERR_INVALID_ARG;
    const int rc = toy_seeds_ready(*t, who);
    if (rc != GF_OK) return rc;
    const size_t M = t->nseed, at = (size_t)scale * M, per = 3 * (size_t)t->nbins;
    hipStream_t st = t->rs.set.stream;
    if (cube) GF_HIP(hipMemcpyAsync(cube, t->d_u + at * t->a.nscan, sizeof(double) * M * t->a.nscan, hipMemcpyDeviceToHost, st));
    if (lnprob) GF_HIP(hipMemcpyAsync(lnprob, t->d_lnl + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (lp) GF_HIP(hipMemcpyAsync(lp, t->d_lp + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (fr) GF_HIP(hipMemcpyAsync(fr, t->d_fr + at * 3, sizeof(double) * M * 3, hipMemcpyDeviceToHost, st));
    if (fr_bins) GF_HIP(hipMemcpyAsync(fr_bins, t->d_frb + at * per, sizeof(double) * M * per, hipMemcpyDeviceToHost, st));
    if (status) GF_HIP(hipMemcpyAsync(status, t->d_st + at, sizeof(int32_t) * M, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

int toy_select_run(ToyTail& a, int S, hipStream_t st, ToySelectLaunch select, int32_t* index, double* score, int32_t* count, double* cube,
                   const char* who)
{
    const int KM = a.K <= 1 ? 1 : a.K <= 4 ? 4 : MAX_STARTS;
    a.nparts = (a.M + CHUNK - 1) / CHUNK;
    const size_t pairs = (size_t)S * a.T, ent = pairs * a.nparts * KM, sel = pairs * a.K;
    GfScratch scratch(GF_MEM_DRIVER);
    scratch.take(&a.part_s, sizeof(double) * ent, who);
    scratch.take(&a.part_i, sizeof(int32_t) * ent, who);
    scratch.take(&a.out_index, sizeof(int32_t) * sel, who);
    scratch.take(&a.out_score, sizeof(double) * sel, who);
    scratch.take(&a.out_count, sizeof(int32_t) * pairs, who);
    a.out_cube = nullptr;
    if (a.seed_u && cube) scratch.take(&a.out_cube, sizeof(double) * sel * a.N, who);
    if (scratch.failed != GF_OK) return scratch.failed;
    select(a, KM, S, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((pairs + GF_BLOCK - 1) / GF_BLOCK));
        if (KM == 1) hipLaunchKernelGGL(k_toy_merge<1>, grid, dim3(GF_BLOCK), 0, st, a, (int64_t)pairs);
        else if (KM == 4) hipLaunchKernelGGL(k_toy_merge<4>, grid, dim3(GF_BLOCK), 0, st, a, (int64_t)pairs);
        else hipLaunchKernelGGL(k_toy_merge<MAX_STARTS>, grid, dim3(GF_BLOCK), 0, st, a, (int64_t)pairs);
        e = hipGetLastError();
    }
    auto down = [&](void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && dst) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    };
    down(index, a.out_index, sizeof(int32_t) * sel);
    down(score, a.out_score, sizeof(double) * sel);
    down(count, a.out_count, sizeof(int32_t) * pairs);
    if (a.out_cube) down(cube, a.out_cube, sizeof(double) * sel * a.N);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e != hipSuccess ? gf_hip_fail(e, who) : GF_OK;
}

int toy_select_alone(int device, ToyTail& a, ToySelectLaunch select, const ToyUpload* blocks, int nblocks, int32_t* index, double* score,
                     int32_t* count, const char* who)
{
    int cus = 0;
    int rc = pool_device(device, &cus);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(device));
    void* stv = nullptr;
    rc = gf_internal_borrow_stream(device, &stv);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stv;
    {
        GfScratch scratch(GF_MEM_DRIVER);
        std::vector<char*> d(nblocks, nullptr);
        for (int b = 0; b < nblocks; ++b) scratch.take(&d[b], blocks[b].bytes, who);
        rc = scratch.failed;
        hipError_t e = hipSuccess;
        for (int b = 0; b < nblocks && rc == GF_OK && e == hipSuccess; ++b) {
            e = hipMemcpyAsync(d[b], blocks[b].host, blocks[b].bytes, hipMemcpyHostToDevice, st);
            *blocks[b].dev = d[b];
        }
        if (rc == GF_OK && e != hipSuccess) rc = gf_hip_fail(e, who);
        if (rc == GF_OK) rc = toy_select_run(a, 1, st, select, index, score, count, nullptr, who);
        (void)hipStreamSynchronize(st);                                   // idle before the scratch and the stream go back
    }
    gf_internal_return_stream(device, stv);
    return rc;
}
