// gf_cube_runs.hip -- the host layer of the cube runs (gf_cube_runs.hpp, which says what each function does) and k_cube_draw: compiled
// here once for the nested sampler, the maximiser and the realisation ensembles.  The layer's own device buffers and its arbitration
// queue come from the driver, not from the device cache (the device cache's table of allocators).
#include "gf_cube_runs.hpp"

namespace {
// n cube points per run (blockIdx.y), drawn uniformly (counter (run id, it, point, pair of coordinates)) into u [R][n][nscan]
// and mapped to theta [R][n][ndim]
__global__ __launch_bounds__(GF_BLOCK) void k_cube_draw(const GfCubeRuns a, uint32_t it, int n, double* u, double* theta)
{
    const int r = blockIdx.y;
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    if (i >= n) return;
    double v[GF_MAX_DIM];
    for (int p = 0; 2 * p < a.nscan; ++p) {
        double w[2];
        cube_uniform2(a, r, it, (uint32_t)i, (uint32_t)p, w);
        v[2 * p] = w[0];
        if (2 * p + 1 < a.nscan) v[2 * p + 1] = w[1];
    }
    double* dst = u + ((int64_t)r * n + i) * a.nscan;
    for (int d = 0; d < a.nscan; ++d) dst[d] = v[d];
    cube_to_theta(a, a.commons[r], r, v, theta + ((int64_t)r * n + i) * a.ndim);
}
}  // namespace

void cube_runs_free(GfCubeRunsHost& h, GfCubeRuns& a)
{
    gf_modelset_free(&h.set);
    void* ptrs[] = {h.d_btab_runs, h.d_run_ids, h.d_bases, h.d_state, h.d_ctl, a.pq, a.pend_rows};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    h.d_btab_runs = nullptr; h.d_run_ids = nullptr; h.d_bases = nullptr;
    h.d_state = nullptr; h.d_ctl = nullptr; a.pq = nullptr; a.pend_rows = nullptr;
}

int cube_runs_create(GfCubeRunsHost& h, GfCubeRuns& a, gf_model* const* models, int nruns, int nscan, const int32_t* cols,
                     const double* bases, uint64_t seed, const char* who)
{
    const GfModelSet& set = h.set;
    int rc = gf_modelset_create(&h.set, models, nruns, who);
    const int ndim = set.ndim;
    for (int d = 0; d < GF_MAX_DIM; ++d) a.slot[d] = -1;
    bool cols_ok = ndim > 0;                                              // (0: models[0] is unusable)
    for (int k = 0; k < nscan && cols_ok; ++k) {
        cols_ok = cols[k] >= 0 && cols[k] < ndim && a.slot[cols[k]] < 0;
        if (cols_ok) a.slot[cols[k]] = k;
    }
    if (!cols_ok) rc = GF_ERR_INVALID_ARG;
    else if (set.differs >= 0) rc = gf_fail_msg(GF_ERR_INVALID_ARG, "%s: every model must share device, ndim and mode with model 0", who);
    else if (set.kind == GF_LLH_MIXED) {
        const int nbinned = (int)std::count(set.carries.begin(), set.carries.end(), (int)GF_LLH_BINNED);
        const int ntable = (int)std::count(set.carries.begin(), set.carries.end(), (int)GF_LLH_TABLE);
        rc = nbinned ? gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d of the %d models carry a binned measurement; all of a set must, or none", who, nbinned, nruns)
                     : gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d of the %d models carry a tabulated likelihood; all of a set must, or none", who, ntable, nruns);
    }
    if (rc != GF_OK) { cube_runs_free(h, a); return rc; }
    a.seed = seed;
    a.nruns = nruns; a.nscan = nscan; a.ndim = ndim; a.nbins_max = set.nbins_max;
    const size_t R = nruns;
    std::vector<double> hb(R * GF_MAX_DIM, 0.0);
    for (size_t r = 0; r < R; ++r)
        for (int d = 0; d < ndim; ++d) hb[r * GF_MAX_DIM + d] = bases[r * ndim + d];
    std::vector<uint64_t> ids(R);
    for (size_t r = 0; r < R; ++r) ids[r] = r;
    GfStepState hs = {};
    hs.thin = 1;
    hipError_t e = hipSetDevice(set.device);
    auto put = [&](void** d, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(d, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(*d, src, bytes, hipMemcpyHostToDevice, set.stream);
    };
    put((void**)&h.d_run_ids, ids.data(), sizeof(uint64_t) * R);
    put((void**)&h.d_bases, hb.data(), sizeof(double) * R * GF_MAX_DIM);
    put((void**)&h.d_state, &hs, sizeof(hs));
    if (e == hipSuccess) e = hipStreamSynchronize(set.stream);            // the host vectors go out of scope
    if (e != hipSuccess) { rc = gf_hip_fail(e, who); cube_runs_free(h, a); return rc; }
    a.commons = set.d_commons; a.tbs = set.d_tbs; a.ptabs = set.d_ptabs; a.btabs = set.d_btabs; a.ttabs = set.d_ttabs; a.tsides = set.d_tsides;
    a.run_ids = h.d_run_ids; a.bases = h.d_bases;
    return GF_OK;
}

int cube_runs_begin(GfCubeRunsHost& h, const char* who)
{
    int now = GF_LLH_FLUX;
    const int differs = gf_modelset_kind_differs(&h.set, &now);
    if (differs >= 0)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: model %d now carries %s; a set keeps the likelihood its models carried when it was created (%s)",
                           who, differs, gf_likelihood_name(now), gf_likelihood_name(h.set.kind));
    if (h.initialised) {
        const int replaced = gf_modelset_replaced(&h.set);
        if (replaced >= 0)
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the likelihood of model %d was replaced after the set's runs began; a run that has begun does not change likelihood",
                               who, replaced);
        return GF_OK;
    }
    const int rc = gf_modelset_refresh_tables(&h.set, who);
    if (rc != GF_OK) return rc;
    gf_modelset_mark(&h.set);
    return GF_OK;
}

hipError_t cube_runs_alloc_queue(GfCubeRunsHost& h, GfCubeRuns& a, size_t w)
{
    if (h.set.mode != MODE_BSM_GAUSS) return hipSuccess;
    return gf_alloc_arb_queue(GF_MEM_DRIVER, w, h.set.stream, &a.pq, &a.pend_rows, &h.d_ctl);
}

void cube_runs_settle_args(const GfCubeRunsHost& h, const GfCubeRuns& a, int nwalkers, GfSettleArgs& sa)
{
    sa.state = h.d_state; sa.pq = a.pq; sa.pend_rows = a.pend_rows; sa.ctl = h.d_ctl;
    sa.nchains = a.nruns; sa.nwalkers = nwalkers; sa.ndim = a.ndim; sa.commons = h.set.d_commons; sa.tbs = h.set.d_tbs; sa.multi = 1;
}

int cube_runs_set_ids(GfCubeRunsHost& h, const GfCubeRuns& a, const uint64_t* ids, const char* late)
{
    if (h.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s", late);
    GF_HIP(hipSetDevice(h.set.device));
    GF_HIP(hipMemcpyAsync(h.d_run_ids, ids, sizeof(uint64_t) * (size_t)a.nruns, hipMemcpyHostToDevice, h.set.stream));
    GF_HIP(hipStreamSynchronize(h.set.stream));
    return GF_OK;
}

int cube_runs_set_measurements(GfCubeRunsHost& h, const GfCubeRuns& a, const double* bf, const double* smearing, const char* who)
{
    if (h.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: before the first run", who);
    if (h.set.kind == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry a tabulated likelihood, which has no Gaussian measurement to replace", who);
    if (h.set.kind == GF_LLH_BINNED)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry a binned measurement; a run's own measurement replaces the flux-averaged one only", who);
    if (h.set.mode != MODE_SM_GAUSS && h.set.mode != MODE_BSM_GAUSS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models have no Gaussian measurement (mode %d)", who, h.set.mode);
    const size_t R = a.nruns;
    std::vector<GfCommon> hc(R);
    for (size_t r = 0; r < R; ++r) {
        const double sm = smearing[r];
        if (!(sm > 0.0) || !std::isfinite(sm) || !std::isfinite(bf[3 * r]) || !std::isfinite(bf[3 * r + 1]) || !std::isfinite(bf[3 * r + 2]))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: run %zu needs a finite measurement and a smearing > 0", who, r);
        const GfCommon* c; const GfBsm* tb; const double* pt; int device, cus, nb;
        const int rc = gf_model_constants(h.set.models[r], &c, &tb, &pt, &device, &cus, &nb);
        if (rc != GF_OK) return rc;
        hc[r] = *c;
        for (int k = 0; k < 3; ++k) hc[r].bf[k] = bf[3 * r + k];
        gf_internal_gauss_consts(sm, &hc[r].inv_smear, &hc[r].gauss_c0, &hc[r].gauss_mh, &hc[r].gauss_k);
        if (!std::isfinite(hc[r].gauss_mh) || !std::isfinite(hc[r].gauss_k))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the smearing of run %zu is outside the range of the Gaussian's constants", who, r);
    }
    GF_HIP(hipSetDevice(h.set.device));
    GF_HIP(hipMemcpyAsync(h.set.d_commons, hc.data(), sizeof(GfCommon) * R, hipMemcpyHostToDevice, h.set.stream));
    GF_HIP(hipStreamSynchronize(h.set.stream));                              // hc goes out of scope
    return GF_OK;
}

int cube_runs_set_binned_measurements(GfCubeRunsHost& h, const GfCubeRuns& a, int nbins, const double* fr_bins, const double* sigma,
                                      const char* who)
{
    if (h.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: before the first run", who);
    if (h.set.kind == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry a tabulated likelihood, which has no binned measurement to replace", who);
    if (h.set.kind != GF_LLH_BINNED)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry no binned measurement; a run's own binned measurement replaces a model's", who);
    const size_t R = a.nruns, nb = nbins > 0 ? nbins : 0;
    for (size_t r = 0; r < R; ++r) {
        const GfCommon* c; const GfBsm* tb; const double* pt; int device, cus, mnb;
        const int rc = gf_model_constants(h.set.models[r], &c, &tb, &pt, &device, &cus, &mnb);
        if (rc != GF_OK) return rc;
        if (nbins != mnb) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: %d bins given, the model of run %zu has %d", who, nbins, r, mnb);
    }
    std::vector<double> tab(R * nb * GF_BINNED_STRIDE);
    std::vector<const double*> hbt(R);
    for (size_t r = 0; r < R; ++r)
        for (size_t k = 0; k < nb; ++k) {
            const double* f = fr_bins + (r * nb + k) * 3;
            const double sg = sigma[r * nb + k];
            if (!std::isfinite(f[0]) || !std::isfinite(f[1]) || !std::isfinite(f[2]) || !(sg > 0.0) || !std::isfinite(sg))
                return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: bin %zu of run %zu needs a finite composition and a width > 0", who, k, r);
            double inv_smear, c0;
            double* t = tab.data() + (r * nb + k) * GF_BINNED_STRIDE;
            t[0] = f[0]; t[1] = f[1]; t[2] = f[2];
            gf_internal_gauss_consts(sg, &inv_smear, &c0, &t[3], &t[4]);
            if (!std::isfinite(t[3]) || !std::isfinite(t[4]))
                return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the width of bin %zu of run %zu is outside the range of the Gaussian's constants", who, k, r);
        }
    GF_HIP(hipSetDevice(h.set.device));
    if (!h.d_btab_runs) GF_HIP(hipMalloc((void**)&h.d_btab_runs, sizeof(double) * tab.size()));
    for (size_t r = 0; r < R; ++r) hbt[r] = h.d_btab_runs + r * nb * GF_BINNED_STRIDE;
    GF_HIP(hipMemcpyAsync(h.d_btab_runs, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, h.set.stream));
    GF_HIP(hipMemcpyAsync((void*)h.set.d_btabs, hbt.data(), sizeof(void*) * R, hipMemcpyHostToDevice, h.set.stream));
    GF_HIP(hipStreamSynchronize(h.set.stream));                              // the host vectors go out of scope
    return GF_OK;
}

void cube_runs_draw_points(const GfCubeRunsHost& h, const GfCubeRuns& a, uint32_t it, int n, double* u, double* theta)
{
    const dim3 grid((unsigned)((n + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(k_cube_draw, grid, dim3(GF_BLOCK), 0, h.set.stream, a, it, n, u, theta);
}

int cube_runs_draw(const GfCubeRunsHost& h, const GfCubeRuns& a, uint32_t it, int n, double* u, double* theta, double* lnl,
                   int32_t* status)
{
    cube_runs_draw_points(h, a, it, n, u, theta);
    GF_HIP(hipGetLastError());
    for (int r = 0; r < a.nruns; ++r) {
        const int rc = gf_model_lnprob_on(h.set.models[r], h.set.stream, theta + (size_t)r * n * a.ndim, GF_LAYOUT_AOS, n,
                                          lnl + (size_t)r * n, nullptr, status + (size_t)r * n);
        if (rc != GF_OK) return rc;
    }
    return GF_OK;
}
