// gf_modelset.hip -- see gf_modelset.h.  Host code only: no kernel.
#include "gf_devcache.h"                // large device allocations are cached, not handed back to the driver
#include "gf_host.h"
#include "gf_modelset.h"

int gf_modelset_create(GfModelSet* set, gf_model* const* models, int nmodels, const char* who)
{
    void* stream;
    if (!models[0] || gf_model_internal(models[0], &set->c, &set->tb, &set->ptab, &stream, &set->device) != GF_OK) return GF_ERR_INVALID_ARG;
    set->stream = (hipStream_t)stream; set->ndim = set->c->ndim; set->mode = set->c->mode;
    const size_t nm = (size_t)nmodels;
    std::vector<GfCommon> hc(nm);
    std::vector<const GfBsm*> htb(nm);
    std::vector<const double*> hpt(nm), hbt(nm);
    set->h_ttabs.assign(nm, nullptr); set->h_tsides.assign(nm, 0);
    for (int r = 0; r < nmodels; ++r) {
        const GfCommon* c; int device, cus, nbins;
        if (!models[r] || gf_model_constants(models[r], &c, &htb[r], &hpt[r], &device, &cus, &nbins) != GF_OK || device != set->device ||
            c->ndim != set->ndim || c->mode != set->mode) {
            set->differs = r;
            return GF_ERR_INVALID_ARG;
        }
        hc[r] = *c;
        // pointer and side of a table are the model's of now (gf_modelset_refresh_tables); a binned table's address is the model's for
        // good: a measurement set later lands in the same table.  A model carries one of the two at most.
        set->h_tsides[r] = gf_model_table(models[r], &set->h_ttabs[r]);
        const int binned = gf_model_binned(models[r], &hbt[r]);
        set->carries.push_back(set->h_tsides[r] > 0 ? GF_LLH_TABLE : binned ? GF_LLH_BINNED : GF_LLH_FLUX);
        if (r == 0) set->cus = cus;
        if (nbins > set->nbins_max) set->nbins_max = nbins;
    }
    set->kind = set->carries[0];
    for (int k : set->carries)
        if (k != set->kind) { set->kind = GF_LLH_MIXED; return GF_ERR_INVALID_ARG; }
    set->models.assign(models, models + nmodels);
    // every transfer goes through the set's stream: a synchronous (null-stream) hipMemcpy / hipMemset issued while ANOTHER host
    // thread is capturing its sampler's graph fails and poisons that capture on this runtime
    hipError_t e = hipSetDevice(set->device);
    auto put = [&](void** d, const void* src, size_t bytes) {
        if (e == hipSuccess) e = gf_cached_malloc(d, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(*d, src, bytes, hipMemcpyHostToDevice, set->stream);
    };
    put((void**)&set->d_commons, hc.data(), sizeof(GfCommon) * nm);
    put((void**)&set->d_tbs, htb.data(), sizeof(void*) * nm);
    put((void**)&set->d_ptabs, hpt.data(), sizeof(void*) * nm);
    if (set->kind == GF_LLH_BINNED) put((void**)&set->d_btabs, hbt.data(), sizeof(void*) * nm);
    if (set->kind == GF_LLH_TABLE) {
        put((void**)&set->d_ttabs, set->h_ttabs.data(), sizeof(void*) * nm);
        put((void**)&set->d_tsides, set->h_tsides.data(), sizeof(int32_t) * nm);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(set->stream);          // the host vectors go out of scope
    if (e == hipSuccess) return GF_OK;
    gf_modelset_free(set);
    return gf_hip_fail(e, who);
}

int gf_modelset_refresh_tables(GfModelSet* set, const char* who)
{
    if (set->kind != GF_LLH_TABLE) return GF_OK;
    const size_t nm = set->models.size();
    bool changed = false;
    for (size_t r = 0; r < nm; ++r) {
        const double* d = nullptr;
        const int side = gf_model_table(set->models[r], &d);
        if (side <= 0) return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: model %d no longer carries a tabulated likelihood", who, (int)r);
        if (d != set->h_ttabs[r] || side != set->h_tsides[r]) { set->h_ttabs[r] = d; set->h_tsides[r] = side; changed = true; }
    }
    if (!changed) return GF_OK;
    GF_HIP(hipMemcpyAsync((void*)set->d_ttabs, set->h_ttabs.data(), sizeof(void*) * nm, hipMemcpyHostToDevice, set->stream));
    GF_HIP(hipMemcpyAsync(set->d_tsides, set->h_tsides.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice, set->stream));
    return GF_OK;
}

int gf_modelset_kind_differs(const GfModelSet* set, int* now)
{
    for (size_t r = 0; r < set->models.size(); ++r) {
        const int has = gf_model_table(set->models[r], nullptr) > 0 ? GF_LLH_TABLE : gf_model_binned(set->models[r], nullptr) ? GF_LLH_BINNED : GF_LLH_FLUX;
        if (has != set->kind) { if (now) *now = has; return (int)r; }
    }
    return -1;
}

void gf_modelset_mark(GfModelSet* set)
{
    set->marked.resize(set->models.size());
    for (size_t r = 0; r < set->models.size(); ++r) set->marked[r] = gf_model_likelihood_sets(set->models[r]);
}

int gf_modelset_replaced(const GfModelSet* set)
{
    for (size_t r = 0; r < set->marked.size() && r < set->models.size(); ++r)
        if (gf_model_likelihood_sets(set->models[r]) != set->marked[r]) return (int)r;
    return -1;
}

void gf_modelset_free(GfModelSet* set)
{
    if (set->stream) {
        (void)hipSetDevice(set->device);
        (void)hipStreamSynchronize(set->stream);
    }
    void* ptrs[] = {set->d_commons, (void*)set->d_tbs, (void*)set->d_ptabs, (void*)set->d_btabs, (void*)set->d_ttabs, set->d_tsides};
    for (void* p : ptrs) if (p) (void)gf_cached_free(p);
    set->d_commons = nullptr; set->d_tbs = nullptr; set->d_ptabs = nullptr; set->d_btabs = nullptr; set->d_ttabs = nullptr; set->d_tsides = nullptr;
    set->models.clear();
}
