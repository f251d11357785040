// gf_toys.hip -- the shared seeding of a realisation ensemble: many mock measurements of one Gaussian
// measurement profiled at every new-physics scale, with the scales' seed points drawn and propagated once.
//
// A seed point's composition, prior sum and unitarity verdict do not depend on the measurement; only the Gaussian block of lnprob does
// (gf_reweight.hip uses the same fact for stored chains).  Per scale (one run of a run set, gf_cube_runs.hpp):
//   k_cube_draw     nseed cube points of Philox counter (the scale's run id, SX_SEED_ITER, point, pair of coordinates): the points
//                   gf_simplex.hip's seeding draws for that run id
//   the bulk path   gf_model_lnprob_on with compositions and status: the verdicts with the bulk path's own arbitration
//   k_toy_prior     (gf_toys_prior.hpp) the prior sum lp_i of every seed by the evaluation kernels' own device function (lnprior / lnprior_tab), -inf
//                   outside the box; counts the seeds the reference would have raised on, once per scale
// and per (scale, realisation):
//   k_toy_select    a lane owns a realisation (its constants in registers); the workgroup streams a part of the seed range through
//                   LDS, every lane reading the same seed (a broadcast), and each lane keeps the best of its part in registers
//                   (gf_toys.hpp: score, order, list); the seed range is split over blockIdx.y
//   k_toy_merge     a lane per (scale, realisation) merges the parts' lists under the same total order, so the result does not depend
//                   on the split, and gathers the selected seeds' cube points: the starts of that realisation's polish
//                   (gf_simplex.hip with nseed = 0 and gf_toys_set_measurements)
// No floating-point atomics, nothing order-dependent: the only atomic is the integer count of non-unitary seeds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "gf_cube_runs.hpp"
#include "gf_pool.h"
#include "gf_toys.hpp"
#include "gf_toys_prior.hpp"

namespace {
using namespace gftoy;

constexpr int TOY_LANES = 64;            // realisations per workgroup of k_toy_select: one wave
constexpr int TOY_TILE = 256;            // seeds staged in LDS at a time: {lp, fr[3]} each, 8 KiB
static_assert(MAX_STARTS == GF_TOY_MAX_STARTS, "gf_toys.hpp states the public limit");
static_assert(STATUS_NON_UNITARY == GF_ST_NON_UNITARY && STATUS_NON_UNITARY == ST_NON_UNITARY, "gf_toys.hpp states the public status");
static_assert(CHUNK % TOY_TILE == 0, "a part of the seed range is whole tiles");

struct DevLogOfExp {
    __device__ __forceinline__ double operator()(double x) const { return gfdev::log_of_exp(x); }
};

struct ToySelArgs {
    const double* lp;                   // [S][M]
    const double* fr;                   // [S][M][3]
    const int32_t* st;                  // [S][M]
    const Meas* meas;                   // [S][T], or [T] shared by the scales (meas_stride = 0)
    int64_t meas_stride;
    int32_t M, T, nparts, K;
    double* part_s;                     // [S][T][nparts][KM]
    int32_t* part_i;
    const double* seed_u;               // [S][M][N], NULL: no cube points
    int32_t N;
    int32_t* out_index;                 // [S][T][K], -1 behind the count
    double* out_score;                  // [S][T][K], -inf behind the count
    int32_t* out_count;                 // [S][T]
    double* out_cube;                   // [S][T][K][N], NaN behind the count (NULL without seed_u)
    double* all_scores;                 // k_toy_score: [S][T][M]
};

// blockIdx = (block of TOY_LANES realisations, part of the seed range, scale)
template <int KM>
__global__ __launch_bounds__(TOY_LANES) void k_toy_select(const ToySelArgs a)
{
    __shared__ __attribute__((aligned(16))) double tile[TOY_TILE][4];
    const int s = blockIdx.z, part = blockIdx.y;
    const int t = blockIdx.x * TOY_LANES + threadIdx.x;
    const bool live = t < a.T;
    const Meas g = a.meas[(int64_t)s * a.meas_stride + (live ? t : 0)];
    Best<KM> best;
    best.clear();
    const int i0 = part * CHUNK;
    const int i1 = i0 + CHUNK < a.M ? i0 + CHUNK : a.M;
    const double* lp = a.lp + (int64_t)s * a.M;
    const double* fr = a.fr + (int64_t)s * a.M * 3;
    const int32_t* st = a.st + (int64_t)s * a.M;
    for (int base = i0; base < i1; base += TOY_TILE) {
        const int nt = i1 - base < TOY_TILE ? i1 - base : TOY_TILE;
        __syncthreads();                                               // the previous tile has been read
        for (int j = threadIdx.x; j < nt; j += TOY_LANES) {
            const int i = base + j;
            tile[j][0] = seed_lp(lp[i], st[i]);
            tile[j][1] = fr[3 * (int64_t)i]; tile[j][2] = fr[3 * (int64_t)i + 1]; tile[j][3] = fr[3 * (int64_t)i + 2];
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {                                // uniform: every lane reads the same seed
            const double2 p = *reinterpret_cast<const double2*>(&tile[j][0]);
            const double2 q = *reinterpret_cast<const double2*>(&tile[j][2]);
            best.offer(score(p.x, p.y, q.x, q.y, g, DevLogOfExp()), base + j);
        }
    }
    if (!live) return;
    const int64_t at = (((int64_t)s * a.T + t) * a.nparts + part) * KM;
#pragma unroll
    for (int j = 0; j < KM; ++j) { a.part_s[at + j] = best.s[j]; a.part_i[at + j] = best.i[j]; }
}

// a lane per (scale, realisation): the parts' lists merged, the first K entries out
template <int KM>
__global__ __launch_bounds__(GF_BLOCK) void k_toy_merge(const ToySelArgs a, int64_t npairs)
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

// every score, all_scores [S][T][M]: what the selection ranks (the tests hold it to the models' bulk lnprob)
__global__ __launch_bounds__(GF_BLOCK) void k_toy_score(const ToySelArgs a)
{
    const int s = blockIdx.z, t = blockIdx.y;
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    if (i >= a.M) return;
    const Meas g = a.meas[(int64_t)s * a.meas_stride + t];
    const int64_t at = (int64_t)s * a.M + i;
    a.all_scores[((int64_t)s * a.T + t) * a.M + i] = score(seed_lp(a.lp[at], a.st[at]), a.fr[3 * at], a.fr[3 * at + 1], a.fr[3 * at + 2], g, DevLogOfExp());
}

template <int KM>
hipError_t launch_select_km(const ToySelArgs& a, int S, hipStream_t st)
{
    const dim3 grid((unsigned)((a.T + TOY_LANES - 1) / TOY_LANES), (unsigned)a.nparts, (unsigned)S);
    hipLaunchKernelGGL(k_toy_select<KM>, grid, dim3(TOY_LANES), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t npairs = (int64_t)S * a.T;
    hipLaunchKernelGGL(k_toy_merge<KM>, dim3((unsigned)((npairs + GF_BLOCK - 1) / GF_BLOCK)), dim3(GF_BLOCK), 0, st, a, npairs);
    return hipGetLastError();
}

inline int toy_km(int K) { return K <= 1 ? 1 : K <= 4 ? 4 : MAX_STARTS; }

// The selection of S scales' seeds under T realisations on `st`: the device inputs of `a` (lp, fr, st, meas, seed_u) are the caller's, the
// parts' lists and the outputs are scratch of this call, copied to the host arrays (NULL = skip) before it returns.
int toy_select_run(ToySelArgs a, int S, hipStream_t st, int32_t* index, double* score, int32_t* count, double* cube, const char* who)
{
    const int KM = toy_km(a.K);
    a.nparts = (a.M + CHUNK - 1) / CHUNK;
    const size_t pairs = (size_t)S * a.T, ent = pairs * a.nparts * KM, sel = pairs * a.K;
    GfScratch scratch;
    scratch.take(&a.part_s, sizeof(double) * ent, who);
    scratch.take(&a.part_i, sizeof(int32_t) * ent, who);
    scratch.take(&a.out_index, sizeof(int32_t) * sel, who);
    scratch.take(&a.out_score, sizeof(double) * sel, who);
    scratch.take(&a.out_count, sizeof(int32_t) * pairs, who);
    a.out_cube = nullptr;
    if (a.seed_u && cube) scratch.take(&a.out_cube, sizeof(double) * sel * a.N, who);
    if (scratch.failed != GF_OK) return scratch.failed;
    hipError_t e = KM == 1 ? launch_select_km<1>(a, S, st) : KM == 4 ? launch_select_km<4>(a, S, st) : launch_select_km<MAX_STARTS>(a, S, st);
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

// the realisations' constants on the host: [n] of Meas from bf [n][3], smearing [n] and offset[k * offset_stride]
int toy_measurements(const double* bf, const double* smearing, size_t n, const double* offset, size_t per_offset, std::vector<Meas>& out,
                     const char* who)
{
    out.resize(n);
    for (size_t k = 0; k < n; ++k) {
        const double sm = smearing[k];
        if (!(sm > 0.0) || !std::isfinite(sm) || !std::isfinite(bf[3 * k]) || !std::isfinite(bf[3 * k + 1]) || !std::isfinite(bf[3 * k + 2]))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: realisation %zu needs a finite measurement and a smearing > 0", who, k);
        Meas& g = out[k];
        double inv_smear, c0;
        for (int d = 0; d < 3; ++d) g.m[d] = bf[3 * k + d];
        gf_internal_gauss_consts(sm, &inv_smear, &c0, &g.mh, &g.k);
        if (!std::isfinite(g.mh) || !std::isfinite(g.k))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the smearing of realisation %zu is outside the range of the Gaussian's constants", who, k);
        g.offset = offset[per_offset ? k / per_offset : 0];
    }
    return GF_OK;
}

}  // namespace

struct gf_toys {
    GfCubeRunsHost rs;
    GfCubeRuns a = {};
    int nseed = 0, seeded = 0;
    std::vector<double> offset;         // [nscales] the scale models' offsets
    double* d_u = nullptr;              // [S][M][N]
    double* d_theta = nullptr;          // [S][M][ndim]
    double* d_lnl = nullptr;            // [S][M] the scale models' own lnprob (under the models' measurement)
    double* d_fr = nullptr;             // [S][M][3]
    int32_t* d_st = nullptr;            // [S][M]
    double* d_lp = nullptr;             // [S][M]
    unsigned int* d_nonunit = nullptr;  // [S]
};

namespace {
// the measurements of a gf_toys call on the device; `meas` is released by the caller's scratch
int toys_upload_meas(gf_toys* t, const double* bf, int per_scale, const double* smearing, int ntoys, GfScratch& scratch, ToySelArgs& a, const char* who)
{
    const size_t S = t->a.nruns, n = (per_scale ? S : 1) * (size_t)ntoys;
    std::vector<double> sm(n);
    for (size_t k = 0; k < n; ++k) sm[k] = smearing[k % ntoys];
    std::vector<Meas> hm;
    // a scale's realisations carry that scale's offset; shared realisations the offset of scale 0, which every scale's model shares
    // with it (checked at create)
    const int rc = toy_measurements(bf, sm.data(), n, t->offset.data(), per_scale ? (size_t)ntoys : 0, hm, who);
    if (rc != GF_OK) return rc;
    Meas* d = nullptr;
    if (scratch.take(&d, sizeof(Meas) * n, who) != GF_OK) return scratch.failed;
    GF_HIP(hipMemcpyAsync(d, hm.data(), sizeof(Meas) * n, hipMemcpyHostToDevice, t->rs.stream));
    GF_HIP(hipStreamSynchronize(t->rs.stream));                          // hm goes out of scope
    a = ToySelArgs{};
    a.lp = t->d_lp; a.fr = t->d_fr; a.st = t->d_st; a.meas = d; a.meas_stride = per_scale ? ntoys : 0;
    a.M = t->nseed; a.T = ntoys; a.seed_u = t->d_u; a.N = t->a.nscan;
    return GF_OK;
}
}  // namespace

extern "C" {

int gf_toys_create(gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed, uint64_t seed,
                   gf_toys** out)
{
    if (!models || !cols || !bases || !out || nscales < 1 || nscales > 65535 || nscan < 1 || nscan > GF_MAX_DIM || nseed < 1 ||
        nseed > (1 << 22))
        return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_toys* t = new (std::nothrow) gf_toys();
    if (!t) return GF_ERR_ALLOC;
    int rc = cube_runs_create(t->rs, t->a, models, nscales, nscan, cols, bases, seed, "gf_toys_create");
    if (rc != GF_OK) { delete t; return rc; }
    if (t->rs.table)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_create: the models carry a tabulated likelihood; a realisation of a table is not defined");
    else if (t->rs.binned)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_create: the models carry a binned measurement; realisations are of the flux-averaged Gaussian likelihood");
    else if (t->rs.mode != MODE_SM_GAUSS && t->rs.mode != MODE_BSM_GAUSS)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_create: the models have no Gaussian measurement (mode %d)", t->rs.mode);
    t->nseed = nseed;
    t->offset.resize(nscales);
    for (int r = 0; r < nscales && rc == GF_OK; ++r) {
        const GfCommon* c; const GfBsm* tb; const double* pt; int device, cus, nb;
        rc = gf_model_constants(models[r], &c, &tb, &pt, &device, &cus, &nb);
        if (rc == GF_OK) t->offset[r] = c->offset;
        // realisations shared by the scales are scored once per scale with one set of constants
        if (rc == GF_OK && !(c->offset == t->offset[0]))
            rc = gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_create: model %d has another likelihood offset than model 0", r);
    }
    if (rc != GF_OK) { gf_toys_destroy(t); return rc; }
    const size_t S = nscales, M = nseed;
    hipError_t e = hipSuccess;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    al((void**)&t->d_u, sizeof(double) * S * M * nscan);
    al((void**)&t->d_theta, sizeof(double) * S * M * t->a.ndim);
    al((void**)&t->d_lnl, sizeof(double) * S * M);
    al((void**)&t->d_fr, sizeof(double) * S * M * 3);
    al((void**)&t->d_st, sizeof(int32_t) * S * M);
    al((void**)&t->d_lp, sizeof(double) * S * M);
    al((void**)&t->d_nonunit, sizeof(unsigned int) * S);
    if (e != hipSuccess) { rc = gf_hip_fail(e, "gf_toys_create"); gf_toys_destroy(t); return rc; }
    *out = t;
    return GF_OK;
}

void gf_toys_destroy(gf_toys* t)
{
    if (!t) return;
    cube_runs_free(t->rs, t->a);
    void* ptrs[] = {t->d_u, t->d_theta, t->d_lnl, t->d_fr, t->d_st, t->d_lp, t->d_nonunit};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete t;
}

int gf_toys_set_run_ids(gf_toys* t, const uint64_t* ids)
{
    if (!t || !ids) return GF_ERR_INVALID_ARG;
    return cube_runs_set_ids(t->rs, t->a, ids, "gf_toys_set_run_ids: before gf_toys_seed");
}

int gf_toys_seed(gf_toys* t, uint32_t* nonunitary)
{
    if (!t) return GF_ERR_INVALID_ARG;
    if (t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_seed: the seeds have been drawn");
    GF_HIP(hipSetDevice(t->rs.device));
    const GfCubeRuns& a = t->a;
    const int n = t->nseed;
    hipStream_t st = t->rs.stream;
    const dim3 grid((unsigned)((n + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(k_cube_draw, grid, dim3(GF_BLOCK), 0, st, a, SX_SEED_ITER, n, t->d_u, t->d_theta);
    GF_HIP(hipGetLastError());
    for (int r = 0; r < a.nruns; ++r) {
        const size_t at = (size_t)r * n;
        const int rc = gf_model_lnprob_on(t->rs.models[r], st, t->d_theta + at * a.ndim, GF_LAYOUT_AOS, n, t->d_lnl + at, t->d_fr + at * 3,
                                          t->d_st + at);
        if (rc != GF_OK) return rc;
    }
    GF_HIP(hipMemsetAsync(t->d_nonunit, 0, sizeof(unsigned int) * a.nruns, st));
    if (t->rs.mode == MODE_BSM_GAUSS) hipLaunchKernelGGL(k_toy_prior<true>, grid, dim3(GF_BLOCK), 0, st, a, n, t->d_theta, t->d_st, t->d_lp, t->d_nonunit);
    else hipLaunchKernelGGL(k_toy_prior<false>, grid, dim3(GF_BLOCK), 0, st, a, n, t->d_theta, t->d_st, t->d_lp, t->d_nonunit);
    GF_HIP(hipGetLastError());
    std::vector<unsigned int> nu(a.nruns);
    GF_HIP(hipMemcpyAsync(nu.data(), t->d_nonunit, sizeof(unsigned int) * a.nruns, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    const int rc = gf_internal_check_overflow(t->rs.device, st);
    if (rc != GF_OK) return rc;
    if (nonunitary) for (int r = 0; r < a.nruns; ++r) nonunitary[r] = nu[r];
    t->seeded = 1;
    t->rs.initialised = 1;
    return GF_OK;
}

int gf_toys_get_seeds(gf_toys* t, int scale, double* cube, double* lnprob, double* lp, double* fr, int32_t* status)
{
    if (!t || scale < 0 || scale >= t->a.nruns) return GF_ERR_INVALID_ARG;
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_get_seeds: after gf_toys_seed");
    GF_HIP(hipSetDevice(t->rs.device));
    const size_t M = t->nseed, at = (size_t)scale * M;
    hipStream_t st = t->rs.stream;
    if (cube) GF_HIP(hipMemcpyAsync(cube, t->d_u + at * t->a.nscan, sizeof(double) * M * t->a.nscan, hipMemcpyDeviceToHost, st));
    if (lnprob) GF_HIP(hipMemcpyAsync(lnprob, t->d_lnl + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (lp) GF_HIP(hipMemcpyAsync(lp, t->d_lp + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (fr) GF_HIP(hipMemcpyAsync(fr, t->d_fr + at * 3, sizeof(double) * M * 3, hipMemcpyDeviceToHost, st));
    if (status) GF_HIP(hipMemcpyAsync(status, t->d_st + at, sizeof(int32_t) * M, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

int gf_toys_select(gf_toys* t, const double* bf, int per_scale, const double* smearing, int ntoys, int K, double* cube, int32_t* index,
                   double* score, int32_t* count)
{
    if (!t || !bf || !smearing || ntoys < 1 || ntoys > (1 << 20) || (per_scale != 0 && per_scale != 1)) return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select: after gf_toys_seed");
    GF_HIP(hipSetDevice(t->rs.device));
    GfScratch scratch;
    ToySelArgs a;
    const int rc = toys_upload_meas(t, bf, per_scale, smearing, ntoys, scratch, a, "gf_toys_select");
    if (rc != GF_OK) return rc;
    a.K = K;
    return toy_select_run(a, t->a.nruns, t->rs.stream, index, score, count, cube, "gf_toys_select");
}

int gf_toys_scores(gf_toys* t, const double* bf, int per_scale, const double* smearing, int ntoys, double* scores)
{
    if (!t || !bf || !smearing || !scores || ntoys < 1 || ntoys > 65535 || (per_scale != 0 && per_scale != 1)) return GF_ERR_INVALID_ARG;
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_scores: after gf_toys_seed");
    GF_HIP(hipSetDevice(t->rs.device));
    GfScratch scratch;
    ToySelArgs a;
    const int rc = toys_upload_meas(t, bf, per_scale, smearing, ntoys, scratch, a, "gf_toys_scores");
    if (rc != GF_OK) return rc;
    const size_t n = (size_t)t->a.nruns * ntoys * t->nseed;
    if (scratch.take(&a.all_scores, sizeof(double) * n, "gf_toys_scores") != GF_OK) return scratch.failed;
    const dim3 grid((unsigned)((a.M + GF_BLOCK - 1) / GF_BLOCK), (unsigned)ntoys, (unsigned)t->a.nruns);
    hipLaunchKernelGGL(k_toy_score, grid, dim3(GF_BLOCK), 0, t->rs.stream, a);
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(scores, a.all_scores, sizeof(double) * n, hipMemcpyDeviceToHost, t->rs.stream));
    GF_HIP(hipStreamSynchronize(t->rs.stream));
    return GF_OK;
}

int gf_toy_select(int device, const double* lp, const double* fr, const int32_t* status, int nseed, const double* bf, const double* smearing,
                  double offset, int ntoys, int K, int32_t* out_index, double* out_score, int32_t* out_count)
{
    if (!lp || !fr || !status || !bf || !smearing || nseed < 1 || nseed > (1 << 22) || ntoys < 1 || ntoys > (1 << 20))
        return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toy_select: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    std::vector<Meas> hm;
    int rc = toy_measurements(bf, smearing, (size_t)ntoys, &offset, 0, hm, "gf_toy_select");
    if (rc != GF_OK) return rc;
    int cus = 0;
    rc = pool_device(device, &cus);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(device));
    void* stv = nullptr;
    rc = gf_internal_borrow_stream(device, &stv);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stv;
    {
        GfScratch scratch;
        const size_t M = nseed;
        double *d_lp = nullptr, *d_fr = nullptr;
        int32_t* d_st = nullptr;
        Meas* d_meas = nullptr;
        scratch.take(&d_lp, sizeof(double) * M, "gf_toy_select");
        scratch.take(&d_fr, sizeof(double) * M * 3, "gf_toy_select");
        scratch.take(&d_st, sizeof(int32_t) * M, "gf_toy_select");
        scratch.take(&d_meas, sizeof(Meas) * ntoys, "gf_toy_select");
        rc = scratch.failed;
        hipError_t e = hipSuccess;
        auto up = [&](void* dst, const void* src, size_t bytes) { if (rc == GF_OK && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
        up(d_lp, lp, sizeof(double) * M);
        up(d_fr, fr, sizeof(double) * M * 3);
        up(d_st, status, sizeof(int32_t) * M);
        up(d_meas, hm.data(), sizeof(Meas) * ntoys);
        if (rc == GF_OK && e != hipSuccess) rc = gf_hip_fail(e, "gf_toy_select");
        if (rc == GF_OK) {
            ToySelArgs a = {};
            a.lp = d_lp; a.fr = d_fr; a.st = d_st; a.meas = d_meas; a.meas_stride = 0; a.M = nseed; a.T = ntoys; a.K = K;
            rc = toy_select_run(a, 1, st, out_index, out_score, out_count, nullptr, "gf_toy_select");
        }
        (void)hipStreamSynchronize(st);                                   // idle before the scratch and the stream go back
    }
    gf_internal_return_stream(device, stv);
    return rc;
}

}  // extern "C"
