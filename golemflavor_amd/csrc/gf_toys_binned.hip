// gf_toys_binned.hip -- the shared seeding of a realisation ensemble under the energy-resolved likelihood: many
// mock measurements of one binned measurement profiled at every new-physics scale, with the scales' seed points drawn and propagated
// once.
//
// A seed point's prior sum, its unitarity verdict and its composition at every energy bin do not depend on the measurement; only the
// per-bin Gaussian terms do.  Per scale (one run of a run set, gf_cube_runs.hpp):
//   k_cube_draw     the nseed cube points gf_simplex.hip's seeding draws for that run id
//   the bulk path   gf_model_lnprob_on: the scale model's own binned lnprob and the status, the verdicts by the bulk path's arbitration
//   k_bsm_bins      gf_model_bins_on with that status: the compositions fr_bins [S][M][nb][3] (24 S M nb bytes), NaN for a row whose
//                   status is not OK
//   k_toy_prior     the prior sum lp_i (gf_toys_prior.hpp), and the count of the seeds the reference would have raised on
// and per (scale, realisation):
//   k_toyb_select   a lane owns a realisation and keeps its best seeds in registers.  A realisation has 5 nb constants and a seed
//                   1 + 3 nb doubles, so neither sits in registers whole: the workgroup stages a tile of TOYB_TILE seeds in LDS, the bin
//                   loop runs outermost, a lane loads its realisation's five constants of bin k (table [nb][5][T]: contiguous across the
//                   lanes) and adds that bin's term of every seed of the tile -- read from LDS at one address by all lanes, a broadcast
//                   -- into one accumulator per seed, in registers.  Each seed's sum still ascends in k.  After the last bin the lane
//                   offers lp_j + (acc_j + offset), j ascending.  The seed range is split over blockIdx.y, the scales over blockIdx.z.
//   k_toyb_merge    as k_toy_merge (gf_toys.hip): the parts' lists merged under the same total order, the selected cube points gathered
//   k_toyb_score    every score, for the tests
// No floating-point atomics and nothing order-dependent; no result depends on the tile, the part, the grid or on the other scales and
// realisations of a call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "gf_cube_runs.hpp"
#include "gf_pool.h"
#include "gf_toys_binned.hpp"
#include "gf_toys_prior.hpp"

namespace {
using namespace gftoyb;

constexpr int TOYB_LANES = 64;           // realisations per workgroup of k_toyb_select: one wave
constexpr int TOYB_TILE = 32;            // seeds staged in LDS at a time, one accumulator each in every lane's registers
// doubles between a tile's bins in LDS: TOYB_TILE compositions and three of padding, so that the staging writes of consecutive bins
// (lanes three apart) start 6 banks apart and a wave's ds_write_b64 takes the four passes its 128 dwords need at the least
constexpr int TOYB_KSTRIDE = 3 * TOYB_TILE + 3;
static_assert(MAX_STARTS == GF_TOY_MAX_STARTS, "gf_toys.hpp states the public limit");
static_assert(gftoy::STATUS_NON_UNITARY == GF_ST_NON_UNITARY && gftoy::STATUS_NON_UNITARY == ST_NON_UNITARY, "gf_toys.hpp states the public status");
static_assert(NCONST == GF_BINNED_STRIDE, "gf_toys_binned.hpp states the binned table's stride");
static_assert(CHUNK % TOYB_TILE == 0, "a part of the seed range is whole tiles");
// the tile of k_toyb_select: 16 096 bytes at 20 bins, 50 944 at GF_MAX_BINS.  Sized by the call's bins, not by the limit, so that a CU
// holds more than three workgroups at the usual binnings
constexpr size_t toyb_lds_bytes(int nb) { return sizeof(double) * (size_t)(TOYB_TILE + nb * TOYB_KSTRIDE); }
static_assert(toyb_lds_bytes(GF_MAX_BINS) <= 64 * 1024, "the tile at GF_MAX_BINS fits 64 KiB of LDS");

struct DevLogOfExp {
    __device__ __forceinline__ double operator()(double x) const { return gfdev::log_of_exp(x); }
};

struct ToybSelArgs {
    const double* lp;                   // [S][M]
    const double* frb;                  // [S][M][nb][3]
    const int32_t* st;                  // [S][M]
    const double* tab;                  // [S][nb][5][T], or [nb][5][T] shared by the scales (tab_stride = 0)
    int64_t tab_stride;
    double offset;
    int32_t M, T, nb, nparts, K;
    double* part_s;                     // [S][T][nparts][KM]
    int32_t* part_i;
    const double* seed_u;               // [S][M][N], NULL: no cube points
    int32_t N;
    int32_t* out_index;                 // [S][T][K], -1 behind the count
    double* out_score;                  // [S][T][K], -inf behind the count
    int32_t* out_count;                 // [S][T]
    double* out_cube;                   // [S][T][K][N], NaN behind the count (NULL without seed_u)
    double* all_scores;                 // k_toyb_score: [S][T][M]
};

// blockIdx = (block of TOYB_LANES realisations, part of the seed range, scale)
template <int KM>
__global__ __launch_bounds__(TOYB_LANES) void k_toyb_select(const ToybSelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double toyb_lds[];     // toyb_lds_bytes(nb): the kernel's only LDS
    double* tile_lp = toyb_lds;                                            // [TOYB_TILE]
    double* tile_fr = toyb_lds + TOYB_TILE;                                // [nb][TOYB_TILE][3], padded per bin
    const int s = blockIdx.z, part = blockIdx.y;
    const int t = blockIdx.x * TOYB_LANES + threadIdx.x;
    const bool live = t < a.T;
    const int nb = a.nb, per = 3 * nb;
    const int64_t T = a.T;
    const double* tab = a.tab + (int64_t)s * a.tab_stride + (live ? t : 0);
    Best<KM> best;
    best.clear();
    const int i0 = part * CHUNK;
    const int i1 = i0 + CHUNK < a.M ? i0 + CHUNK : a.M;
    const double* lp = a.lp + (int64_t)s * a.M;
    const double* frb = a.frb + (int64_t)s * a.M * per;
    const int32_t* st = a.st + (int64_t)s * a.M;
    for (int base = i0; base < i1; base += TOYB_TILE) {
        const int nt = i1 - base < TOYB_TILE ? i1 - base : TOYB_TILE;
        __syncthreads();                                               // the previous tile has been read
        // a seed's 3 nb doubles are contiguous in memory; the rows behind the part's last seed are (-inf, 0): never offered
        if (threadIdx.x < TOYB_TILE) tile_lp[threadIdx.x] = (int)threadIdx.x < nt ? seed_lp(lp[base + threadIdx.x], st[base + threadIdx.x]) : neg_inf();
        for (int j = 0; j < TOYB_TILE; ++j) {
            const double* src = frb + (int64_t)(base + j) * per;
            for (int e = threadIdx.x; e < per; e += TOYB_LANES) {
                const int k = e / 3, d = e - 3 * k;
                tile_fr[k * TOYB_KSTRIDE + 3 * j + d] = j < nt ? src[e] : 0.0;
            }
        }
        __syncthreads();
        double acc[TOYB_TILE];
#pragma unroll
        for (int j = 0; j < TOYB_TILE; ++j) acc[j] = 0.0;
        for (int k = 0; k < nb; ++k) {
            const double m0 = tab[const_at(k, 0, T, 0)], m1 = tab[const_at(k, 1, T, 0)], m2 = tab[const_at(k, 2, T, 0)];
            const double mh = tab[const_at(k, 3, T, 0)], kk = tab[const_at(k, 4, T, 0)];
            const double* f = tile_fr + k * TOYB_KSTRIDE;
#pragma unroll
            for (int j = 0; j < TOYB_TILE; ++j)                        // uniform: every lane reads the same seed
                acc[j] = add_term(acc[j], bin_term(f[3 * j], f[3 * j + 1], f[3 * j + 2], m0, m1, m2, mh, kk, DevLogOfExp()));
        }
#pragma unroll
        for (int j = 0; j < TOYB_TILE; ++j) best.offer(finish(tile_lp[j], acc[j], a.offset), base + j);
    }
    if (!live) return;
    const int64_t at = (((int64_t)s * a.T + t) * a.nparts + part) * KM;
#pragma unroll
    for (int j = 0; j < KM; ++j) { a.part_s[at + j] = best.s[j]; a.part_i[at + j] = best.i[j]; }
}

// a lane per (scale, realisation): the parts' lists merged, the first K entries out
template <int KM>
__global__ __launch_bounds__(GF_BLOCK) void k_toyb_merge(const ToybSelArgs a, int64_t npairs)
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
__global__ __launch_bounds__(GF_BLOCK) void k_toyb_score(const ToybSelArgs a)
{
    const int s = blockIdx.z, t = blockIdx.y;
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    if (i >= a.M) return;
    const int64_t at = (int64_t)s * a.M + i;
    a.all_scores[((int64_t)s * a.T + t) * a.M + i] = score(seed_lp(a.lp[at], a.st[at]), a.frb + at * 3 * a.nb, a.nb, a.tab + (int64_t)s * a.tab_stride,
                                                           (int64_t)a.T, (int64_t)t, a.offset, DevLogOfExp());
}

template <int KM>
hipError_t launch_select_km(const ToybSelArgs& a, int S, hipStream_t st)
{
    const dim3 grid((unsigned)((a.T + TOYB_LANES - 1) / TOYB_LANES), (unsigned)a.nparts, (unsigned)S);
    hipLaunchKernelGGL(k_toyb_select<KM>, grid, dim3(TOYB_LANES), toyb_lds_bytes(a.nb), st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t npairs = (int64_t)S * a.T;
    hipLaunchKernelGGL(k_toyb_merge<KM>, dim3((unsigned)((npairs + GF_BLOCK - 1) / GF_BLOCK)), dim3(GF_BLOCK), 0, st, a, npairs);
    return hipGetLastError();
}

inline int toy_km(int K) { return K <= 1 ? 1 : K <= 4 ? 4 : MAX_STARTS; }

// The selection of S scales' seeds under T realisations on `st`: the device inputs of `a` (lp, frb, st, tab, seed_u) are the caller's,
// the parts' lists and the outputs are scratch of this call, copied to the host arrays (NULL = skip) before it returns.
int toyb_select_run(ToybSelArgs a, int S, hipStream_t st, int32_t* index, double* score, int32_t* count, double* cube, const char* who)
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

// The realisations' constants on the host: `sets` tables [nb][5][T] from meas [sets][T][nb][3] and sigma ([T][nb], or [nb] shared by the
// realisations), the constants by gf_internal_gauss_consts as gf_model_set_binned_measurement derives them
int toyb_table(const double* meas, const double* sigma, int per_toy_sigma, size_t sets, size_t T, size_t nb, std::vector<double>& out, const char* who)
{
    out.resize(sets * nb * NCONST * T);
    for (size_t q = 0; q < sets; ++q)
        for (size_t t = 0; t < T; ++t)
            for (size_t k = 0; k < nb; ++k) {
                const double* m = meas + ((q * T + t) * nb + k) * 3;
                const double sg = sigma[(per_toy_sigma ? t * nb : 0) + k];
                if (!(sg > 0.0) || !std::isfinite(sg) || !std::isfinite(m[0]) || !std::isfinite(m[1]) || !std::isfinite(m[2]))
                    return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: bin %zu of realisation %zu needs a finite composition and a width > 0", who, k, t);
                double inv_smear, c0, mh, kk;
                gf_internal_gauss_consts(sg, &inv_smear, &c0, &mh, &kk);
                if (!std::isfinite(mh) || !std::isfinite(kk))
                    return gf_fail_msg(GF_ERR_INVALID_ARG, "%s: the width of bin %zu of realisation %zu is outside the range of the Gaussian's constants", who, k, t);
                double* o = out.data() + q * nb * NCONST * T;
                for (int d = 0; d < 3; ++d) o[const_at((int)k, d, (int64_t)T, (int64_t)t)] = m[d];
                o[const_at((int)k, 3, (int64_t)T, (int64_t)t)] = mh;
                o[const_at((int)k, 4, (int64_t)T, (int64_t)t)] = kk;
            }
    return GF_OK;
}

}  // namespace

struct gf_toys_binned {
    GfCubeRunsHost rs;
    GfCubeRuns a = {};
    int nseed = 0, nbins = 0, seeded = 0;
    double offset = 0.0;                // the scale models' likelihood offset: one for all
    double* d_u = nullptr;              // [S][M][N]
    double* d_theta = nullptr;          // [S][M][ndim]
    double* d_lnl = nullptr;            // [S][M] the scale models' own lnprob (under the models' binned measurement)
    double* d_fr = nullptr;             // [S][M][3] the flux-averaged compositions
    double* d_frb = nullptr;            // [S][M][nb][3]
    int32_t* d_st = nullptr;            // [S][M]
    double* d_lp = nullptr;             // [S][M]
    unsigned int* d_nonunit = nullptr;  // [S]
};

namespace {
// the measurements of a gf_toys_binned call on the device; the table is released by the caller's scratch
int toysb_upload(gf_toys_binned* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, GfScratch& scratch,
                 ToybSelArgs& a, const char* who)
{
    const size_t S = t->a.nruns, sets = per_scale ? S : 1, nb = t->nbins;
    std::vector<double> tab;
    const int rc = toyb_table(meas, sigma, per_toy_sigma, sets, (size_t)ntoys, nb, tab, who);
    if (rc != GF_OK) return rc;
    double* d = nullptr;
    if (scratch.take(&d, sizeof(double) * tab.size(), who) != GF_OK) return scratch.failed;
    GF_HIP(hipMemcpyAsync(d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, t->rs.stream));
    GF_HIP(hipStreamSynchronize(t->rs.stream));                          // tab goes out of scope
    a = ToybSelArgs{};
    a.lp = t->d_lp; a.frb = t->d_frb; a.st = t->d_st; a.tab = d; a.tab_stride = per_scale ? (int64_t)nb * NCONST * ntoys : 0;
    a.offset = t->offset; a.M = t->nseed; a.T = ntoys; a.nb = t->nbins; a.seed_u = t->d_u; a.N = t->a.nscan;
    return GF_OK;
}
}  // namespace

extern "C" {

int gf_toys_create_binned(gf_model* const* models, int nscales, int nscan, const int32_t* cols, const double* bases, int nseed, uint64_t seed,
                          gf_toys_binned** out)
{
    if (!models || !cols || !bases || !out || nscales < 1 || nscales > 65535 || nscan < 1 || nscan > GF_MAX_DIM || nseed < 1 ||
        nseed > (1 << 22))
        return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_toys_binned* t = new (std::nothrow) gf_toys_binned();
    if (!t) return GF_ERR_ALLOC;
    int rc = cube_runs_create(t->rs, t->a, models, nscales, nscan, cols, bases, seed, "gf_toys_create_binned");
    if (rc != GF_OK) { delete t; return rc; }
    if (t->rs.table)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_create_binned: the models carry a tabulated likelihood; a realisation of a table is not defined");
    else if (!t->rs.binned)
        rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_create_binned: the models carry no binned measurement; gf_toys_create seeds the flux-averaged Gaussian likelihood");
    t->nseed = nseed;
    for (int r = 0; r < nscales && rc == GF_OK; ++r) {
        const GfCommon* c; const GfBsm* tb; const double* pt; int device, cus, nb;
        rc = gf_model_constants(models[r], &c, &tb, &pt, &device, &cus, &nb);
        if (rc != GF_OK) break;
        if (r == 0) { t->nbins = nb; t->offset = c->offset; }
        // realisations shared by the scales are scored once per scale with one table and one offset
        if (nb != t->nbins || nb < 1 || nb > GF_MAX_BINS)
            rc = gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_create_binned: model %d has %d energy bins, model 0 has %d", r, nb, t->nbins);
        else if (!(c->offset == t->offset))
            rc = gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_create_binned: model %d has another likelihood offset than model 0", r);
    }
    if (rc != GF_OK) { gf_toys_destroy_binned(t); return rc; }
    const size_t S = nscales, M = nseed;
    hipError_t e = hipSuccess;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    al((void**)&t->d_u, sizeof(double) * S * M * nscan);
    al((void**)&t->d_theta, sizeof(double) * S * M * t->a.ndim);
    al((void**)&t->d_lnl, sizeof(double) * S * M);
    al((void**)&t->d_fr, sizeof(double) * S * M * 3);
    al((void**)&t->d_frb, sizeof(double) * S * M * 3 * t->nbins);
    al((void**)&t->d_st, sizeof(int32_t) * S * M);
    al((void**)&t->d_lp, sizeof(double) * S * M);
    al((void**)&t->d_nonunit, sizeof(unsigned int) * S);
    if (e != hipSuccess) { rc = gf_hip_fail(e, "gf_toys_create_binned"); gf_toys_destroy_binned(t); return rc; }
    *out = t;
    return GF_OK;
}

void gf_toys_destroy_binned(gf_toys_binned* t)
{
    if (!t) return;
    cube_runs_free(t->rs, t->a);
    void* ptrs[] = {t->d_u, t->d_theta, t->d_lnl, t->d_fr, t->d_frb, t->d_st, t->d_lp, t->d_nonunit};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete t;
}

int gf_toys_set_run_ids_binned(gf_toys_binned* t, const uint64_t* ids)
{
    if (!t || !ids) return GF_ERR_INVALID_ARG;
    return cube_runs_set_ids(t->rs, t->a, ids, "gf_toys_set_run_ids_binned: before gf_toys_seed_binned");
}

int gf_toys_seed_binned(gf_toys_binned* t, uint32_t* nonunitary)
{
    if (!t) return GF_ERR_INVALID_ARG;
    if (t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_seed_binned: the seeds have been drawn");
    GF_HIP(hipSetDevice(t->rs.device));
    const GfCubeRuns& a = t->a;
    const int n = t->nseed;
    hipStream_t st = t->rs.stream;
    const dim3 grid((unsigned)((n + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(k_cube_draw, grid, dim3(GF_BLOCK), 0, st, a, SX_SEED_ITER, n, t->d_u, t->d_theta);
    GF_HIP(hipGetLastError());
    for (int r = 0; r < a.nruns; ++r) {
        const size_t at = (size_t)r * n;
        int rc = gf_model_lnprob_on(t->rs.models[r], st, t->d_theta + at * a.ndim, GF_LAYOUT_AOS, n, t->d_lnl + at, t->d_fr + at * 3, t->d_st + at);
        if (rc == GF_OK)
            rc = gf_model_bins_on(t->rs.models[r], st, t->d_theta + at * a.ndim, GF_LAYOUT_AOS, n, t->d_frb + at * 3 * t->nbins, 0, t->d_st + at);
        if (rc != GF_OK) return rc;
    }
    GF_HIP(hipMemsetAsync(t->d_nonunit, 0, sizeof(unsigned int) * a.nruns, st));
    hipLaunchKernelGGL(k_toy_prior<true>, grid, dim3(GF_BLOCK), 0, st, a, n, t->d_theta, t->d_st, t->d_lp, t->d_nonunit);
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

int gf_toys_get_seeds_binned(gf_toys_binned* t, int scale, double* cube, double* lnprob, double* lp, double* fr, double* fr_bins, int32_t* status)
{
    if (!t || scale < 0 || scale >= t->a.nruns) return GF_ERR_INVALID_ARG;
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_get_seeds_binned: after gf_toys_seed_binned");
    GF_HIP(hipSetDevice(t->rs.device));
    const size_t M = t->nseed, at = (size_t)scale * M, per = 3 * (size_t)t->nbins;
    hipStream_t st = t->rs.stream;
    if (cube) GF_HIP(hipMemcpyAsync(cube, t->d_u + at * t->a.nscan, sizeof(double) * M * t->a.nscan, hipMemcpyDeviceToHost, st));
    if (lnprob) GF_HIP(hipMemcpyAsync(lnprob, t->d_lnl + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (lp) GF_HIP(hipMemcpyAsync(lp, t->d_lp + at, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (fr) GF_HIP(hipMemcpyAsync(fr, t->d_fr + at * 3, sizeof(double) * M * 3, hipMemcpyDeviceToHost, st));
    if (fr_bins) GF_HIP(hipMemcpyAsync(fr_bins, t->d_frb + at * per, sizeof(double) * M * per, hipMemcpyDeviceToHost, st));
    if (status) GF_HIP(hipMemcpyAsync(status, t->d_st + at, sizeof(int32_t) * M, hipMemcpyDeviceToHost, st));
    GF_HIP(hipStreamSynchronize(st));
    return GF_OK;
}

int gf_toys_select_binned(gf_toys_binned* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, int K,
                          double* cube, int32_t* index, double* score, int32_t* count)
{
    if (!t || !meas || !sigma || ntoys < 1 || ntoys > (1 << 20) || (per_scale != 0 && per_scale != 1) || (per_toy_sigma != 0 && per_toy_sigma != 1))
        return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select_binned: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select_binned: after gf_toys_seed_binned");
    GF_HIP(hipSetDevice(t->rs.device));
    GfScratch scratch;
    ToybSelArgs a;
    const int rc = toysb_upload(t, meas, per_scale, sigma, per_toy_sigma, ntoys, scratch, a, "gf_toys_select_binned");
    if (rc != GF_OK) return rc;
    a.K = K;
    return toyb_select_run(a, t->a.nruns, t->rs.stream, index, score, count, cube, "gf_toys_select_binned");
}

int gf_toys_scores_binned(gf_toys_binned* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, double* scores)
{
    if (!t || !meas || !sigma || !scores || ntoys < 1 || ntoys > 65535 || (per_scale != 0 && per_scale != 1) ||
        (per_toy_sigma != 0 && per_toy_sigma != 1))
        return GF_ERR_INVALID_ARG;
    if (!t->seeded) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_scores_binned: after gf_toys_seed_binned");
    GF_HIP(hipSetDevice(t->rs.device));
    GfScratch scratch;
    ToybSelArgs a;
    const int rc = toysb_upload(t, meas, per_scale, sigma, per_toy_sigma, ntoys, scratch, a, "gf_toys_scores_binned");
    if (rc != GF_OK) return rc;
    const size_t n = (size_t)t->a.nruns * ntoys * t->nseed;
    if (scratch.take(&a.all_scores, sizeof(double) * n, "gf_toys_scores_binned") != GF_OK) return scratch.failed;
    const dim3 grid((unsigned)((a.M + GF_BLOCK - 1) / GF_BLOCK), (unsigned)ntoys, (unsigned)t->a.nruns);
    hipLaunchKernelGGL(k_toyb_score, grid, dim3(GF_BLOCK), 0, t->rs.stream, a);
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(scores, a.all_scores, sizeof(double) * n, hipMemcpyDeviceToHost, t->rs.stream));
    GF_HIP(hipStreamSynchronize(t->rs.stream));
    return GF_OK;
}

int gf_toy_select_binned(int device, const double* lp, const double* fr_bins, const int32_t* status, int nseed, int nbins, const double* meas,
                         const double* sigma, int per_toy_sigma, double offset, int ntoys, int K, int32_t* out_index, double* out_score,
                         int32_t* out_count)
{
    if (!lp || !fr_bins || !status || !meas || !sigma || nseed < 1 || nseed > (1 << 22) || nbins < 1 || nbins > GF_MAX_BINS || ntoys < 1 ||
        ntoys > (1 << 20) || (per_toy_sigma != 0 && per_toy_sigma != 1))
        return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toy_select_binned: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    std::vector<double> tab;
    int rc = toyb_table(meas, sigma, per_toy_sigma, 1, (size_t)ntoys, (size_t)nbins, tab, "gf_toy_select_binned");
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
        const size_t M = nseed, per = 3 * (size_t)nbins;
        double *d_lp = nullptr, *d_frb = nullptr, *d_tab = nullptr;
        int32_t* d_st = nullptr;
        scratch.take(&d_lp, sizeof(double) * M, "gf_toy_select_binned");
        scratch.take(&d_frb, sizeof(double) * M * per, "gf_toy_select_binned");
        scratch.take(&d_st, sizeof(int32_t) * M, "gf_toy_select_binned");
        scratch.take(&d_tab, sizeof(double) * tab.size(), "gf_toy_select_binned");
        rc = scratch.failed;
        hipError_t e = hipSuccess;
        auto up = [&](void* dst, const void* src, size_t bytes) { if (rc == GF_OK && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
        up(d_lp, lp, sizeof(double) * M);
        up(d_frb, fr_bins, sizeof(double) * M * per);
        up(d_st, status, sizeof(int32_t) * M);
        up(d_tab, tab.data(), sizeof(double) * tab.size());
        if (rc == GF_OK && e != hipSuccess) rc = gf_hip_fail(e, "gf_toy_select_binned");
        if (rc == GF_OK) {
            ToybSelArgs a = {};
            a.lp = d_lp; a.frb = d_frb; a.st = d_st; a.tab = d_tab; a.tab_stride = 0; a.offset = offset; a.M = nseed; a.T = ntoys; a.nb = nbins; a.K = K;
            rc = toyb_select_run(a, 1, st, out_index, out_score, out_count, nullptr, "gf_toy_select_binned");
        }
        (void)hipStreamSynchronize(st);                                   // idle before the scratch and the stream go back
    }
    gf_internal_return_stream(device, stv);
    return rc;
}

}  // extern "C"
