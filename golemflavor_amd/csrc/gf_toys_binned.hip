// gf_toys_binned.hip -- the realisation ensembles of the energy-resolved likelihood: many mock measurements of
// one binned measurement profiled at every new-physics scale, with the scales' seed points drawn and propagated once.  The seed set
// (with its compositions at every energy bin), the merge of a selection and the stand-alone wrapper are the shared layer's
// (gf_toys_common.hpp, gf_toys_common.hip); this file plugs the binned score into it.
//
// A seed point's prior sum, its unitarity verdict and its composition at every energy bin do not depend on the measurement; only the
// per-bin Gaussian terms do.  Per (scale, realisation):
//   k_toyb_select   a lane owns a realisation and keeps its best seeds in registers.  A realisation has 5 nb constants and a seed
//                   1 + 3 nb doubles, so neither sits in registers whole: the workgroup stages a tile of TOYB_TILE seeds in LDS, the bin
//                   loop runs outermost, a lane loads its realisation's five constants of bin k (table [nb][5][T]: contiguous across the
//                   lanes) and adds that bin's term of every seed of the tile -- read from LDS at one address by all lanes, a broadcast
//                   -- into one accumulator per seed, in registers.  Each seed's sum still ascends in k.  After the last bin the lane
//                   offers lp_j + (acc_j + offset), j ascending.  The seed range is split over blockIdx.y, the scales over blockIdx.z.
//   k_toyb_score    every score, for the tests
// Nothing order-dependent; no result depends on the tile, the part, the grid or on the other scales and realisations of a call.
#include <cmath>
#include <vector>

#include "gf_toys_binned.hpp"
#include "gf_toys_common.hpp"

namespace {
using namespace gftoyb;

constexpr int TOYB_LANES = 64;           // realisations per workgroup of k_toyb_select: one wave
constexpr int TOYB_TILE = 32;            // seeds staged in LDS at a time, one accumulator each in every lane's registers
// doubles between a tile's bins in LDS: TOYB_TILE compositions and three of padding, so that the staging writes of consecutive bins
// (lanes three apart) start 6 banks apart and a wave's ds_write_b64 takes the four passes its 128 dwords need at the least
constexpr int TOYB_KSTRIDE = 3 * TOYB_TILE + 3;
static_assert(NCONST == GF_BINNED_STRIDE, "gf_toys_binned.hpp states the binned table's stride");
static_assert(CHUNK % TOYB_TILE == 0, "a part of the seed range is whole tiles");
// the tile of k_toyb_select: 16 096 bytes at 20 bins, 50 944 at GF_MAX_BINS.  Sized by the call's bins, not by the limit, so that a CU
// holds more than three workgroups at the usual binnings
constexpr size_t toyb_lds_bytes(int nb) { return sizeof(double) * (size_t)(TOYB_TILE + nb * TOYB_KSTRIDE); }
static_assert(toyb_lds_bytes(GF_MAX_BINS) <= 64 * 1024, "the tile at GF_MAX_BINS fits 64 KiB of LDS");

struct ToybSelArgs : ToyTail {
    const double* lp;                   // [S][M]
    const double* frb;                  // [S][M][nb][3]
    const int32_t* st;                  // [S][M]
    const double* tab;                  // [S][nb][5][T], or [nb][5][T] shared by the scales (tab_stride = 0)
    int64_t tab_stride;
    double offset;
    int32_t nb;
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

void launch_select(const ToyTail& tail, int KM, int S, hipStream_t st)
{
    const ToybSelArgs& a = static_cast<const ToybSelArgs&>(tail);
    const dim3 grid((unsigned)((a.T + TOYB_LANES - 1) / TOYB_LANES), (unsigned)a.nparts, (unsigned)S);
    if (KM == 1) hipLaunchKernelGGL(k_toyb_select<1>, grid, dim3(TOYB_LANES), toyb_lds_bytes(a.nb), st, a);
    else if (KM == 4) hipLaunchKernelGGL(k_toyb_select<4>, grid, dim3(TOYB_LANES), toyb_lds_bytes(a.nb), st, a);
    else hipLaunchKernelGGL(k_toyb_select<MAX_STARTS>, grid, dim3(TOYB_LANES), toyb_lds_bytes(a.nb), st, a);
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

// the measurements of a gf_toys_binned call on the device; the table is released by the caller's scratch
int toysb_upload(ToySeedSet* t, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, GfScratch& scratch,
                 ToybSelArgs& a, const char* who)
{
    const size_t S = t->a.nruns, sets = per_scale ? S : 1, nb = t->nbins;
    std::vector<double> tab;
    const int rc = toyb_table(meas, sigma, per_toy_sigma, sets, (size_t)ntoys, nb, tab, who);
    if (rc != GF_OK) return rc;
    double* d = nullptr;
    if (scratch.take(&d, sizeof(double) * tab.size(), who) != GF_OK) return scratch.failed;
    GF_HIP(hipMemcpyAsync(d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, t->rs.set.stream));
    GF_HIP(hipStreamSynchronize(t->rs.set.stream));                          // tab goes out of scope
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
    return toy_seeds_create((void**)out, models, nscales, nscan, cols, bases, nseed, seed, true, "gf_toys_create_binned", "gf_toys_seed_binned");
}

void gf_toys_destroy_binned(gf_toys_binned* h) { toy_seeds_destroy(toy_set(h)); }

int gf_toys_set_run_ids_binned(gf_toys_binned* h, const uint64_t* ids)
{
    return toy_seeds_set_ids(toy_set(h), ids, "gf_toys_set_run_ids_binned: before gf_toys_seed_binned");
}

int gf_toys_seed_binned(gf_toys_binned* h, uint32_t* nonunitary) { return toy_seeds_seed(toy_set(h), nonunitary, "gf_toys_seed_binned"); }

int gf_toys_get_seeds_binned(gf_toys_binned* h, int scale, double* cube, double* lnprob, double* lp, double* fr, double* fr_bins, int32_t* status)
{
    return toy_seeds_get(toy_set(h), scale, cube, lnprob, lp, fr, fr_bins, status, "gf_toys_get_seeds_binned");
}

int gf_toys_select_binned(gf_toys_binned* h, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, int K,
                          double* cube, int32_t* index, double* score, int32_t* count)
{
    ToySeedSet* t = toy_set(h);
    if (!t || !meas || !sigma || ntoys < 1 || ntoys > (1 << 20) || (per_scale != 0 && per_scale != 1) || (per_toy_sigma != 0 && per_toy_sigma != 1))
        return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select_binned: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    int rc = toy_seeds_ready(*t, "gf_toys_select_binned");
    if (rc != GF_OK) return rc;
    GfScratch scratch(GF_MEM_DRIVER);
    ToybSelArgs a;
    rc = toysb_upload(t, meas, per_scale, sigma, per_toy_sigma, ntoys, scratch, a, "gf_toys_select_binned");
    if (rc != GF_OK) return rc;
    a.K = K;
    return toy_select_run(a, t->a.nruns, t->rs.set.stream, launch_select, index, score, count, cube, "gf_toys_select_binned");
}

int gf_toys_scores_binned(gf_toys_binned* h, const double* meas, int per_scale, const double* sigma, int per_toy_sigma, int ntoys, double* scores)
{
    ToySeedSet* t = toy_set(h);
    if (!t || !meas || !sigma || !scores || ntoys < 1 || ntoys > 65535 || (per_scale != 0 && per_scale != 1) ||
        (per_toy_sigma != 0 && per_toy_sigma != 1))
        return GF_ERR_INVALID_ARG;
    int rc = toy_seeds_ready(*t, "gf_toys_scores_binned");
    if (rc != GF_OK) return rc;
    GfScratch scratch(GF_MEM_DRIVER);
    ToybSelArgs a;
    rc = toysb_upload(t, meas, per_scale, sigma, per_toy_sigma, ntoys, scratch, a, "gf_toys_scores_binned");
    if (rc != GF_OK) return rc;
    const size_t n = (size_t)t->a.nruns * ntoys * t->nseed;
    if (scratch.take(&a.all_scores, sizeof(double) * n, "gf_toys_scores_binned") != GF_OK) return scratch.failed;
    const dim3 grid((unsigned)((a.M + GF_BLOCK - 1) / GF_BLOCK), (unsigned)ntoys, (unsigned)t->a.nruns);
    hipLaunchKernelGGL(k_toyb_score, grid, dim3(GF_BLOCK), 0, t->rs.set.stream, a);
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(scores, a.all_scores, sizeof(double) * n, hipMemcpyDeviceToHost, t->rs.set.stream));
    GF_HIP(hipStreamSynchronize(t->rs.set.stream));
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
    const int rc = toyb_table(meas, sigma, per_toy_sigma, 1, (size_t)ntoys, (size_t)nbins, tab, "gf_toy_select_binned");
    if (rc != GF_OK) return rc;
    ToybSelArgs a = {};
    a.tab_stride = 0; a.offset = offset; a.M = nseed; a.T = ntoys; a.nb = nbins; a.K = K;
    const size_t M = nseed;
    const ToyUpload up[] = {{lp, sizeof(double) * M, (const void**)&a.lp}, {fr_bins, sizeof(double) * M * 3 * nbins, (const void**)&a.frb},
                            {status, sizeof(int32_t) * M, (const void**)&a.st}, {tab.data(), sizeof(double) * tab.size(), (const void**)&a.tab}};
    return toy_select_alone(device, a, launch_select, up, 4, out_index, out_score, out_count, "gf_toy_select_binned");
}

}  // extern "C"
