// gf_toys.hip -- the realisation ensembles of the flux-averaged Gaussian likelihood: many mock measurements of
// one Gaussian measurement profiled at every new-physics scale, with the scales' seed points drawn and propagated once.  The seed
// set, the merge of a selection and the stand-alone wrapper are the shared layer's (gf_toys_common.hpp, gf_toys_common.hip); this file
// plugs the Gaussian score into it.
//
// A seed point's composition, prior sum and unitarity verdict do not depend on the measurement; only the Gaussian block of lnprob does
// (gf_reweight.hip uses the same fact for stored chains).  Per (scale, realisation):
//   k_toy_select    a lane owns a realisation (its constants in registers); the workgroup streams a part of the seed range through
//                   LDS, every lane reading the same seed (a broadcast), and each lane keeps the best of its part in registers
//                   (gf_toys.hpp: score, order, list); the seed range is split over blockIdx.y
//   k_toy_score     every score, for the tests
// Nothing order-dependent: no result depends on the tile, the part or the grid.
#include <vector>

#include "gf_toys_common.hpp"

namespace {
using namespace gftoy;

constexpr int TOY_LANES = 64;            // realisations per workgroup of k_toy_select: one wave
constexpr int TOY_TILE = 256;            // seeds staged in LDS at a time: {lp, fr[3]} each, 8 KiB
static_assert(CHUNK % TOY_TILE == 0, "a part of the seed range is whole tiles");

struct ToySelArgs : ToyTail {
    const double* lp;                   // [S][M]
    const double* fr;                   // [S][M][3]
    const int32_t* st;                  // [S][M]
    const Meas* meas;                   // [S][T], or [T] shared by the scales (meas_stride = 0)
    int64_t meas_stride;
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

void launch_select(const ToyTail& tail, int KM, int S, hipStream_t st)
{
    const ToySelArgs& a = static_cast<const ToySelArgs&>(tail);
    const dim3 grid((unsigned)((a.T + TOY_LANES - 1) / TOY_LANES), (unsigned)a.nparts, (unsigned)S);
    if (KM == 1) hipLaunchKernelGGL(k_toy_select<1>, grid, dim3(TOY_LANES), 0, st, a);
    else if (KM == 4) hipLaunchKernelGGL(k_toy_select<4>, grid, dim3(TOY_LANES), 0, st, a);
    else hipLaunchKernelGGL(k_toy_select<MAX_STARTS>, grid, dim3(TOY_LANES), 0, st, a);
}

// the realisations' constants on the host: [n] of Meas from bf [n][3], smearing[k % ntoys] and the seed set's offset
int toy_measurements(const double* bf, const double* smearing, size_t n, size_t ntoys, double offset, std::vector<Meas>& out, const char* who)
{
    out.resize(n);
    for (size_t k = 0; k < n; ++k) {
        const int rc = gf_gauss_realisation(bf + 3 * k, smearing[k % ntoys], k, who, out[k].m, &out[k].mh, &out[k].k);
        if (rc != GF_OK) return rc;
        out[k].offset = offset;
    }
    return GF_OK;
}

// the measurements of a gf_toys call on the device; `meas` is released by the caller's scratch
int toys_upload_meas(ToySeedSet* t, const double* bf, int per_scale, const double* smearing, int ntoys, GfScratch& scratch, ToySelArgs& a, const char* who)
{
    const size_t S = t->a.nruns, n = (per_scale ? S : 1) * (size_t)ntoys;
    std::vector<Meas> hm;
    // every realisation carries the one offset the scales' models share (checked at create)
    const int rc = toy_measurements(bf, smearing, n, (size_t)ntoys, t->offset, hm, who);
    if (rc != GF_OK) return rc;
    Meas* d = nullptr;
    if (scratch.take(&d, sizeof(Meas) * n, who) != GF_OK) return scratch.failed;
    GF_HIP(hipMemcpyAsync(d, hm.data(), sizeof(Meas) * n, hipMemcpyHostToDevice, t->rs.set.stream));
    GF_HIP(hipStreamSynchronize(t->rs.set.stream));                          // hm goes out of scope
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
    return toy_seeds_create((void**)out, models, nscales, nscan, cols, bases, nseed, seed, false, "gf_toys_create", "gf_toys_seed");
}

void gf_toys_destroy(gf_toys* h) { toy_seeds_destroy(toy_set(h)); }

int gf_toys_set_run_ids(gf_toys* h, const uint64_t* ids)
{
    return toy_seeds_set_ids(toy_set(h), ids, "gf_toys_set_run_ids: before gf_toys_seed");
}

int gf_toys_seed(gf_toys* h, uint32_t* nonunitary) { return toy_seeds_seed(toy_set(h), nonunitary, "gf_toys_seed"); }

int gf_toys_get_seeds(gf_toys* h, int scale, double* cube, double* lnprob, double* lp, double* fr, int32_t* status)
{
    return toy_seeds_get(toy_set(h), scale, cube, lnprob, lp, fr, nullptr, status, "gf_toys_get_seeds");
}

int gf_toys_select(gf_toys* h, const double* bf, int per_scale, const double* smearing, int ntoys, int K, double* cube, int32_t* index,
                   double* score, int32_t* count)
{
    ToySeedSet* t = toy_set(h);
    if (!t || !bf || !smearing || ntoys < 1 || ntoys > (1 << 20) || (per_scale != 0 && per_scale != 1)) return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_select: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    int rc = toy_seeds_ready(*t, "gf_toys_select");
    if (rc != GF_OK) return rc;
    GfScratch scratch(GF_MEM_DRIVER);
    ToySelArgs a;
    rc = toys_upload_meas(t, bf, per_scale, smearing, ntoys, scratch, a, "gf_toys_select");
    if (rc != GF_OK) return rc;
    a.K = K;
    return toy_select_run(a, t->a.nruns, t->rs.set.stream, launch_select, index, score, count, cube, "gf_toys_select");
}

int gf_toys_scores(gf_toys* h, const double* bf, int per_scale, const double* smearing, int ntoys, double* scores)
{
    ToySeedSet* t = toy_set(h);
    if (!t || !bf || !smearing || !scores || ntoys < 1 || ntoys > 65535 || (per_scale != 0 && per_scale != 1)) return GF_ERR_INVALID_ARG;
    int rc = toy_seeds_ready(*t, "gf_toys_scores");
    if (rc != GF_OK) return rc;
    GfScratch scratch(GF_MEM_DRIVER);
    ToySelArgs a;
    rc = toys_upload_meas(t, bf, per_scale, smearing, ntoys, scratch, a, "gf_toys_scores");
    if (rc != GF_OK) return rc;
    const size_t n = (size_t)t->a.nruns * ntoys * t->nseed;
    if (scratch.take(&a.all_scores, sizeof(double) * n, "gf_toys_scores") != GF_OK) return scratch.failed;
    const dim3 grid((unsigned)((a.M + GF_BLOCK - 1) / GF_BLOCK), (unsigned)ntoys, (unsigned)t->a.nruns);
    hipLaunchKernelGGL(k_toy_score, grid, dim3(GF_BLOCK), 0, t->rs.set.stream, a);
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(scores, a.all_scores, sizeof(double) * n, hipMemcpyDeviceToHost, t->rs.set.stream));
    GF_HIP(hipStreamSynchronize(t->rs.set.stream));
    return GF_OK;
}

int gf_toy_select(int device, const double* lp, const double* fr, const int32_t* status, int nseed, const double* bf, const double* smearing,
                  double offset, int ntoys, int K, int32_t* out_index, double* out_score, int32_t* out_count)
{
    if (!lp || !fr || !status || !bf || !smearing || nseed < 1 || nseed > (1 << 22) || ntoys < 1 || ntoys > (1 << 20))
        return GF_ERR_INVALID_ARG;
    if (K < 1 || K > MAX_STARTS) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toy_select: %d starts asked for, 1 to %d can be selected", K, MAX_STARTS);
    std::vector<Meas> hm;
    const int rc = toy_measurements(bf, smearing, (size_t)ntoys, (size_t)ntoys, offset, hm, "gf_toy_select");
    if (rc != GF_OK) return rc;
    ToySelArgs a = {};
    a.meas_stride = 0; a.M = nseed; a.T = ntoys; a.K = K;
    const size_t M = nseed;
    const ToyUpload up[] = {{lp, sizeof(double) * M, (const void**)&a.lp}, {fr, sizeof(double) * M * 3, (const void**)&a.fr},
                            {status, sizeof(int32_t) * M, (const void**)&a.st}, {hm.data(), sizeof(Meas) * ntoys, (const void**)&a.meas}};
    return toy_select_alone(device, a, launch_select, up, 4, out_index, out_score, out_count, "gf_toy_select");
}

}  // extern "C"
