// gf_spectrum.hip -- the composition at EACH energy bin.  flux_averaged_BSMu (golemflavor/fr.py:441-457) evaluates
// u_to_fr(source, params_to_BSMu(..., energy = E_k)) for every bin and keeps only the width-weighted mean; flux_average
// (gf_bsm_device.hpp) does the same with (f_e, f_mu) of bin k in registers.  k_bsm_bins is that value loop with the accumulation
// replaced by a store: same per-walker prologue, same bin_moduli<UNI_NONE>, same propagation, bit for bit the terms of the average.
// The verdict is not this kernel's: a status array written by the existing propagate path says which rows the reference would have
// raised on (fr.py:398-399: at the first failing bin, so such a sample has no composition at ANY energy), and those rows get NaN.
//
// Host side: the launch, gf_propagate_bins[_device], and the reduction of a bin-major slab [nbins][n][3] with the energy bins as
// gf_marginal_run's "chains" (gf_sampler_spectrum in gf_postprocess.hip, gf_nested_spectrum in gf_nested_post.hip call it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_marginal.h"
#include "gf_spectrum.h"

namespace {
using namespace gfdev;

// One lane per row, one wave per tile of 64 rows (staged through LDS as k_bsm stages them), grid-stride over the tiles.  Nothing is
// carried across the bin loop but the invariants k_bsm<UNI_NONE> carries, so the register budget is that kernel's: three waves per
// SIMD at a compile-time row width, two at the generic one.
// Stores, inside the bin loop (no per-bin array):
//   bin-major  out[(k n + i) 3 + .]: the wave's 64 rows of bin k are one contiguous 1536-byte run;
//   row-major  out[(i nbins + k) 3 + .]: a lane's bins follow one another, 24 nbins bytes from the next lane's; the tile's
//              64 x 24 nbins bytes are contiguous and written by this wave alone within one pass of the loop, so the lines fill in L2
//              before they leave for HBM.
template <int NDIM>
__global__ __launch_bounds__(GF_BLOCK, NDIM == 0 ? 2 : 3) void k_bsm_bins(const GfCommon* __restrict__ cp, const GfBsm* __restrict__ tb,
                                                                           const double* __restrict__ ptab, const double* __restrict__ theta,
                                                                           int layout, int64_t n, double* __restrict__ out, int bin_major,
                                                                           const int32_t* __restrict__ status)
{
    const GfCommon& c = *cp;                                             // by pointer: see k_bsm
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * (NDIM ? NDIM : GF_MAX_DIM)];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, ptab, tb, true);
    __syncthreads();
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GF_WAVE);
    const int ndim = NDIM ? NDIM : c.ndim;
    const int nb = tb->nbins;
    double* tile = tiles[wave];
    const int64_t ntiles = (n + GF_WAVE - 1) / GF_WAVE;
    const int64_t stride = (int64_t)gridDim.x * GF_WAVES_PER_BLOCK;
    // element stride between a row's consecutive bins, and between consecutive rows of one bin
    const int64_t kstep = bin_major ? 3 * n : 3;
    const int64_t istep = bin_major ? 3 : 3 * (int64_t)nb;
    for (int64_t t = (int64_t)blockIdx.x * GF_WAVES_PER_BLOCK + wave; t < ntiles; t += stride) {
        const int64_t w0 = t * GF_WAVE;
        stage_theta<NDIM>(theta, layout, n, w0, ndim, tile, lane);
        const int64_t i = w0 + lane;
        if (i < n) {
            const double* row = tile + lane * ndim;
            const bool bad = status != nullptr && status[i] != ST_OK;
            Herm3 S, N;
            hamiltonian_terms(c, tb, ttab, row, S, N);
            Herm3 Sn, Nn;
            BinInv w;
            bin_invariants(S, N, Sn, Nn, w);
            // the source enters as src / sum(src), exactly as in flux_average
            const double isrc = fast_rcp(c.src_fixed_sum);
            const double s2 = c.src_fixed[2] * isrc;
            const double ds0 = fma(c.src_fixed[0], isrc, -s2), ds1 = fma(c.src_fixed[1], isrc, -s2);
            UniAcc acc = {0.0, 0.0, 0ull, 2.0};                           // untouched by UNI_NONE
            double* o = out + i * istep;
            for (int k = 0; k < nb; ++k) {
                double p[3][3];
                bin_moduli<UNI_NONE>(w, Sn, Nn, tb->rho[k], p, acc, k, tb);
                const double p02 = (1.0 - p[0][0]) - p[0][1], p12 = (1.0 - p[1][0]) - p[1][1];
                const double w0s = fma(ds1, p[1][0], fma(ds0, p[0][0], s2));
                const double w1s = fma(ds1, p[1][1], fma(ds0, p[0][1], s2));
                const double w2s = fma(ds1, p12, fma(ds0, p02, s2));
                const double dw0 = w0s - w2s, dw1 = w1s - w2s;
                double f0 = fma(p[0][1], dw1, fma(p[0][0], dw0, w2s));
                double f1 = fma(p[1][1], dw1, fma(p[1][0], dw0, w2s));
                double f2 = (1.0 - f0) - f1;                               // sum(src / sum src) = 1
                if (bad) f0 = f1 = f2 = gf_nan();
                o[0] = f0; o[1] = f1; o[2] = f2;
                o += kstep;
            }
        }
        // the next tile overwrites this wave's LDS rows
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int NDIM>
hipError_t launch_bins(const GfCommon* d_common, const GfBsm* d_bsm, const double* ptab, const double* theta, int layout, int64_t n, double* out,
                       int bin_major, const int32_t* status, int cus, hipStream_t s)
{
    int64_t blocks = (n + GF_BLOCK - 1) / GF_BLOCK;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 256) * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_bsm_bins<NDIM>, dim3((unsigned)blocks), dim3(GF_BLOCK), 0, s, d_common, d_bsm, ptab, theta, layout, n, out, bin_major, status);
    return hipGetLastError();
}

}  // namespace

hipError_t gf_launch_bsm_bins(const GfCommon& c, const GfCommon* d_common, const GfBsm* d_bsm, int nbins, const double* ptab, const double* theta,
                              int layout, int64_t n, double* out, int bin_major, const int32_t* status, int cus, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (nbins < 1 || nbins > GF_MAX_BINS || !d_common || !d_bsm || !theta || !out) return hipErrorInvalidValue;
    switch (c.ndim) {
    case 7: return launch_bins<7>(d_common, d_bsm, ptab, theta, layout, n, out, bin_major, status, cus, s);
    case 12: return launch_bins<12>(d_common, d_bsm, ptab, theta, layout, n, out, bin_major, status, cus, s);
    default: return launch_bins<0>(d_common, d_bsm, ptab, theta, layout, n, out, bin_major, status, cus, s);
    }
}

int gf_spectrum_check_args(int nbins_e, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out)
{
    if (!spec || !out || nbins_e < 1 || nbins_e > GF_MAX_BINS || nrows < 1) return GF_ERR_INVALID_ARG;
    if (spec->nbins1 < 1 || spec->nbins1 > 1024 || spec->nq < 0 || (spec->nq > 0 && !spec->q)) return GF_ERR_INVALID_ARG;
    for (int i = 0; i < spec->nq; ++i)
        if (!(spec->q[i] >= 0.0 && spec->q[i] <= 100.0)) return GF_ERR_INVALID_ARG;
    if (2 * spec->nq > GF_MARGINAL_MAX_RANKS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "spectrum: 2 x %d percentiles exceed GF_MARGINAL_MAX_RANKS = %d", spec->nq, GF_MARGINAL_MAX_RANKS);
    return GF_OK;
}

int gf_spectrum_reduce(hipStream_t st, const double* d_slab, int nbins_e, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out,
                       int ch)
{
    const int nb1 = spec->nbins1, R = 2 * spec->nq;
    // np.linspace(0, 1, nb1 + 1) as numpy forms it: arange * (1 / nb1), the last edge set to the stop; the same for all three flavours.
    // The 2-D products of the marginal routine are not part of the result: null outputs, one bin
    std::vector<double> e1((size_t)3 * (nb1 + 1));
    const double step = 1.0 / (double)nb1;
    for (int c = 0; c < 3; ++c) {
        for (int b = 0; b < nb1; ++b) e1[(size_t)c * (nb1 + 1) + b] = (double)b * step;
        e1[(size_t)c * (nb1 + 1) + nb1] = 1.0;
    }
    const double e2[6] = {0.0, 1.0, 0.0, 1.0, 0.0, 1.0};
    const double coverage[1] = {50.0};                                      // the argument check wants one; no region is computed
    gf_marginal_spec ms;
    std::memset(&ms, 0, sizeof(ms));
    ms.nbins1 = nb1; ms.nbins2 = 1; ms.edges1 = e1.data(); ms.edges2 = e2;
    ms.radius = 0; ms.ncov = 1; ms.weights = nullptr; ms.coverage = coverage;
    ms.nranks = 0; ms.nq = spec->nq; ms.ranks = nullptr; ms.q = spec->q;
    ms.cap1 = 0; ms.cap2 = 0;
    gf_marginal_out mo;
    std::memset(&mo, 0, sizeof(mo));
    const size_t at = (size_t)ch * nbins_e;
    if (out->nvalid) mo.nvalid = out->nvalid + at;
    if (out->mean) mo.mean = out->mean + at * 3;
    if (out->cov) mo.cov = out->cov + at * 9;
    if (out->ostat && R) mo.ostat = out->ostat + at * 3 * R;
    if (out->orank && R) mo.orank = out->orank + at * 3 * R;
    if (out->counts) mo.counts1 = out->counts + at * 3 * nb1;
    return gf_marginal_run(st, d_slab, nrows * 3, nbins_e, nrows, 3, &ms, &mo);
}

extern "C" {

int gf_propagate_bins_device(gf_model* m, const double* d_theta, int layout, int64_t n, double* d_fr_bins, int bin_major, const int32_t* d_status)
{
    if (!m || n < 0 || (layout != GF_LAYOUT_AOS && layout != GF_LAYOUT_SOA)) return GF_ERR_INVALID_ARG;
    if (gf_model_nbins(m) < 1) return GF_ERR_UNSUPPORTED;
    if (n == 0) return GF_OK;
    if (!d_theta || !d_fr_bins || ((uintptr_t)d_theta % 16) || ((uintptr_t)d_fr_bins % 8) || ((uintptr_t)d_status % 4)) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    const int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);      // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    return gf_model_bins_on(m, stream, d_theta, layout, n, d_fr_bins, bin_major, d_status);
}

int gf_propagate_bins(gf_model* m, const double* theta, int64_t n, double* fr_bins, int32_t* status)
{
    if (!m || n < 0 || (n > 0 && (!theta || !fr_bins))) return GF_ERR_INVALID_ARG;
    const int nbins = gf_model_nbins(m);
    if (nbins < 1) return GF_ERR_UNSUPPORTED;
    if (n == 0) return GF_OK;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = sizeof(double) * 3 * (size_t)nbins * (size_t)n;
    GfScratch buf(GF_MEM_CACHED);
    double *d_theta = nullptr, *d_out = nullptr; int32_t* d_st = nullptr;
    hipError_t e = buf.get(&d_theta, sizeof(double) * (size_t)c->ndim * n);
    if (e == hipSuccess) e = buf.get(&d_out, out_bytes);
    if (e == hipSuccess && status) e = buf.get(&d_st, sizeof(int32_t) * (size_t)n);
    if (e == hipSuccess) e = hipMemcpyAsync(d_theta, theta, sizeof(double) * (size_t)c->ndim * n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return gf_hip_fail(e, "gf_propagate_bins"); }
    // the verdict is the existing path's, unchanged; its compositions land in the head of the output buffer and are overwritten
    if (status) rc = gf_model_propagate_on(m, stream, d_theta, GF_LAYOUT_AOS, n, d_out, d_st);
    if (rc == GF_OK) rc = gf_model_bins_on(m, stream, d_theta, GF_LAYOUT_AOS, n, d_out, 0, d_st);
    if (rc == GF_OK && status) e = hipMemcpyAsync(status, d_st, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st);
    if (rc == GF_OK && e == hipSuccess) rc = gf_internal_d2h(device, stream, fr_bins, d_out, out_bytes);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, "gf_propagate_bins");
    return status ? gf_internal_check_overflow(device, stream) : GF_OK;
}

}  // extern "C"
