// gf_diag.hip -- convergence diagnostics of stored chains [nsteps][nwalkers][ndim]: per chain and column the
// integrated autocorrelation time of the walker-averaged autocorrelation function and of the ensemble-mean series, each with Sokal's
// window, and split R-hat.  The arithmetic and the order of every sum are gf_diag.hpp's; nothing here uses an atomic, so the
// results do not depend on the grid, on how many chains are stacked or on which wave computes which lag.
//
// Per chain, on the caller's stream:
//   k_diag_transpose    [step][walker * dim] -> series-major [walker * dim][step] through a padded 32 x 32 LDS tile: 256-byte runs
//                       on the reading and on the writing side instead of one 128-byte line per double
//   k_walker_mean       (gf_sampler.hip) the ensemble-mean series [step][dim]
//   k_diag_acf          one workgroup per series: the series is loaded into LDS, summed, centred (the half sums of R-hat are taken
//                       here), and every thread computes whole lags: lane t reads y[i] as a broadcast and y[i + t] at consecutive
//                       addresses, conflict-free.  Writes A(t) / A(0) [series][lags] and the series' excluded flag.  Runs once on
//                       the transposed chain and once on the mean series (ndim series read at stride ndim: 8 n ndim bytes).
//   k_diag_walker_avg   one thread per (column, lag): the included walkers' values in gf_diag.hpp's blocked order
// and, once all chains are through, k_diag_final: one lane per (chain, column) does both running sums, windows and R-hat.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_devcache.h"                // the transposed chain and the per-walker functions are each about the size of one chain
#include "gf_host.h"
#include "gf_diag.h"
#include "gf_diag.hpp"

namespace {

constexpr int DG_TILE = 32;
constexpr int DG_TILE_ROWS = 8;
constexpr int DG_ACF_MAX_BLOCK = 1024;
constexpr int DG_BLOCK = 256;

// in [n][K] -> out [K][n]; grid (ceil(K / 32), ceil(n / 32)), block (32, 8)
__global__ __launch_bounds__(DG_TILE* DG_TILE_ROWS) void k_diag_transpose(const double* __restrict__ in, double* __restrict__ out, int64_t n,
                                                                          int64_t K)
{
    __shared__ double tile[DG_TILE][DG_TILE + 1];
    const int64_t k0 = (int64_t)blockIdx.x * DG_TILE, i0 = (int64_t)blockIdx.y * DG_TILE;
    for (int r = threadIdx.y; r < DG_TILE; r += DG_TILE_ROWS) {
        const int64_t i = i0 + r, k = k0 + threadIdx.x;
        if (i < n && k < K) tile[r][threadIdx.x] = in[i * K + k];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < DG_TILE; r += DG_TILE_ROWS) {
        const int64_t k = k0 + r, i = i0 + threadIdx.x;
        if (i < n && k < K) out[k * n + i] = tile[threadIdx.x][r];
    }
}

// the series sum of gf_diag.hpp by the whole workgroup: the first 256 threads take a partial each, then the halving tree in LDS.
// Every thread gets the sum.  `part`: 256 doubles of LDS.
template <int TERM>
__device__ __forceinline__ double dg_block_sum(const double* y, int lo, int hi, double c, double* part)
{
    const int tid = threadIdx.x;
    if (tid < gfdg::PARTS) part[tid] = gfdg::series_partial<TERM>(y, 1, lo, hi, tid, c);
    __syncthreads();
    for (int s = gfdg::PARTS / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] = gfdg::add(part[tid], part[tid + s]);
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();                                       // part is free again
    return r;
}

// One workgroup per series s: x_i = src[s * series_stride + i * elem_stride], i < n.  Dynamic LDS: (n + 256) doubles.
// racf [series][nlags], excl [series], halves [series][4] or NULL.  nan_excluded: an excluded series' racf is filled with NaN
// (else it is left as it is: the walker average skips it).
__global__ __launch_bounds__(DG_ACF_MAX_BLOCK) void k_diag_acf(const double* __restrict__ src, int64_t series_stride, int64_t elem_stride, int n,
                                                               int nlags, double* __restrict__ racf, int32_t* __restrict__ excl,
                                                               double* __restrict__ halves, int nan_excluded)
{
    extern __shared__ __attribute__((aligned(16))) double dg_lds[];
    double* y = dg_lds;
    double* part = dg_lds + n;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t s = blockIdx.x;
    src += s * series_stride;
    racf += s * (int64_t)nlags;
    int bad = 0;
    for (int i = tid; i < n; i += nt) {
        const double v = src[(int64_t)i * elem_stride];
        y[i] = v;
        bad |= !gfdg::finite(v);
    }
    const bool nonfinite = __syncthreads_or(bad) != 0;     // also: y is complete
    const double m = gfdg::div(dg_block_sum<gfdg::TERM_VALUE>(y, 0, n, 0.0, part), (double)n);
    for (int i = tid; i < n; i += nt) y[i] = gfdg::sub(y[i], m);
    __syncthreads();
    if (halves) {
        const int h = n / 2;
        for (int k = 0; k < 2; ++k) {
            const int lo = k ? n - h : 0;
            const double mu = gfdg::div(dg_block_sum<gfdg::TERM_VALUE>(y, lo, lo + h, 0.0, part), (double)h);
            const double q = dg_block_sum<gfdg::TERM_SQUARE>(y, lo, lo + h, mu, part);
            if (tid == 0) {
                halves[s * gfdg::HALF_FIELDS + 2 * k] = gfdg::add(m, mu);
                halves[s * gfdg::HALF_FIELDS + 2 * k + 1] = gfdg::div(q, (double)(h - 1));
            }
        }
    }
    // whole lags per thread; round k takes the lags [k nt, (k + 1) nt), odd rounds back to front so that a thread's long and
    // short lags even out.  The thread that owns lag 0 publishes A(0).
    for (int k = 0; k * nt < nlags; ++k) {
        const int t = k * nt + ((k & 1) ? nt - 1 - tid : tid);
        if (t < nlags) {
            const double a = gfdg::acov_lag(y, n, t);
            racf[t] = a;
            if (t == 0) part[0] = a;
        }
    }
    __syncthreads();
    const double a0 = part[0];
    const bool out = gfdg::excluded(nonfinite, a0);
    if (tid == 0) excl[s] = out ? 1 : 0;
    if (out && !nan_excluded) return;
    for (int k = 0; k * nt < nlags; ++k) {
        const int t = k * nt + ((k & 1) ? nt - 1 - tid : tid);
        if (t < nlags) racf[t] = out ? gfdg::nan() : gfdg::div(racf[t], a0);       // the thread's own earlier store
    }
}

// rho [ndim][nlags] = the walker average of racf [nwalkers][ndim][nlags]; grid (ceil(nlags / 256), ndim)
__global__ __launch_bounds__(DG_BLOCK) void k_diag_walker_avg(const double* __restrict__ racf, const int32_t* __restrict__ excl, int nwalkers,
                                                              int ndim, int nlags, double* __restrict__ rho)
{
    const int t = blockIdx.x * DG_BLOCK + threadIdx.x, d = blockIdx.y;
    if (t >= nlags) return;
    rho[(int64_t)d * nlags + t] = gfdg::walker_average(racf + (int64_t)d * nlags + t, (int64_t)ndim * nlags, excl + d, ndim, nwalkers, nullptr);
}

struct DgFinalArgs {
    const double *rho, *rho_mean;         // [nchains][ndim][nlags]
    const double* halves;                 // [nchains][nwalkers][ndim][4]
    const int32_t* excl;                  // [nchains][nwalkers][ndim]
    double *tau, *tau_mean, *rhat;        // [nchains][ndim]
    int64_t *window, *window_mean;
    int32_t* nexcluded;
    int nchains, nwalkers, ndim, n, nlags;
    double c;
};

// one lane per (chain, column)
__global__ __launch_bounds__(DG_BLOCK) void k_diag_final(const DgFinalArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * DG_BLOCK + threadIdx.x;
    if (e >= (int64_t)a.nchains * a.ndim) return;
    const int64_t ch = e / a.ndim;
    const int d = (int)(e % a.ndim);
    int64_t w = 0;
    a.tau[e] = gfdg::sokal_tau(a.rho + e * a.nlags, a.nlags, a.c, &w);
    a.window[e] = w;
    a.tau_mean[e] = gfdg::sokal_tau(a.rho_mean + e * a.nlags, a.nlags, a.c, &w);
    a.window_mean[e] = w;
    const int32_t* ex = a.excl + ch * a.nwalkers * a.ndim + d;
    int nex = 0;
    for (int k = 0; k < a.nwalkers; ++k) nex += ex[(int64_t)k * a.ndim] != 0;
    a.nexcluded[e] = nex;
    a.rhat[e] = gfdg::split_rhat(a.halves + (ch * a.nwalkers * a.ndim + d) * gfdg::HALF_FIELDS, (int64_t)a.ndim * gfdg::HALF_FIELDS, ex, a.ndim,
                                 a.nwalkers, a.n);
}

template <typename T>
hipError_t dg_fetch(T* host, const T* dev, size_t count, hipStream_t st)
{
    return host ? hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
}

}  // namespace

int gf_diag_check_args(int nchains, int64_t nsteps, int nwalkers, int ndim, const gf_diag_spec* spec, const gf_diag_out* out)
{
    if (!spec || !out || nchains < 1 || nsteps < 2 || nwalkers < 1 || ndim < 1 || ndim > GF_MAX_DIM) return GF_ERR_INVALID_ARG;
    if (!(spec->c > 0.0) || spec->maxlag >= nsteps) return GF_ERR_INVALID_ARG;
    if (nsteps > gfdg::MAX_STEPS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "chain diagnostics hold a series in LDS: %lld stored steps exceed %d, thin the chain",
                           (long long)nsteps, gfdg::MAX_STEPS);
    return GF_OK;
}

int gf_diag_run(hipStream_t st, const double* d_chain, int64_t chain_stride, int nchains, int64_t nsteps, int nwalkers, int ndim,
                const gf_diag_spec* spec, const gf_diag_out* out)
{
    const int n = (int)nsteps;
    const int nlags = (int)(spec->maxlag < 0 ? nsteps - 1 : spec->maxlag) + 1;
    const int64_t K = (int64_t)nwalkers * ndim;
    const size_t per = (size_t)nchains * ndim;
    GfScratch buf(GF_MEM_CACHED);
    double *d_t = nullptr, *d_racf = nullptr, *d_mean = nullptr, *d_halves = nullptr, *d_rho = nullptr, *d_rho_mean = nullptr;
    double *d_tau = nullptr, *d_tau_mean = nullptr, *d_rhat = nullptr;
    int64_t *d_window = nullptr, *d_window_mean = nullptr;
    int32_t *d_excl = nullptr, *d_excl_mean = nullptr, *d_nexcl = nullptr;
    hipError_t e = buf.get(&d_t, sizeof(double) * K * n);
    if (e == hipSuccess) e = buf.get(&d_racf, sizeof(double) * K * nlags);
    if (e == hipSuccess) e = buf.get(&d_mean, sizeof(double) * (size_t)n * ndim);
    if (e == hipSuccess) e = buf.get(&d_halves, sizeof(double) * gfdg::HALF_FIELDS * K * nchains);
    if (e == hipSuccess) e = buf.get(&d_excl, sizeof(int32_t) * K * nchains);
    if (e == hipSuccess) e = buf.get(&d_excl_mean, sizeof(int32_t) * per);
    if (e == hipSuccess) e = buf.get(&d_rho, sizeof(double) * per * nlags);
    if (e == hipSuccess) e = buf.get(&d_rho_mean, sizeof(double) * per * nlags);
    if (e == hipSuccess) e = buf.get(&d_tau, sizeof(double) * per);
    if (e == hipSuccess) e = buf.get(&d_tau_mean, sizeof(double) * per);
    if (e == hipSuccess) e = buf.get(&d_rhat, sizeof(double) * per);
    if (e == hipSuccess) e = buf.get(&d_window, sizeof(int64_t) * per);
    if (e == hipSuccess) e = buf.get(&d_window_mean, sizeof(int64_t) * per);
    if (e == hipSuccess) e = buf.get(&d_nexcl, sizeof(int32_t) * per);
    const size_t lds = sizeof(double) * ((size_t)n + gfdg::PARTS);
    const int acf_block = lds > 32768 ? DG_ACF_MAX_BLOCK : DG_BLOCK;
    if (e == hipSuccess && lds > 65536)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_diag_acf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 tgrid((unsigned)((K + DG_TILE - 1) / DG_TILE), (unsigned)((n + DG_TILE - 1) / DG_TILE));
    for (int ch = 0; ch < nchains && e == hipSuccess; ++ch) {
        const double* chain = d_chain + (int64_t)ch * chain_stride;
        hipLaunchKernelGGL(k_diag_transpose, tgrid, dim3(DG_TILE, DG_TILE_ROWS), 0, st, chain, d_t, (int64_t)n, K);
        e = hipGetLastError();
        if (e == hipSuccess) e = gf_launch_walker_mean(chain, n, n, 1, nwalkers, ndim, d_mean, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_diag_acf, dim3((unsigned)K), dim3(acf_block), lds, st, d_t, (int64_t)n, (int64_t)1, n, nlags, d_racf,
                               d_excl + (int64_t)ch * K, d_halves + (int64_t)ch * K * gfdg::HALF_FIELDS, 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_diag_acf, dim3((unsigned)ndim), dim3(acf_block), lds, st, d_mean, (int64_t)1, (int64_t)ndim, n, nlags,
                               d_rho_mean + (size_t)ch * ndim * nlags, d_excl_mean + (size_t)ch * ndim, (double*)nullptr, 1);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_diag_walker_avg, dim3((unsigned)((nlags + DG_BLOCK - 1) / DG_BLOCK), (unsigned)ndim), dim3(DG_BLOCK), 0, st, d_racf,
                               d_excl + (int64_t)ch * K, nwalkers, ndim, nlags, d_rho + (size_t)ch * ndim * nlags);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        const DgFinalArgs a = {d_rho, d_rho_mean, d_halves, d_excl, d_tau, d_tau_mean, d_rhat, d_window, d_window_mean, d_nexcl,
                               nchains, nwalkers, ndim, n, nlags, spec->c};
        hipLaunchKernelGGL(k_diag_final, dim3((unsigned)((per + DG_BLOCK - 1) / DG_BLOCK)), dim3(DG_BLOCK), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = dg_fetch(out->tau, d_tau, per, st);
    if (e == hipSuccess) e = dg_fetch(out->tau_mean, d_tau_mean, per, st);
    if (e == hipSuccess) e = dg_fetch(out->rhat, d_rhat, per, st);
    if (e == hipSuccess) e = dg_fetch(out->window, d_window, per, st);
    if (e == hipSuccess) e = dg_fetch(out->window_mean, d_window_mean, per, st);
    if (e == hipSuccess) e = dg_fetch(out->nexcluded, d_nexcl, per, st);
    if (e == hipSuccess) e = dg_fetch(out->rho, d_rho, per * nlags, st);
    if (e == hipSuccess) e = dg_fetch(out->rho_mean, d_rho_mean, per * nlags, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    return e == hipSuccess ? GF_OK : gf_hip_fail(e, "chain diagnostics");
}

extern "C" {

int gf_chain_diagnostics_device(gf_model* m, const double* d_chain, int64_t chain_stride, int nchains, int64_t nsteps, int nwalkers, int ndim,
                                const gf_diag_spec* spec, const gf_diag_out* out)
{
    int rc = gf_diag_check_args(nchains, nsteps, nwalkers, ndim, spec, out);
    if (rc != GF_OK) return rc;
    if (!d_chain || ((uintptr_t)d_chain & 7u) || (nchains > 1 && chain_stride < nsteps * nwalkers * ndim)) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);                      // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    GF_HIP(hipStreamSynchronize((hipStream_t)stream));
    return gf_diag_run((hipStream_t)stream, d_chain, chain_stride, nchains, nsteps, nwalkers, ndim, spec, out);
}

int gf_chain_diagnostics(gf_model* m, const double* chain, int64_t nsteps, int nwalkers, int ndim, const gf_diag_spec* spec,
                         const gf_diag_out* out)
{
    int rc = gf_diag_check_args(1, nsteps, nwalkers, ndim, spec, out);
    if (rc != GF_OK) return rc;
    if (!chain) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(double) * (size_t)nsteps * nwalkers * ndim;
    GfScratch buf(GF_MEM_CACHED);
    double* d_chain = nullptr;
    GF_HIP(buf.get(&d_chain, bytes));
    GF_HIP(hipMemcpyAsync(d_chain, chain, bytes, hipMemcpyHostToDevice, st));
    GF_HIP(hipStreamSynchronize(st));
    return gf_diag_run(st, d_chain, 0, 1, nsteps, nwalkers, ndim, spec, out);
}

}  // extern "C"
