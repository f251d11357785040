// gf_elements.hip -- rows of sampled columns [n][width_in] turned into the element-space rows [n][width_out] the reference plots for
// --plot-elements (golemflavor/plot.py:528-567): moduli |U_ij| and source composition in place of the angle projections, the
// arithmetic of gf_elements.hpp.  A pure stream, 8 width_in bytes read and 8 width_out written per row, laid out as DESIGN.md
// section 3 lays out theta: a wave owns 64 consecutive rows = one contiguous span, loads it with 16-byte lane-contiguous loads into
// a wave-private LDS tile [64][width_in], every lane evaluates its own row (plan fields are kernel-argument scalar loads at uniform
// indices, the row's columns LDS reads at uniform column indices) into a second wave-private tile [64][width_out], and the wave
// stores that tile's span the way it loaded the other.  No workgroup barrier: both tiles are wave-private.
//
// The fp64 moduli cannot settle the float32 table where an entry is below ~1e-7 (gf_elements_exact.hpp), so k_element_rows also
// writes one 64-bit mask per tile -- the rows with a modulus below GFEL_SMALL -- and k_element_rows_exact, launched behind it, gives
// those rows' moduli again through the emulated 80-bit chain (plans with round32 only: round32 off keeps the fp64 values).  It reads nrows / 8 bytes of masks and touches only marked rows: a
// sampled posterior has next to none (|U_e3| ~ 0.15 is the smallest modulus of the PMNS matrix), the edges of the box do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_elements.h"
#include "gf_elements_exact.hpp"

namespace {

constexpr int EL_BLOCK = 256;
constexpr int EL_WAVE = 64;
constexpr int EL_WAVES = EL_BLOCK / EL_WAVE;
// Grid cap in blocks per compute unit.  Not tuned, nothing here is timed yet: the C5 shape (12 -> 17 columns) takes 59 KB of LDS per
// block, so about two are resident and the rest of the grid queues; a mask buffer is taken from the cache and given back on every
// call; the exact kernel visits every tile's mask even when no row is marked (nrows / 8 bytes).  When timings are taken, a
// device-side any-marked flag and a padded LDS row stride (even widths conflict on the lanes' row reads) are the things to try.
constexpr int EL_BLOCKS_PER_CU = 8;

// doubles of a wave's tile of `w` columns, a whole number of 16-byte vectors
__host__ __device__ inline int el_tile(int w) { return (EL_WAVE * w + 1) & ~1; }

// same-wave LDS write -> read (or read -> rewrite): in order in hardware; keeps the compiler from reordering across it
__device__ __forceinline__ void el_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// `count` doubles from src to dst, lane-contiguous; VEC: both 16-byte aligned, 16 bytes per lane and instruction
template <bool VEC>
__device__ __forceinline__ void el_copy(const double* __restrict__ src, double* __restrict__ dst, int count, int lane)
{
    if (VEC) {
        for (int d = 2 * lane; d < count; d += 2 * EL_WAVE) {
            if (d + 1 < count) *reinterpret_cast<double2*>(dst + d) = *reinterpret_cast<const double2*>(src + d);
            else dst[d] = src[d];
        }
    } else {
        for (int d = lane; d < count; d += EL_WAVE) dst[d] = src[d];
    }
}

// grid (tile groups, 1, chains), blocks of EL_BLOCK threads, or of half as many where four waves' tiles exceed 64 KiB;
// dynamic LDS: (el_tile(win) + el_tile(wout)) doubles per wave
// mask: [chains][tiles], bit l of a tile's word = its row l goes to k_element_rows_exact
template <bool VEC>
__global__ __launch_bounds__(EL_BLOCK) void k_element_rows(const gf_element_plan plan, const double* __restrict__ in, int64_t in_stride,
                                                           double* __restrict__ out, int64_t out_stride, int64_t nrows, int win, int wout,
                                                           unsigned long long* __restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) double el_lds[];
    const int lane = threadIdx.x & (EL_WAVE - 1), wave = threadIdx.x / EL_WAVE;
    double* tin = el_lds + wave * (el_tile(win) + el_tile(wout));
    double* tout = tin + el_tile(win);
    in += (int64_t)blockIdx.z * in_stride;
    out += (int64_t)blockIdx.z * out_stride;
    const int64_t ntiles = (nrows + EL_WAVE - 1) / EL_WAVE;
    const int waves = blockDim.x / EL_WAVE;
    mask += (int64_t)blockIdx.z * ntiles;
    for (int64_t t = (int64_t)blockIdx.x * waves + wave; t < ntiles; t += (int64_t)gridDim.x * waves) {
        const int64_t r0 = t * EL_WAVE;
        const int rows = nrows - r0 < EL_WAVE ? (int)(nrows - r0) : EL_WAVE;
        el_copy<VEC>(in + r0 * win, tin, rows * win, lane);
        el_wave_sync();
        bool small = false;
        if (lane < rows) small = gfel::element_row_fast(plan, tin + lane * win, tout + lane * wout);
        const unsigned long long mk = __ballot(small);
        if (lane == 0) mask[t] = mk;
        el_wave_sync();
        el_copy<VEC>(tout, out + r0 * wout, rows * wout, lane);
        el_wave_sync();                                               // the tiles are rewritten by the same wave next iteration
    }
}

// grid (tile groups, 1, chains), blocks of EL_BLOCK threads: the marked rows of every tile, straight from and to memory
__global__ __launch_bounds__(EL_BLOCK) void k_element_rows_exact(const gf_element_plan plan, const double* __restrict__ in, int64_t in_stride,
                                                                 double* __restrict__ out, int64_t out_stride, int64_t nrows, int win, int wout,
                                                                 const unsigned long long* __restrict__ mask)
{
    const int lane = threadIdx.x & (EL_WAVE - 1), wave = threadIdx.x / EL_WAVE;
    const int64_t ntiles = (nrows + EL_WAVE - 1) / EL_WAVE;
    in += (int64_t)blockIdx.z * in_stride;
    out += (int64_t)blockIdx.z * out_stride;
    mask += (int64_t)blockIdx.z * ntiles;
    for (int64_t t = (int64_t)blockIdx.x * EL_WAVES + wave; t < ntiles; t += (int64_t)gridDim.x * EL_WAVES) {
        const unsigned long long mk = mask[t];
        const int64_t r = t * EL_WAVE + lane;
        if (((mk >> lane) & 1ull) && r < nrows) gfel::element_row_exact(plan, in + r * win, out + r * wout);
    }
}

inline bool el_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

hipError_t gf_element_run(hipStream_t st, const double* d_in, int64_t in_stride, int nchains, int64_t nrows, int width_in,
                          const gf_element_plan* plan, double* d_out, int64_t out_stride, int cus)
{
    if (nrows <= 0 || nchains <= 0) return hipStreamSynchronize(st);
    const int wout = gfel::plan_width(plan, width_in);
    const int64_t ntiles = (nrows + EL_WAVE - 1) / EL_WAVE;
    const size_t lds_wave = sizeof(double) * (size_t)(el_tile(width_in) + el_tile(wout));           // <= 17920
    const int waves = lds_wave * EL_WAVES <= 65536 ? EL_WAVES : EL_WAVES / 2;
    int64_t blocks = (ntiles + waves - 1) / waves;
    const int64_t cap = ((int64_t)cus * EL_BLOCKS_PER_CU + nchains - 1) / nchains;
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks, 1u, (unsigned)nchains), block((unsigned)(waves * EL_WAVE));
    const size_t lds = lds_wave * waves;
    GfScratch buf(GF_MEM_CACHED);
    unsigned long long* d_mask = nullptr;
    hipError_t e = buf.get(&d_mask, sizeof(unsigned long long) * (size_t)ntiles * nchains);
    if (e != hipSuccess) return e;
    // a tile's span starts a multiple of 512 width bytes behind its chain's first row
    const bool vec = el_aligned16(d_in) && el_aligned16(d_out) && (nchains == 1 || (in_stride % 2 == 0 && out_stride % 2 == 0));
    if (vec)
        hipLaunchKernelGGL(k_element_rows<true>, grid, block, lds, st, *plan, d_in, in_stride, d_out, out_stride, nrows, width_in, wout, d_mask);
    else
        hipLaunchKernelGGL(k_element_rows<false>, grid, block, lds, st, *plan, d_in, in_stride, d_out, out_stride, nrows, width_in, wout, d_mask);
    e = hipGetLastError();
    if (e == hipSuccess && plan->round32) {
        int64_t xb = (ntiles + EL_WAVES - 1) / EL_WAVES;
        if (xb > cap) xb = cap;
        hipLaunchKernelGGL(k_element_rows_exact, dim3((unsigned)xb, 1u, (unsigned)nchains), dim3(EL_BLOCK), 0, st, *plan, d_in, in_stride, d_out,
                           out_stride, nrows, width_in, wout, d_mask);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    return e == hipSuccess ? e2 : e;
}

extern "C" {

int gf_element_plan_width(const gf_element_plan* plan, int width_in) { return gfel::plan_width(plan, width_in); }

int gf_element_rows_device(gf_model* m, const double* d_in, int64_t nrows, int width_in, const gf_element_plan* plan, double* d_out)
{
    if (nrows < 0 || gfel::plan_width(plan, width_in) < 0 || (nrows > 0 && (!d_in || !d_out))) return GF_ERR_INVALID_ARG;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7u) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; int device, cus, nbins;
    int rc = gf_model_constants(m, &c, &tb, &ptab, &device, &cus, &nbins);
    void* stream;
    if (rc == GF_OK) rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);    // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = gf_element_run(st, d_in, 0, 1, nrows, width_in, plan, d_out, 0, cus);
    return e == hipSuccess ? GF_OK : gf_hip_fail(e, "gf_element_rows_device");
}

int gf_element_rows(gf_model* m, const double* rows, int64_t nrows, int width_in, const gf_element_plan* plan, double* out)
{
    const int wout = gfel::plan_width(plan, width_in);
    if (nrows < 0 || wout < 0 || (nrows > 0 && (!rows || !out))) return GF_ERR_INVALID_ARG;
    if (nrows == 0) return GF_OK;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nin = sizeof(double) * (size_t)nrows * width_in, nout = sizeof(double) * (size_t)nrows * wout;
    GfScratch buf(GF_MEM_CACHED);
    double *d_in = nullptr, *d_out = nullptr;
    hipError_t e = buf.get(&d_in, nin);
    if (e == hipSuccess) e = buf.get(&d_out, nout);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, rows, nin, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) rc = gf_element_rows_device(m, d_in, nrows, width_in, plan, d_out);
    if (e == hipSuccess && rc == GF_OK) e = hipMemcpyAsync(out, d_out, nout, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && rc == GF_OK) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_element_rows");
    return rc;
}

}  // extern "C"
