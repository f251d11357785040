// gf_region.hip -- the credible regions of the flavor triangle, golemflavor/plot.py:371-392, on the device and for several
// chains in one set of launches: what flavor_contour does between np.histogramdd (k_flavor_hist, gf_kernels.hip) and the
// geometry.  Input: counts [nchains][nb][nb][nb] (uint64, axis 2 contiguous).  Per chain
//   normalise  H = count / total, one IEEE division per cell                                  (plot.py:371  H / np.sum(H))
//   smooth     three 1-D passes (axis 0, 1, 2) of scipy's correlate1d, mode 'reflect'         (plot.py:374  gaussian_filter)
//   select     the cells with H_s > 0 in descending order of H_s (equal values: descending flat index), their running sum taken
//              SEQUENTIALLY in fp64, and for every coverage c the number of leading cells whose sum is < c / 100
//                                                                    (plot.py:377-383  argsort, cumsum, searchsorted, mask)
// Every value that is compared with numpy / scipy is computed with __ddiv_rn / __dmul_rn / __dadd_rn: nothing is contracted.
//
// The sort is a bitonic network over (H_s, flat index) pairs: the pair is a total order, so the result does not depend on the
// order in which the compaction (one atomic per wave) happened to place the cells.  Tiles of RG_TILE pairs are sorted and
// merged in LDS; only the steps whose partner lies outside a tile go through global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_region.h"

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_TILE = 2048;            // pairs a workgroup sorts in LDS: 16 KiB of values + 8 KiB of indices
constexpr int RG_ROW_LDS = 2048;         // doubles of LDS the axis-2 pass stages rows in (16 KiB)
constexpr int RG_MAX_GRID = 1 << 20;

struct RgWeights {
    double w[2 * GF_REGION_MAX_RADIUS + 1];
};
struct RgCover {
    double cf[GF_REGION_MAX_COVERAGES];  // coverage / 100., ascending
    int32_t ncov;
};

// ---- normalise ---------------------------------------------------------------------------------------------------------------
// sums [nchains][2]: the counts' low and high 32-bit halves summed apart, so that no input can wrap the sum (each half is at
// most 2^30 cells x 2^32); the total is hi * 2^32 + lo
__global__ __launch_bounds__(RG_BLOCK) void k_region_total(const unsigned long long* __restrict__ counts, int64_t nb3,
                                                           unsigned long long* __restrict__ sums)
{
    const int ch = blockIdx.y;
    const unsigned long long* c = counts + (size_t)ch * nb3;
    unsigned long long lo = 0, hi = 0;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < nb3; i += (int64_t)gridDim.x * RG_BLOCK) {
        const unsigned long long v = c[i];
        lo += v & 0xffffffffull;
        hi += v >> 32;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo += __shfl_down(lo, off);
        hi += __shfl_down(hi, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo) atomicAdd(sums + 2 * ch, lo);
        if (hi) atomicAdd(sums + 2 * ch + 1, hi);
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_region_normalise(const unsigned long long* __restrict__ counts, int64_t nb3,
                                                               const unsigned long long* __restrict__ sums, double* __restrict__ H)
{
    const int ch = blockIdx.y;
    const unsigned long long total = sums[2 * ch] + (sums[2 * ch + 1] << 32);      // >= 2^53: the host refuses the call
    const double dt = (double)total;
    const unsigned long long* c = counts + (size_t)ch * nb3;
    double* h = H + (size_t)ch * nb3;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < nb3; i += (int64_t)gridDim.x * RG_BLOCK)
        h[i] = total ? __ddiv_rn((double)c[i], dt) : 0.0;
}

// ---- smooth ------------------------------------------------------------------------------------------------------------------
// scipy's 'reflect' (d c b a | a b c d | d c b a), continued periodically when the radius exceeds the axis
__device__ __forceinline__ int rg_reflect(int q, int n)
{
    if (q >= 0 && q < n) return q;
    const int p = 2 * n;
    int m = q % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// One pass along axis 0 (stride nb * nb) or axis 1 (stride nb).  One lane per cell in memory order, so a wave reads and writes
// runs of consecutive k: every tap of the loop over the filtered axis is a coalesced load at a constant offset of whole rows
// (planes), never a per-lane stride.  Summation order of scipy's symmetric correlate1d: centre, then the pairs from the
// outermost inwards.
__global__ __launch_bounds__(RG_BLOCK) void k_region_smooth_axis(const double* __restrict__ in, double* __restrict__ out, int nb,
                                                                 int64_t stride, int64_t ncells, int r, RgWeights W)
{
    for (int64_t g = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; g < ncells; g += (int64_t)gridDim.x * RG_BLOCK) {
        const int p = (int)((g / stride) % nb);
        double tmp = __dmul_rn(in[g], W.w[r]);
        for (int j = r; j >= 1; --j) {
            const int a = rg_reflect(p - j, nb), b = rg_reflect(p + j, nb);
            const double pair = __dadd_rn(in[g + (int64_t)(a - p) * stride], in[g + (int64_t)(b - p) * stride]);
            tmp = __dadd_rn(tmp, __dmul_rn(pair, W.w[r - j]));
        }
        out[g] = tmp;
    }
}

// The pass along the contiguous axis: a workgroup stages `rows` whole rows with their reflected halo of r in LDS.
__global__ __launch_bounds__(RG_BLOCK) void k_region_smooth_rows(const double* __restrict__ in, double* __restrict__ out, int nb,
                                                                 int64_t nrows, int rows, int r, RgWeights W)
{
    __shared__ double lds[RG_ROW_LDS];
    const int width = nb + 2 * r;
    for (int64_t row0 = (int64_t)blockIdx.x * rows; row0 < nrows; row0 += (int64_t)gridDim.x * rows) {
        const int nr = (int)(nrows - row0 < rows ? nrows - row0 : rows);
        for (int e = threadIdx.x; e < nr * width; e += RG_BLOCK) {
            const int rr = e / width, c = e - rr * width;
            lds[e] = in[(row0 + rr) * nb + rg_reflect(c - r, nb)];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nr * nb; e += RG_BLOCK) {
            const int rr = e / nb, k = e - rr * nb;
            const double* x = lds + rr * width + k + r;
            double tmp = __dmul_rn(x[0], W.w[r]);
            for (int j = r; j >= 1; --j) tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(x[-j], x[j]), W.w[r - j]));
            out[(row0 + rr) * nb + k] = tmp;
        }
        __syncthreads();
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_BLOCK) void k_region_count(const double* __restrict__ H, int64_t nb3, unsigned long long* __restrict__ nnz)
{
    const int ch = blockIdx.y;
    const double* h = H + (size_t)ch * nb3;
    unsigned long long n = 0;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < nb3; i += (int64_t)gridDim.x * RG_BLOCK) n += h[i] > 0.0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(nnz + ch, n);
}

// the cells with H_s > 0 of chain ch -> vals / idx [ch][0 .. nnz[ch]) in any order: one atomic per wave
__global__ __launch_bounds__(RG_BLOCK) void k_region_compact(const double* __restrict__ H, int64_t nb3, int64_t N,
                                                             unsigned long long* __restrict__ cursor, double* __restrict__ vals,
                                                             int32_t* __restrict__ idx)
{
    const int ch = blockIdx.y;
    const double* h = H + (size_t)ch * nb3;
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * RG_BLOCK; base < nb3; base += (int64_t)gridDim.x * RG_BLOCK) {
        const int64_t i = base + threadIdx.x;
        const double v = i < nb3 ? h[i] : 0.0;
        const bool keep = v > 0.0;
        const unsigned long long mask = __ballot(keep);
        if (mask == 0) continue;                                   // uniform in the wave
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long start = 0;
        if (lane == leader) start = atomicAdd(cursor + ch, (unsigned long long)__popcll(mask));
        start = __shfl(start, leader);
        if (keep) {
            const unsigned long long slot = start + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < (unsigned long long)N) {                    // N >= nnz[ch]: always true
                vals[(size_t)ch * N + slot] = v;
                idx[(size_t)ch * N + slot] = (int32_t)i;
            }
        }
    }
}

// the tail [nnz[ch], N) of every segment: pairs that sort behind every cell
__global__ __launch_bounds__(RG_BLOCK) void k_region_pad(const unsigned long long* __restrict__ nnz, int64_t N, double* __restrict__ vals,
                                                         int32_t* __restrict__ idx)
{
    const int ch = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * RG_BLOCK)
        if ((unsigned long long)i >= nnz[ch]) {
            vals[(size_t)ch * N + i] = -1.0;
            idx[(size_t)ch * N + i] = -1;
        }
}

// (va, ia) comes before (vb, ib): larger H_s first, equal values by descending flat index
__device__ __forceinline__ bool rg_before(double va, int32_t ia, double vb, int32_t ib) { return va > vb || (va == vb && ia > ib); }

// Steps of the network inside a tile, in LDS: for k = k_lo .. k_hi (doubling), j = min(k, RG_TILE) / 2 .. 1.
// (2, RG_TILE) sorts every tile; (k, k) with k > RG_TILE finishes the merge of stage k after its global steps.
__global__ __launch_bounds__(RG_BLOCK) void k_region_sort_tile(double* __restrict__ vals, int32_t* __restrict__ idx, int64_t N, int64_t k_lo,
                                                               int64_t k_hi)
{
    __shared__ double sv[RG_TILE];
    __shared__ int32_t si[RG_TILE];
    const size_t base = (size_t)blockIdx.x * RG_TILE;
    const int64_t pos0 = (int64_t)(base & (size_t)(N - 1));        // position of the tile in its chain's segment (N = 2^m >= RG_TILE)
    for (int e = threadIdx.x; e < RG_TILE; e += RG_BLOCK) { sv[e] = vals[base + e]; si[e] = idx[base + e]; }
    __syncthreads();
    for (int64_t k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)(k < RG_TILE ? k : RG_TILE) >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < RG_TILE / 2; t += RG_BLOCK) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const bool fwd = ((pos0 + a) & k) == 0;
                const double va = sv[a], vb = sv[b];
                const int32_t ia = si[a], ib = si[b];
                if (fwd ? rg_before(vb, ib, va, ia) : rg_before(va, ia, vb, ib)) { sv[a] = vb; sv[b] = va; si[a] = ib; si[b] = ia; }
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < RG_TILE; e += RG_BLOCK) { vals[base + e] = sv[e]; idx[base + e] = si[e]; }
}

// one step (k, j) with j >= RG_TILE: partners in different tiles, one lane per pair
__global__ __launch_bounds__(RG_BLOCK) void k_region_sort_step(double* __restrict__ vals, int32_t* __restrict__ idx, int64_t npairs, int64_t N,
                                                               int64_t k, int64_t j)
{
    for (int64_t t = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; t < npairs; t += (int64_t)gridDim.x * RG_BLOCK) {
        const int64_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
        const bool fwd = ((a & (N - 1)) & k) == 0;
        const double va = vals[a], vb = vals[b];
        const int32_t ia = idx[a], ib = idx[b];
        if (fwd ? rg_before(vb, ib, va, ia) : rg_before(va, ia, vb, ib)) { vals[a] = vb; vals[b] = va; idx[a] = ib; idx[b] = ia; }
    }
}

// The running sum, one lane per chain, in the order np.cumsum takes it; the workgroup only stages the sorted values in LDS.
// For coverage q (ascending): thres = leading cells whose inclusive sum is < cf[q] (np.searchsorted, side='left').  The walk
// ends as soon as the largest coverage is crossed.
__global__ __launch_bounds__(RG_BLOCK) void k_region_scan(const double* __restrict__ vals, const unsigned long long* __restrict__ nnz, int64_t N,
                                                          RgCover cov, long long* __restrict__ thres, int32_t* __restrict__ saturated,
                                                          double* __restrict__ level_in, double* __restrict__ level_out, double* __restrict__ mass)
{
    __shared__ double tile[RG_TILE];
    __shared__ double scf[GF_REGION_MAX_COVERAGES + 1];           // the coverages, closed by +inf
    __shared__ int done;
    const int ch = blockIdx.x;
    const int64_t n = (int64_t)nnz[ch];
    const double* v = vals + (size_t)ch * N;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double s = 0.0, prev = nan;
    int q = 0;
    if (threadIdx.x == 0) done = 0;
    if (threadIdx.x <= GF_REGION_MAX_COVERAGES)
        scf[threadIdx.x] = (int)threadIdx.x < cov.ncov ? cov.cf[threadIdx.x] : std::numeric_limits<double>::infinity();
    __syncthreads();
    for (int64_t base = 0; base < n; base += RG_TILE) {
        const int m = (int)(n - base < RG_TILE ? n - base : RG_TILE);
        for (int e = threadIdx.x; e < m; e += RG_BLOCK) tile[e] = v[base + e];
        __syncthreads();
        if (threadIdx.x == 0) {
            double target = scf[q];
#pragma unroll 8
            for (int t = 0; t < m; ++t) {
                const double x = tile[t];
                const double s2 = __dadd_rn(s, x);
                while (s2 >= target) {                             // the cell that crosses the coverage is outside
                    const int o = ch * cov.ncov + q;
                    thres[o] = base + t; saturated[o] = 0; level_in[o] = prev; level_out[o] = x; mass[o] = s;
                    ++q;
                    target = scf[q];
                }
                s = s2; prev = x;
                if (q >= cov.ncov) break;
            }
            if (q >= cov.ncov) done = 1;
        }
        __syncthreads();
        if (done) break;
    }
    if (threadIdx.x == 0)
        for (; q < cov.ncov; ++q) {                                // never reached: the reference's mask is the whole cube
            const int o = ch * cov.ncov + q;
            thres[o] = n; saturated[o] = n > 0; level_in[o] = prev; level_out[o] = nan; mass[o] = s;
        }
}

// One list per marginal (gf_marginal.hip): the first min(take[ch], cap) sorted pairs of segment ch -> cells / density [ch][cap]
__global__ __launch_bounds__(RG_BLOCK) void k_region_gather(const double* __restrict__ vals, const int32_t* __restrict__ idx, int64_t N,
                                                            const long long* __restrict__ take, int64_t cap, int32_t* __restrict__ cells,
                                                            double* __restrict__ density)
{
    const int ch = blockIdx.y;
    const int64_t n = take[ch] < cap ? take[ch] : cap;
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RG_BLOCK) {
        if (cells) cells[(size_t)ch * cap + i] = idx[(size_t)ch * N + i];
        if (density) density[(size_t)ch * cap + i] = vals[(size_t)ch * N + i];
    }
}

// the compositions of samples whose status is not OK become NaN (the rows a scan saves hold NaN there): k_flavor_hist drops them
__global__ __launch_bounds__(RG_BLOCK) void k_region_mask_fr(double* __restrict__ fr, const int32_t* __restrict__ status, int64_t n)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RG_BLOCK)
        if (status[i] != 0) { fr[3 * i] = nan; fr[3 * i + 1] = nan; fr[3 * i + 2] = nan; }
}

inline unsigned rg_grid(int64_t work_items)
{
    const int64_t b = (work_items + RG_BLOCK - 1) / RG_BLOCK;
    return (unsigned)(b < 1 ? 1 : b > RG_MAX_GRID ? RG_MAX_GRID : b);
}

}  // namespace

hipError_t gf_launch_mask_fr(double* fr, const int32_t* status, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_region_mask_fr, dim3(rg_grid(n)), dim3(RG_BLOCK), 0, s, fr, status, n);
    return hipGetLastError();
}

int gf_region_check_args(int nchains, int nbins, int radius, const double* weights, const double* coverage, int ncov, int64_t cap)
{
    if (nchains < 1 || nbins < 1 || nbins > 1024 || radius < 0 || !coverage || ncov < 1 || ncov > GF_REGION_MAX_COVERAGES || cap < 0)
        return GF_ERR_INVALID_ARG;
    for (int q = 0; q < ncov; ++q)
        if (!(coverage[q] > 0.0 && coverage[q] <= 100.0)) return GF_ERR_INVALID_ARG;       // NaN fails too
    if (radius > GF_REGION_MAX_RADIUS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "flavor region: smoothing radius %d exceeds GF_REGION_MAX_RADIUS = %d", radius,
                           GF_REGION_MAX_RADIUS);
    if (radius > 0 && !weights) return GF_ERR_INVALID_ARG;
    return GF_OK;
}

// Everything after the histogram, on stream `st` of the current device; synchronous.  d_counts [nchains][n0][n1][n2] (axis 2
// contiguous); an axis of length 1 is not filtered (a reflected halo of one cell would sum w * x, which is not x in fp64), so a
// batch of 1-D histograms is (1, 1, n) and a batch of 2-D ones (1, n, n).  Host outputs [nchains][ncov] (and [nchains][ncov][cap])
// may each be NULL; d_smoothed [nchains][n0][n1][n2] (device) may be NULL.  one_list: the regions of a chain are prefixes of one
// sorted list, so cells / density are [nchains][cap] and hold the first min(cap, largest thres) pairs, fetched in
// one copy instead of one per (chain, coverage).
int gf_region_run_shape(hipStream_t st, const uint64_t* d_counts, int nchains, int n0, int n1, int n2, int radius, const double* weights,
                        const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out,
                        double* mass, int32_t* cells, double* density, double* d_smoothed, int one_list)
{
    int rc = gf_region_check_args(nchains, n0, radius, weights, coverage, ncov, cap);
    if (rc == GF_OK) rc = gf_region_check_args(nchains, n1, radius, weights, coverage, ncov, cap);
    if (rc == GF_OK) rc = gf_region_check_args(nchains, n2, radius, weights, coverage, ncov, cap);
    if (rc != GF_OK) return rc;
    if (!d_counts || ((uintptr_t)d_counts % 8) || ((uintptr_t)d_smoothed % 8)) return GF_ERR_INVALID_ARG;
    const int64_t nb3 = (int64_t)n0 * n1 * n2;
    const int naxes = radius > 0 ? (n0 > 1) + (n1 > 1) + (n2 > 1) : 0;          // filter passes executed
    const int64_t ncells = nb3 * nchains;
    const int nres = nchains * ncov;

    // the coverages in ascending order; slot q of the device results belongs to coverage order[q]
    std::vector<int> order(ncov);
    for (int q = 0; q < ncov; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return coverage[a] < coverage[b]; });
    RgCover cov;
    std::memset(&cov, 0, sizeof(cov));
    cov.ncov = ncov;
    for (int q = 0; q < ncov; ++q) cov.cf[q] = coverage[order[q]] / 100.;
    RgWeights W;
    std::memset(&W, 0, sizeof(W));
    for (int t = 0; t < 2 * radius + 1 && radius > 0; ++t) W.w[t] = weights[t];

    // one small block: sums [nchains][2] | nnz [nchains] | cursor [nchains] | thres [nres] | level_in | level_out | mass [nres] | saturated [nres]
    const size_t n_u64 = (size_t)4 * nchains, small_bytes = 8 * (n_u64 + (size_t)4 * nres) + 4 * (size_t)nres;
    GfScratch buf(GF_MEM_CACHED);
    unsigned char* d_small = nullptr;
    double *d_x = nullptr, *d_y = nullptr, *d_vals = nullptr;
    int32_t* d_idx = nullptr;
    std::vector<unsigned char> h_small(small_bytes);
    hipError_t e = buf.get(&d_small, small_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_small, 0, small_bytes, st);
    if (e == hipSuccess && !d_smoothed) e = buf.get(&d_y, sizeof(double) * (size_t)ncells);
    if (e == hipSuccess && naxes > 0) e = buf.get(&d_x, sizeof(double) * (size_t)ncells);
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(d_small);
    unsigned long long* d_nnz = d_sums + 2 * (size_t)nchains;
    unsigned long long* d_cursor = d_nnz + nchains;
    long long* d_thres = reinterpret_cast<long long*>(d_cursor + nchains);
    double* d_lin = reinterpret_cast<double*>(d_thres + nres);
    double* d_lout = d_lin + nres;
    double* d_mass = d_lout + nres;
    int32_t* d_sat = reinterpret_cast<int32_t*>(d_mass + nres);
    double* H = d_smoothed ? d_smoothed : d_y;                   // where H_s ends up
    const dim3 per_chain(rg_grid(nb3) > 4096 ? 4096 : rg_grid(nb3), nchains);
    int64_t N = 0, maxnnz = 0;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_region_total, per_chain, dim3(RG_BLOCK), 0, st, (const unsigned long long*)d_counts, nb3, d_sums);
        // the passes alternate between x and H and the last one writes H: three passes are x -> H (axis 0), H -> x (axis 1),
        // x -> H (axis 2)
        double* src = (naxes & 1) ? d_x : H;
        hipLaunchKernelGGL(k_region_normalise, per_chain, dim3(RG_BLOCK), 0, st, (const unsigned long long*)d_counts, nb3, d_sums, src);
        if (naxes > 0 && n0 > 1) {
            double* dst = src == H ? d_x : H;
            hipLaunchKernelGGL(k_region_smooth_axis, dim3(rg_grid(ncells)), dim3(RG_BLOCK), 0, st, src, dst, n0, (int64_t)n1 * n2, ncells, radius, W);
            src = dst;
        }
        if (naxes > 0 && n1 > 1) {
            double* dst = src == H ? d_x : H;
            hipLaunchKernelGGL(k_region_smooth_axis, dim3(rg_grid(ncells)), dim3(RG_BLOCK), 0, st, src, dst, n1, (int64_t)n2, ncells, radius, W);
            src = dst;
        }
        if (naxes > 0 && n2 > 1) {
            double* dst = src == H ? d_x : H;
            const int rows = RG_ROW_LDS / (n2 + 2 * radius);     // >= 1: n2 + 2 r <= 1024 + 64
            const int64_t nrows = (int64_t)nchains * n0 * n1, blocks = (nrows + rows - 1) / rows;
            hipLaunchKernelGGL(k_region_smooth_rows, dim3((unsigned)(blocks > RG_MAX_GRID ? RG_MAX_GRID : blocks)), dim3(RG_BLOCK), 0, st, src,
                               dst, n2, nrows, rows, radius, W);
            src = dst;
        }
        hipLaunchKernelGGL(k_region_count, per_chain, dim3(RG_BLOCK), 0, st, H, nb3, d_nnz);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_small.data(), d_small, 8 * n_u64, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        const unsigned long long* hs = reinterpret_cast<const unsigned long long*>(h_small.data());
        for (int ch = 0; ch < nchains && rc == GF_OK; ++ch) {
            const unsigned __int128 total = ((unsigned __int128)hs[2 * ch + 1] << 32) + hs[2 * ch];
            if (total >= ((unsigned __int128)1 << 53))
                rc = gf_fail_msg(GF_ERR_UNSUPPORTED, "flavor region: chain %d holds 2^53 samples or more", ch);
            maxnnz = std::max<int64_t>(maxnnz, (int64_t)hs[2 * (size_t)nchains + ch]);
        }
    }
    if (e == hipSuccess && rc == GF_OK) {
        N = RG_TILE;
        while (N < maxnnz) N <<= 1;
        e = buf.get(&d_vals, sizeof(double) * (size_t)N * nchains);
        if (e == hipSuccess) e = buf.get(&d_idx, sizeof(int32_t) * (size_t)N * nchains);
    }
    if (e == hipSuccess && rc == GF_OK) {
        const int64_t all = N * nchains;
        hipLaunchKernelGGL(k_region_compact, per_chain, dim3(RG_BLOCK), 0, st, H, nb3, N, d_cursor, d_vals, d_idx);
        hipLaunchKernelGGL(k_region_pad, dim3(rg_grid(N) > 4096 ? 4096 : rg_grid(N), nchains), dim3(RG_BLOCK), 0, st, d_nnz, N, d_vals, d_idx);
        const unsigned tiles = (unsigned)(all / RG_TILE);
        hipLaunchKernelGGL(k_region_sort_tile, dim3(tiles), dim3(RG_BLOCK), 0, st, d_vals, d_idx, N, (int64_t)2, (int64_t)RG_TILE);
        for (int64_t k = 2 * (int64_t)RG_TILE; k <= N; k <<= 1) {
            for (int64_t j = k >> 1; j >= RG_TILE; j >>= 1)
                hipLaunchKernelGGL(k_region_sort_step, dim3(rg_grid(all / 2)), dim3(RG_BLOCK), 0, st, d_vals, d_idx, all / 2, N, k, j);
            hipLaunchKernelGGL(k_region_sort_tile, dim3(tiles), dim3(RG_BLOCK), 0, st, d_vals, d_idx, N, k, k);
        }
        hipLaunchKernelGGL(k_region_scan, dim3(nchains), dim3(RG_BLOCK), 0, st, d_vals, d_nnz, N, cov, d_thres, d_sat, d_lin, d_lout, d_mass);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(h_small.data() + 8 * n_u64, d_small + 8 * n_u64, small_bytes - 8 * n_u64, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess && rc == GF_OK) {
        const long long* h_thres = reinterpret_cast<const long long*>(h_small.data() + 8 * n_u64);
        const double* h_lin = reinterpret_cast<const double*>(h_thres + nres);
        const double *h_lout = h_lin + nres, *h_mass = h_lout + nres;
        const int32_t* h_sat = reinterpret_cast<const int32_t*>(h_mass + nres);
        std::vector<long long> h_take(one_list ? nchains : 0, 0);
        for (int ch = 0; ch < nchains && e == hipSuccess; ++ch)
            for (int q = 0; q < ncov && e == hipSuccess; ++q) {
                const int src = ch * ncov + q, dst = ch * ncov + order[q];
                if (thres) thres[dst] = h_thres[src];
                if (saturated) saturated[dst] = h_sat[src];
                if (level_in) level_in[dst] = h_lin[src];
                if (level_out) level_out[dst] = h_lout[src];
                if (mass) mass[dst] = h_mass[src];
                // the region is a prefix of the chain's sorted cells: the first min(thres, cap) of them, nothing past them
                if (one_list) {
                    h_take[ch] = std::max<long long>(h_take[ch], h_thres[src]);
                    continue;
                }
                const size_t take = (size_t)std::min<int64_t>(h_thres[src], cap);
                if (take && cells)
                    e = hipMemcpyAsync(cells + (size_t)dst * cap, d_idx + (size_t)ch * N, sizeof(int32_t) * take, hipMemcpyDeviceToHost, st);
                if (take && density && e == hipSuccess)
                    e = hipMemcpyAsync(density + (size_t)dst * cap, d_vals + (size_t)ch * N, sizeof(double) * take, hipMemcpyDeviceToHost, st);
            }
        if (one_list && cap > 0 && (cells || density) && e == hipSuccess) {
            // cells / density are host arrays [nchains][cap]: gather on the device, then one copy each
            GfScratch gathered(GF_MEM_CACHED);
            long long* d_take = nullptr;
            int32_t* d_cells = nullptr;
            double* d_dens = nullptr;
            const size_t nout = (size_t)nchains * (size_t)cap;
            e = gathered.get(&d_take, sizeof(long long) * nchains);
            if (e == hipSuccess && cells) e = gathered.get(&d_cells, sizeof(int32_t) * nout);
            if (e == hipSuccess && density) e = gathered.get(&d_dens, sizeof(double) * nout);
            if (e == hipSuccess && d_cells) e = hipMemsetAsync(d_cells, 0xff, sizeof(int32_t) * nout, st);           // -1 past the list
            if (e == hipSuccess && d_dens) e = hipMemsetAsync(d_dens, 0, sizeof(double) * nout, st);
            if (e == hipSuccess) e = hipMemcpyAsync(d_take, h_take.data(), sizeof(long long) * nchains, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_region_gather, dim3(rg_grid(cap) > 64 ? 64 : rg_grid(cap), nchains), dim3(RG_BLOCK), 0, st, d_vals, d_idx, N,
                                   d_take, cap, d_cells, d_dens);
                e = hipGetLastError();
            }
            if (e == hipSuccess && cells) e = hipMemcpyAsync(cells, d_cells, sizeof(int32_t) * nout, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && density) e = hipMemcpyAsync(density, d_dens, sizeof(double) * nout, hipMemcpyDeviceToHost, st);
            const hipError_t e3 = hipStreamSynchronize(st);
            if (e == hipSuccess) e = e3;
        }
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    } else {
        (void)hipStreamSynchronize(st);
    }
    if (rc != GF_OK) return rc;
    if (e != hipSuccess) return gf_hip_fail(e, "flavor region");
    return GF_OK;
}

int gf_region_run(hipStream_t st, const uint64_t* d_counts, int nchains, int nb, int radius, const double* weights, const double* coverage,
                  int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                  int32_t* cells, double* density, double* d_smoothed)
{
    return gf_region_run_shape(st, d_counts, nchains, nb, nb, nb, radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out,
                               mass, cells, density, d_smoothed, 0);
}

extern "C" {

int gf_flavor_region_device(gf_model* m, const uint64_t* d_counts, int nchains, int nbins, int radius, const double* weights,
                            const double* coverage, int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in,
                            double* level_out, double* mass, int32_t* cells, double* density, double* d_smoothed)
{
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    int rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);          // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    return gf_region_run((hipStream_t)stream, d_counts, nchains, nbins, radius, weights, coverage, ncov, cap, thres, saturated, level_in,
                         level_out, mass, cells, density, d_smoothed);
}

// host compositions fr [n][3] -> histogram -> region of that one chain
int gf_flavor_region(gf_model* m, const double* fr, int64_t n, int nbins, int radius, const double* weights, const double* coverage,
                     int ncov, int64_t cap, int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass,
                     int32_t* cells, double* density, double* d_smoothed)
{
    if (n < 0 || (n > 0 && !fr)) return GF_ERR_INVALID_ARG;
    int rc = gf_region_check_args(1, nbins, radius, weights, coverage, ncov, cap);
    if (rc != GF_OK) return rc;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t nb3 = (size_t)nbins * nbins * nbins;
    GfScratch buf(GF_MEM_CACHED);
    double* d_fr = nullptr;
    uint64_t* d_c = nullptr;
    hipError_t e = buf.get(&d_c, sizeof(uint64_t) * nb3);
    if (e == hipSuccess) e = hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nb3, st);
    if (e == hipSuccess && n > 0) e = buf.get(&d_fr, sizeof(double) * 3 * (size_t)n);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_fr, fr, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n > 0) e = gf_launch_flavor_hist(d_fr, n, nbins, (unsigned long long*)d_c, 256, st);
    if (e == hipSuccess)
        rc = gf_region_run(st, d_c, 1, nbins, radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density,
                           d_smoothed);
    else
        (void)hipStreamSynchronize(st);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_flavor_region");
    return rc;
}

}  // extern "C"
