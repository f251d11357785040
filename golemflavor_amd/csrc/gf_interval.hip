// gf_interval.hip -- the reference's shortest interval around the mode (golemflavor/misc.py:174-213) of every column of every chain
// on the device, and the sorted columns it needs (np.unique(samples[:, 0]).shape of mcmc.py:47 comes with them).  The definition,
// operation by operation, is gf_interval.hpp's; this file brings a batch of chains into sorted columns and evaluates it.
//   keys     rows [nrows][W] read coalesced, transposed through LDS, one order-preserving 64-bit key array per (chain, column)
//            (gf_marginal.hip's mg_key; every NaN becomes the largest key); a NaN or an infinity raises the column's flag
//   sort     segmented LSD radix sort, 8-bit digits, 8 passes, every (chain, column) segment of a batch in the same launches: per
//            pass a digit histogram per tile of 4096 keys, an exclusive scan over (digit, tile) per segment, a stable scatter with
//            in-tile ranks from wave ballots plus per-wave LDS counters.  Every dependency between workgroups is a kernel boundary.
//            Keys are totally ordered and carry no payload: the result does not depend on the grid or the batch.  The last pass
//            writes doubles.
//   unique   an integer count over adjacent pairs
//   mode     one wave per segment: end values and percentiles by indexing, nbins, a streamed arg-max over the bins (63 bins per
//            round, one edge per lane, the neighbour's position by shuffle, the first maximum kept), the centre, the start index
//   walk     one wave per segment: the lanes stage the values left and right of the window into LDS, one lane walks
//            (misc.py:199-212, sequential by definition) and records (low, up) as each requested length is reached
// Scratch: two key buffers per batch of chains from the library's device cache; chains are processed batch after batch so that
// the two stay under GF_INTERVAL_SCRATCH_DEFAULT (2 GiB; one chain at least).  GF_INTERVAL_SCRATCH_BYTES overrides the cap: it
// changes the batching, never a result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_interval.h"
#include "gf_interval.hpp"

namespace {

constexpr int IV_BLOCK = 256;
constexpr int IV_KPT = 16;                       // keys per thread
constexpr int IV_TILE = IV_BLOCK * IV_KPT;       // 4096 keys per tile
constexpr int IV_WAVES = IV_BLOCK / 64;
constexpr int IV_WAVE_KEYS = IV_TILE / IV_WAVES; // a wave's contiguous share of a tile
constexpr int IV_MAXW = GF_ELEMENT_MAX_WIDTH;
constexpr int IV_PAD = IV_BLOCK + 1;             // the transposing tile's row length in LDS
constexpr int IV_STAGE = 1024;                   // values staged on each side of the walk's window
constexpr int IV_P = GF_INTERVAL_MAX_PERCENTILES;

// a total order on the doubles as unsigned integers (gf_marginal.hip's mg_key: -0.0 just below +0.0); every NaN last
__device__ __forceinline__ unsigned long long iv_key(double v)
{
    if (v != v) return ~0ull;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double iv_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// grid (slabs of 256 rows, chains).  keys [chain][W][n]; flags [chain][W]
__global__ __launch_bounds__(IV_BLOCK) void k_iv_keys(const double* __restrict__ rows_all, int64_t chain_stride, int64_t n, int W,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ flags)
{
    extern __shared__ double iv_lds[];                                // [W][IV_PAD]
    const int ch = blockIdx.y, tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * IV_BLOCK;
    const int nr = (int)(n - r0 < IV_BLOCK ? n - r0 : IV_BLOCK);
    const double* src = rows_all + (size_t)ch * chain_stride + r0 * W;
    for (int idx = tid; idx < nr * W; idx += IV_BLOCK) {
        const int r = idx / W, c = idx - r * W;
        iv_lds[c * IV_PAD + r] = src[idx];
    }
    __syncthreads();
    for (int c = 0; c < W; ++c) {
        const bool have = tid < nr;
        const double v = have ? iv_lds[c * IV_PAD + tid] : 0.0;
        if (have) keys[((size_t)ch * W + c) * n + r0 + tid] = iv_key(v);
        if (__any(have && !gfiv::finite(v)) && (tid & 63) == 0) atomicOr(flags + (size_t)ch * W + c, 1);
    }
}

// grid (tiles, segments): hist [segment][tile][256]
__global__ __launch_bounds__(IV_BLOCK) void k_iv_hist(const unsigned long long* __restrict__ keys, int64_t n, int shift, unsigned int* __restrict__ hist)
{
    __shared__ unsigned int h[256];
    const int tid = threadIdx.x;
    const size_t seg = blockIdx.y;
    h[tid] = 0u;
    __syncthreads();
    const unsigned long long* k = keys + seg * n;
    const int64_t base = (int64_t)blockIdx.x * IV_TILE;
    for (int r = 0; r < IV_KPT; ++r) {
        const int64_t i = base + r * IV_BLOCK + tid;
        if (i < n) atomicAdd(h + (int)((k[i] >> shift) & 255ull), 1u);
    }
    __syncthreads();
    hist[(seg * gridDim.x + blockIdx.x) * 256 + tid] = h[tid];
}

// grid (segments), thread = digit: counts -> exclusive offsets in (digit, tile) order, in place
__global__ __launch_bounds__(256) void k_iv_scan(unsigned int* __restrict__ hist, int ntiles)
{
    __shared__ unsigned int tot[256];
    const int d = threadIdx.x;
    unsigned int* h = hist + (size_t)blockIdx.x * ntiles * 256;
    unsigned int sum = 0u;
    for (int t = 0; t < ntiles; ++t) sum += h[(size_t)t * 256 + d];
    tot[d] = sum;
    __syncthreads();
    if (d == 0) {
        unsigned int run = 0u;
        for (int q = 0; q < 256; ++q) { const unsigned int c = tot[q]; tot[q] = run; run += c; }
    }
    __syncthreads();
    unsigned int run = tot[d];
    for (int t = 0; t < ntiles; ++t) {
        const unsigned int c = h[(size_t)t * 256 + d];
        h[(size_t)t * 256 + d] = run;
        run += c;
    }
}

// grid (tiles, segments).  A wave owns a contiguous quarter of the tile and goes through it in rounds of 64 keys: a key's rank among
// its tile's keys of the same digit = the earlier waves' totals + its wave's count in earlier rounds (an LDS counter) + the lower
// lanes of its round with that digit (ballots).  LAST: the destination takes doubles.
template <bool LAST>
__global__ __launch_bounds__(IV_BLOCK) void k_iv_scatter(const unsigned long long* __restrict__ in, int64_t n, int shift,
                                                         const unsigned int* __restrict__ hist, unsigned long long* __restrict__ out)
{
    __shared__ volatile unsigned int cnt[IV_WAVES][256];
    __shared__ unsigned int base[IV_WAVES][256];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t seg = blockIdx.y;
    for (int q = 0; q < IV_WAVES; ++q) cnt[q][tid] = 0u;
    __syncthreads();
    const unsigned long long* k = in + seg * n;
    const int64_t first = (int64_t)blockIdx.x * IV_TILE + (int64_t)w * IV_WAVE_KEYS + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long key[IV_KPT];
    unsigned int rank[IV_KPT];
#pragma unroll
    for (int r = 0; r < IV_KPT; ++r) {
        const int64_t i = first + r * 64;
        const bool valid = i < n;
        key[r] = valid ? k[i] : 0ull;
        const int d = (int)((key[r] >> shift) & 255ull);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned int old = cnt[w][d];
        rank[r] = old + (unsigned int)__popcll(peers & below);
        if (valid && (peers & below) == 0ull) cnt[w][d] = old + (unsigned int)__popcll(peers);
    }
    __syncthreads();
    {
        unsigned int run = hist[(seg * gridDim.x + blockIdx.x) * 256 + tid];
        for (int q = 0; q < IV_WAVES; ++q) { base[q][tid] = run; run += cnt[q][tid]; }
    }
    __syncthreads();
    unsigned long long* o = out + seg * n;
#pragma unroll
    for (int r = 0; r < IV_KPT; ++r) {
        const int64_t i = first + r * 64;
        if (i < n) {
            const int d = (int)((key[r] >> shift) & 255ull);
            const int64_t dst = (int64_t)base[w][d] + rank[r];
            if (dst < n) o[dst] = LAST ? (unsigned long long)__double_as_longlong(iv_unkey(key[r])) : key[r];
        }
    }
}

// grid (tiles, segments): nunique [segment] += the tile's i >= 1 with s[i] != s[i - 1] (integers: the order of the atomics changes nothing)
__global__ __launch_bounds__(IV_BLOCK) void k_iv_unique(const double* __restrict__ sorted, int64_t n, unsigned long long* __restrict__ nunique)
{
    const size_t seg = blockIdx.y;
    const double* s = sorted + seg * n;
    const int64_t base = (int64_t)blockIdx.x * IV_TILE;
    unsigned int c = 0u;
    for (int r = 0; r < IV_KPT; ++r) {
        const int64_t i = base + r * IV_BLOCK + threadIdx.x;
        if (i >= 1 && i < n) c += s[i] != s[i - 1];
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(nunique + seg, (unsigned long long)c);
}

struct IvSeg {                           // per segment, device
    double center;
    int64_t nbins, start;
    int32_t status, pad;
};

// grid (segments), one wave
__global__ __launch_bounds__(64) void k_iv_mode(const double* __restrict__ sorted, int64_t n, double pw, const int* __restrict__ flags, IvSeg* __restrict__ segs)
{
    const size_t seg = blockIdx.x;
    const int lane = threadIdx.x;
    const double* s = sorted + seg * n;
    IvSeg r;
    r.center = gfiv::nan(); r.nbins = -1; r.start = 0; r.status = gfiv::ST_NONFINITE; r.pad = 0;
    if (flags[seg] == 0) {
        const double nbv = gfiv::nbins_value(s, n, pw);
        r.nbins = gfiv::nbins_reported(nbv);
        r.status = gfiv::nbins_status(nbv);
        if (r.status == gfiv::ST_OK) {
            const gfiv::Edges e = gfiv::edges(s, n, (int64_t)nbv);
            long long best = 0, best_count = -1;
            for (int64_t b0 = 0; b0 < e.nb; b0 += 63) {                // uniform trips
                const int64_t b = b0 + lane;
                const long long pos = b <= e.nb ? (long long)gfiv::position(s, n, e, b) : (long long)n;
                const long long next = __shfl_down(pos, 1);
                long long c = (lane < 63 && b < e.nb) ? next - pos : -1;
                long long cb = b;
                for (int off = 32; off > 0; off >>= 1) {              // the largest count, the lowest bin among equals
                    const long long oc = __shfl_down(c, off), ob = __shfl_down(cb, off);
                    if (oc > c || (oc == c && ob < cb)) { c = oc; cb = ob; }
                }
                c = __shfl(c, 0); cb = __shfl(cb, 0);
                if (c > best_count) { best_count = c; best = cb; }
            }
            r.center = gfiv::bin_center(e, best);
            r.start = gfiv::start_index(s, n, r.center);
        }
    }
    if (lane == 0) segs[seg] = r;
}

struct IvWalk {
    double thr[IV_P];                    // ascending
    int32_t order[IV_P];                 // thr[k] belongs to the caller's percentile order[k]
    int32_t npct;
};

// grid (segments), one wave.  low, up, status [segment][npct]
__global__ __launch_bounds__(64) void k_iv_walk(const double* __restrict__ sorted, int64_t n, const IvSeg* __restrict__ segs, const IvWalk P,
                                                double* __restrict__ low_out, double* __restrict__ up_out, int32_t* __restrict__ status_out)
{
    __shared__ double L[IV_STAGE], R[IV_STAGE];
    __shared__ long long sh_low, sh_up;
    __shared__ int sh_k, sh_done;
    const size_t seg = blockIdx.x;
    const int lane = threadIdx.x, npct = P.npct;
    const double* s = sorted + seg * n;
    const IvSeg g = segs[seg];
    double* lo_o = low_out + seg * npct;
    double* up_o = up_out + seg * npct;
    int32_t* st_o = status_out + seg * npct;
    if (g.status != gfiv::ST_OK) {
        if (lane < npct) { lo_o[lane] = gfiv::nan(); up_o[lane] = gfiv::nan(); st_o[lane] = g.status; }
        return;
    }
    long long low = g.start, up = g.start;
    int k = 0;
    for (;;) {                                                        // uniform: the state comes back through LDS
        const long long lbase = low + 1 - IV_STAGE, rbase = up;       // L holds s[lbase ..], low its last; R holds s[rbase ..], up its first
        for (int j = lane; j < IV_STAGE; j += 64) {
            const long long il = lbase + j, ir = rbase + j;
            L[j] = (il >= 0 && il < n) ? s[il] : 0.0;
            R[j] = ir < n ? s[ir] : 0.0;
        }
        __syncthreads();
        if (lane == 0) {
            int done = 0;
            for (;;) {
                while (k < npct && gfiv::reached(low, up, P.thr[k])) {
                    lo_o[P.order[k]] = L[low - lbase]; up_o[P.order[k]] = R[up - rbase]; st_o[P.order[k]] = gfiv::ST_OK;
                    ++k;
                }
                if (k == npct) { done = 1; break; }
                if (low == 0 && up == n - 1) {
                    for (; k < npct; ++k) { lo_o[P.order[k]] = gfiv::nan(); up_o[P.order[k]] = gfiv::nan(); st_o[P.order[k]] = gfiv::ST_INDEX; }
                    done = 1;
                    break;
                }
                if ((low > 0 && low - 1 < lbase) || (up < n - 1 && up + 1 >= rbase + IV_STAGE)) break;      // stage again
                const int d = gfiv::walk_dir(low, up, n, low > 0 ? L[low - 1 - lbase] : 0.0, L[low - lbase], R[up - rbase], up < n - 1 ? R[up + 1 - rbase] : 0.0);
                if (d < 0) --low; else ++up;
            }
            sh_low = low; sh_up = up; sh_k = k; sh_done = done;
        }
        __syncthreads();
        low = sh_low; up = sh_up; k = sh_k;
        if (sh_done) break;
        __syncthreads();                                              // every lane has read the state before L and R change
    }
}

size_t iv_scratch_cap()
{
    const char* v = gf_internal_env("GF_INTERVAL_SCRATCH_BYTES", 0);
    if (v) {
        const long long b = std::atoll(v);
        if (b > 0) return (size_t)b;
    }
    return (size_t)GF_INTERVAL_SCRATCH_DEFAULT;
}

}  // namespace

int gf_interval_check_args(int nchains, int64_t nrows, int W, const gf_interval_spec* sp)
{
    if (nchains < 1 || nrows < 1 || W < 1 || W > IV_MAXW) return GF_ERR_INVALID_ARG;
    if (sp) {
        if (sp->npct < 1 || sp->npct > IV_P || !sp->percentile) return GF_ERR_INVALID_ARG;
        for (int k = 0; k < sp->npct; ++k)
            if (!(sp->percentile[k] > 0.0 && sp->percentile[k] <= 100.0)) return GF_ERR_INVALID_ARG;
    }
    if (nrows >= ((int64_t)1 << 31)) return gf_fail_msg(GF_ERR_UNSUPPORTED, "intervals: 2^31 rows or more per chain");
    return GF_OK;
}

int gf_interval_run(hipStream_t st, const double* d_rows, int64_t chain_stride, int nchains, int64_t nrows, int W, const gf_interval_spec* sp,
                    const gf_interval_out* out, double* d_sorted)
{
    const int rc = gf_interval_check_args(nchains, nrows, W, sp);
    if (rc != GF_OK) return rc;
    if (!d_rows || ((uintptr_t)d_rows % 8) || (nchains > 1 && chain_stride < nrows * W) || (!sp && !d_sorted) || (sp && !out)) return GF_ERR_INVALID_ARG;
    const int64_t n = nrows;
    const int npct = sp ? sp->npct : 0;
    const size_t chain_keys = (size_t)W * n;
    const int ntiles = (int)((n + IV_TILE - 1) / IV_TILE);
    int bchains = (int)std::min<size_t>((size_t)nchains, std::max<size_t>(1, iv_scratch_cap() / (2 * sizeof(uint64_t) * chain_keys)));
    bchains = std::max(1, std::min(bchains, 65535 / W));
    const size_t bsegs = (size_t)bchains * W;
    GfScratch buf(GF_MEM_CACHED);
    unsigned long long *d_a = nullptr, *d_b = nullptr, *d_nuniq = nullptr;
    unsigned int* d_hist = nullptr;
    int* d_flags = nullptr;
    IvSeg* d_seg = nullptr;
    double *d_low = nullptr, *d_up = nullptr;
    int32_t* d_status = nullptr;
    hipError_t e = buf.get(&d_a, sizeof(uint64_t) * chain_keys * bchains);
    if (e == hipSuccess) e = buf.get(&d_b, sizeof(uint64_t) * chain_keys * bchains);
    if (e == hipSuccess) e = buf.get(&d_hist, sizeof(unsigned int) * bsegs * ntiles * 256);
    if (e == hipSuccess) e = buf.get(&d_flags, sizeof(int) * bsegs);
    if (e == hipSuccess) e = buf.get(&d_nuniq, sizeof(uint64_t) * bsegs);
    if (e == hipSuccess) e = buf.get(&d_seg, sizeof(IvSeg) * bsegs);
    if (e == hipSuccess) e = buf.get(&d_low, sizeof(double) * bsegs * std::max(npct, 1));
    if (e == hipSuccess) e = buf.get(&d_up, sizeof(double) * bsegs * std::max(npct, 1));
    if (e == hipSuccess) e = buf.get(&d_status, sizeof(int32_t) * bsegs * std::max(npct, 1));
    if (e != hipSuccess) return gf_fail_msg(GF_ERR_ALLOC, "intervals: %zu bytes of key buffers for %d chains not granted", 2 * sizeof(uint64_t) * chain_keys * bchains, bchains);

    IvWalk wk;
    std::memset(&wk, 0, sizeof(wk));
    wk.npct = npct;
    for (int k = 0; k < npct; ++k) wk.order[k] = k;
    std::stable_sort(wk.order, wk.order + npct, [&](int a, int b) { return gfiv::threshold(sp->percentile[a], n) < gfiv::threshold(sp->percentile[b], n); });
    for (int k = 0; k < npct; ++k) wk.thr[k] = gfiv::threshold(sp->percentile[wk.order[k]], n);
    const double pw = std::pow((double)n, -1. / 3);

    std::vector<IvSeg> h_seg(bsegs);
    std::vector<int> h_flags(bsegs);
    std::vector<unsigned long long> h_nuniq(bsegs);
    std::vector<double> h_low(bsegs * std::max(npct, 1)), h_up(bsegs * std::max(npct, 1));
    std::vector<int32_t> h_status(bsegs * std::max(npct, 1));
    for (int ch0 = 0; ch0 < nchains && e == hipSuccess; ch0 += bchains) {
        const int nb = std::min(bchains, nchains - ch0);
        const unsigned nseg = (unsigned)(nb * W);
        e = hipMemsetAsync(d_flags, 0, sizeof(int) * nseg, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_nuniq, 0, sizeof(uint64_t) * nseg, st);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_iv_keys, dim3((unsigned)((n + IV_BLOCK - 1) / IV_BLOCK), (unsigned)nb), dim3(IV_BLOCK), sizeof(double) * W * IV_PAD, st,
                           d_rows + (size_t)ch0 * chain_stride, chain_stride, n, W, d_a, d_flags);
        // a -> b -> a ... ; the last pass writes the doubles, into a or into the caller's block
        double* sorted = d_sorted ? d_sorted + (size_t)ch0 * chain_keys : reinterpret_cast<double*>(d_a);
        for (int pass = 0; pass < 8; ++pass) {
            const unsigned long long* src = (pass & 1) ? d_b : d_a;
            unsigned long long* dst = (pass & 1) ? d_a : d_b;
            const dim3 grid((unsigned)ntiles, nseg);
            hipLaunchKernelGGL(k_iv_hist, grid, dim3(IV_BLOCK), 0, st, src, n, 8 * pass, d_hist);
            hipLaunchKernelGGL(k_iv_scan, dim3(nseg), dim3(256), 0, st, d_hist, ntiles);
            if (pass < 7) hipLaunchKernelGGL(k_iv_scatter<false>, grid, dim3(IV_BLOCK), 0, st, src, n, 8 * pass, d_hist, dst);
            else hipLaunchKernelGGL(k_iv_scatter<true>, grid, dim3(IV_BLOCK), 0, st, src, n, 8 * pass, d_hist, reinterpret_cast<unsigned long long*>(sorted));
        }
        e = hipGetLastError();
        if (e != hipSuccess || !sp) continue;
        hipLaunchKernelGGL(k_iv_unique, dim3((unsigned)ntiles, nseg), dim3(IV_BLOCK), 0, st, sorted, n, d_nuniq);
        hipLaunchKernelGGL(k_iv_mode, dim3(nseg), dim3(64), 0, st, sorted, n, pw, d_flags, d_seg);
        hipLaunchKernelGGL(k_iv_walk, dim3(nseg), dim3(64), 0, st, sorted, n, d_seg, wk, d_low, d_up, d_status);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_seg.data(), d_seg, sizeof(IvSeg) * nseg, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_flags.data(), d_flags, sizeof(int) * nseg, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_nuniq.data(), d_nuniq, sizeof(uint64_t) * nseg, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_low.data(), d_low, sizeof(double) * nseg * npct, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_up.data(), d_up, sizeof(double) * nseg * npct, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_status.data(), d_status, sizeof(int32_t) * nseg * npct, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) break;
        const size_t s0 = (size_t)ch0 * W;
        for (unsigned q = 0; q < nseg; ++q) {
            if (out->center) out->center[s0 + q] = h_seg[q].center;
            if (out->nbins) out->nbins[s0 + q] = h_seg[q].nbins;
            if (out->nunique) out->nunique[s0 + q] = h_flags[q] ? -1 : 1 + (int64_t)h_nuniq[q];
            for (int k = 0; k < npct; ++k) {
                if (out->low) out->low[(s0 + q) * npct + k] = h_low[(size_t)q * npct + k];
                if (out->up) out->up[(s0 + q) * npct + k] = h_up[(size_t)q * npct + k];
                if (out->status) out->status[(s0 + q) * npct + k] = h_status[(size_t)q * npct + k];
            }
        }
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, "intervals");
    return GF_OK;
}

extern "C" {

int gf_sort_columns_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, double* d_sorted)
{
    int rc = gf_interval_check_args(nchains, nrows, width, nullptr);
    if (rc != GF_OK) return rc;
    if (!d_sorted || ((uintptr_t)d_sorted % 8)) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);              // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    return gf_interval_run((hipStream_t)stream, d_rows, nrows * width, nchains, nrows, width, nullptr, nullptr, d_sorted);
}

int gf_column_intervals_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, const gf_interval_spec* spec,
                               const gf_interval_out* out)
{
    if (!spec || !out) return GF_ERR_INVALID_ARG;
    int rc = gf_interval_check_args(nchains, nrows, width, spec);
    if (rc != GF_OK) return rc;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    return gf_interval_run((hipStream_t)stream, d_rows, nrows * width, nchains, nrows, width, spec, out, nullptr);
}

int gf_column_intervals(gf_model* m, const double* rows, int64_t nrows, int width, const gf_interval_spec* spec, const gf_interval_out* out)
{
    if (!spec || !out || !rows) return GF_ERR_INVALID_ARG;
    int rc = gf_interval_check_args(1, nrows, width, spec);
    if (rc != GF_OK) return rc;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    GfScratch buf(GF_MEM_CACHED);
    double* d_rows = nullptr;
    const size_t bytes = sizeof(double) * (size_t)nrows * width;
    hipError_t e = buf.get(&d_rows, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_column_intervals");
    return gf_interval_run(st, d_rows, nrows * width, 1, nrows, width, spec, out, nullptr);
}

}  // extern "C"
