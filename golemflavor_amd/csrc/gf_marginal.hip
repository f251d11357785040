// gf_marginal.hip -- every chain's rows [nrows][W] reduced to its posterior marginals on the device: the numbers behind the triangle
// plot the reference's scripts end in (golemflavor/plot.py:450-469 plot_Tchain), so that no chain has to cross PCIe to be plotted or
// to be asked for a limit.  Per chain
//   histograms  counts1 [W][nb1] as np.histogram, counts2 [W (W - 1) / 2][nb2][nb2] as np.histogram2d (pairs i < j, lexicographic):
//               the bin is decided by comparison with the caller's edges, a multiplicative guess moved down / up (the rule of
//               k_flavor_hist, gf_kernels.hip); 32-bit counters in LDS, flushed by 64-bit vector atomics; the pairs are split
//               over workgroups (one pair at 50 x 50 is 10 KB of LDS), the groups of one slab of rows are neighbours in the grid;
//   moments     nvalid, mean, cov (ddof 1, centred on the device mean) over the rows without NaN, summed along ONE fixed tree:
//               leaves of MG_CHUNK rows (a lane adds its 16 rows in order, 6 shuffle levels, 4 waves in order), then the leaves
//               of a chain the same way -- the result does not depend on the grid or on the order of any atomic;
//   order statistics   the exact k-th smallest of a column's non-NaN values: most-significant-digit radix select on the
//               order-preserving key of the double, 8 passes of 8 bits, every column and rank advanced in the same pass, ranks
//               that still share a prefix share a digit histogram;
//   regions     gf_region.hip's stages on the batch of 1-D marginals, shape (1, 1, nb1), and of 2-D ones, shape (1, nb2, nb2).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_marginal.h"
#include "gf_region.h"

namespace {

constexpr int MG_BLOCK = 256;
constexpr int MG_LDS_BYTES = 65536;          // per workgroup: two fit a CU's 160 KiB
constexpr int MG_CHUNK = 4096;               // rows per leaf of the summation tree: 16 per lane
constexpr int MG_MAXW = GF_MAX_DIM + 3;      // a scan's rows: composition + sample
constexpr int MG_R = GF_MARGINAL_MAX_RANKS;
constexpr int MG_ADV_BLOCK = 320;            // >= MG_MAXW * MG_R = 304: one lane per (column, rank)
constexpr int MG_SEL_SLOTS = 60;             // (column, rank) digit histograms of 1 KiB a select workgroup holds

// ---- histograms --------------------------------------------------------------------------------------------------------------
// the bin b with e[b] <= v < e[b + 1], the last one closed on the right; -1: outside [e[0], e[nb]] or NaN
__device__ __forceinline__ int mg_bin(double v, const double* __restrict__ e, int nb, double inv)
{
    if (!(v >= e[0] && v <= e[nb])) return -1;
    int b = (int)((v - e[0]) * inv);                                // a guess: finite, within [0, nb (1 + eps)]
    b = b < 0 ? 0 : (b >= nb ? nb - 1 : b);
    while (b > 0 && v < e[b]) --b;
    while (b + 1 < nb && v >= e[b + 1]) ++b;
    return b;
}

struct MgHist {
    const double* rows;
    int64_t chain_stride, nrows;
    const double *e1, *e2;                   // device [W][nb + 1], followed by [W] nb / (hi - lo): the guess's scale
    unsigned long long *c1, *c2;
    int32_t W, nb1, nb2, npairs, ppg;        // ppg: pairs per group
};

// grid (pair groups, slabs, chains).  A lane holds one row in registers (the loops over MAXW are unrolled, so v[] and b[] are
// registers); group 0 also fills the 1-D histograms.
template <int MAXW>
__global__ __launch_bounds__(MG_BLOCK) void k_marg_hist(const MgHist P)
{
    extern __shared__ unsigned int mg_lds[];
    const int g = blockIdx.x, ch = blockIdx.z, W = P.W, nb1 = P.nb1, nb2 = P.nb2;
    const int p0 = g * P.ppg, p1 = p0 + P.ppg < P.npairs ? p0 + P.ppg : P.npairs;
    unsigned int* h1 = mg_lds;
    unsigned int* h2 = mg_lds + W * nb1;
    const int n1 = g == 0 ? W * nb1 : 0, n2 = (p1 > p0 ? p1 - p0 : 0) * nb2 * nb2;
    for (int e = threadIdx.x; e < n1; e += MG_BLOCK) h1[e] = 0u;
    for (int e = threadIdx.x; e < n2; e += MG_BLOCK) h2[e] = 0u;
    __syncthreads();
    const double* rows = P.rows + (size_t)ch * P.chain_stride;
    const double* inv1 = P.e1 + W * (nb1 + 1);
    const double* inv2 = P.e2 + W * (nb2 + 1);
    for (int64_t r = (int64_t)blockIdx.y * MG_BLOCK + threadIdx.x; r < P.nrows; r += (int64_t)gridDim.y * MG_BLOCK) {
        const double* x = rows + r * W;
        int b[MAXW];
#pragma unroll
        for (int c = 0; c < MAXW; ++c) {
            b[c] = -1;
            if (c < W) {
                const double v = x[c];
                b[c] = mg_bin(v, P.e2 + c * (nb2 + 1), nb2, inv2[c]);
                if (g == 0) {
                    const int b1 = mg_bin(v, P.e1 + c * (nb1 + 1), nb1, inv1[c]);
                    if (b1 >= 0) atomicAdd(h1 + c * nb1 + b1, 1u);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < MAXW - 1; ++i) {
#pragma unroll
            for (int j = i + 1; j < MAXW; ++j) {
                const int p = i * (2 * W - i - 1) / 2 + (j - i - 1);           // uniform: scalar arithmetic
                if (j < W && p >= p0 && p < p1 && b[i] >= 0 && b[j] >= 0) atomicAdd(h2 + ((p - p0) * nb2 + b[i]) * nb2 + b[j], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* c1 = P.c1 + (size_t)ch * W * nb1;
    unsigned long long* c2 = P.c2 + ((size_t)ch * P.npairs + p0) * nb2 * nb2;
    for (int e = threadIdx.x; e < n1; e += MG_BLOCK) { const unsigned int v = h1[e]; if (v) atomicAdd(c1 + e, (unsigned long long)v); }
    for (int e = threadIdx.x; e < n2; e += MG_BLOCK) { const unsigned int v = h2[e]; if (v) atomicAdd(c2 + e, (unsigned long long)v); }
}

// ---- moments -----------------------------------------------------------------------------------------------------------------
// the workgroup's sum of s over its 256 lanes in a fixed order: 6 shuffle levels in the wave, then wave 0 + 1 + 2 + 3; valid in
// every lane after the call.  `sm` is 4 doubles of LDS.
__device__ __forceinline__ double mg_block_sum(double s, double* sm)
{
    for (int off = 32; off > 0; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    return __dadd_rn(__dadd_rn(__dadd_rn(sm[0], sm[1]), sm[2]), sm[3]);
}

// Leaf sums.  grid (chunks, chains): partial [ch][chunk][W] = sum of the chunk's rows without NaN; nvalid and the per-column
// non-NaN counts are integers (atomics cannot change them).
template <int MAXW>
__global__ __launch_bounds__(MG_BLOCK) void k_marg_sum(const double* __restrict__ rows_all, int64_t chain_stride, int64_t nrows, int W,
                                                       int64_t nchunks, double* __restrict__ partial, unsigned long long* __restrict__ nvalid,
                                                       unsigned long long* __restrict__ ncol)
{
    __shared__ double sm[4];
    const int ch = blockIdx.y;
    const int64_t chunk = blockIdx.x;
    const double* rows = rows_all + (size_t)ch * chain_stride;
    double s[MAXW];
    unsigned int nc[MAXW];
#pragma unroll
    for (int c = 0; c < MAXW; ++c) { s[c] = 0.0; nc[c] = 0u; }
    unsigned int nv = 0u;
    for (int t = 0; t < MG_CHUNK / MG_BLOCK; ++t) {
        const int64_t r = chunk * MG_CHUNK + t * MG_BLOCK + threadIdx.x;
        if (r >= nrows) break;
        const double* x = rows + r * W;
        double v[MAXW];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < MAXW; ++c) {
            v[c] = c < W ? x[c] : 0.0;
            const bool num = v[c] == v[c];
            ok = ok && num;
            nc[c] += (c < W && num) ? 1u : 0u;
        }
        if (ok) {
            nv += 1u;
#pragma unroll
            for (int c = 0; c < MAXW; ++c) s[c] = __dadd_rn(s[c], v[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < MAXW; ++c) {
        if (c < W) {                                                 // uniform
            const double tot = mg_block_sum(s[c], sm);
            if (threadIdx.x == 0) partial[((size_t)ch * nchunks + chunk) * W + c] = tot;
            unsigned int n = nc[c];
            for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
            if ((threadIdx.x & 63) == 0 && n) atomicAdd(ncol + (size_t)ch * W + c, (unsigned long long)n);
        }
    }
    for (int off = 32; off > 0; off >>= 1) nv += __shfl_down(nv, off);
    if ((threadIdx.x & 63) == 0 && nv) atomicAdd(nvalid + ch, (unsigned long long)nv);
}

// Leaf sums of the centred products.  grid (chunks * W, chains), column i = blockIdx.x % W next to the other columns of the same
// chunk: partial [ch][chunk][i][W] = sum (x_i - m_i)(x_c - m_c), difference, product and sum each rounded once.
template <int MAXW>
__global__ __launch_bounds__(MG_BLOCK) void k_marg_cov(const double* __restrict__ rows_all, int64_t chain_stride, int64_t nrows, int W,
                                                       int64_t nchunks, const double* __restrict__ mean, double* __restrict__ partial)
{
    __shared__ double sm[4];
    const int ch = blockIdx.y;
    const int64_t chunk = blockIdx.x / W;
    const int i = (int)(blockIdx.x - chunk * W);
    const double* rows = rows_all + (size_t)ch * chain_stride;
    double s[MAXW], m[MAXW];
#pragma unroll
    for (int c = 0; c < MAXW; ++c) { s[c] = 0.0; m[c] = c < W ? mean[(size_t)ch * W + c] : 0.0; }
    const double mi = mean[(size_t)ch * W + i];
    for (int t = 0; t < MG_CHUNK / MG_BLOCK; ++t) {
        const int64_t r = chunk * MG_CHUNK + t * MG_BLOCK + threadIdx.x;
        if (r >= nrows) break;
        const double* x = rows + r * W;
        double v[MAXW];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < MAXW; ++c) {
            v[c] = c < W ? x[c] : 0.0;
            ok = ok && v[c] == v[c];
        }
        if (ok) {
            const double di = __dsub_rn(x[i], mi);
#pragma unroll
            for (int c = 0; c < MAXW; ++c) s[c] = __dadd_rn(s[c], __dmul_rn(di, __dsub_rn(v[c], m[c])));
        }
    }
#pragma unroll
    for (int c = 0; c < MAXW; ++c) {
        if (c < W) {
            const double tot = mg_block_sum(s[c], sm);
            if (threadIdx.x == 0) partial[(((size_t)ch * nchunks + chunk) * W + i) * W + c] = tot;
        }
    }
}

// The leaves of one item: grid (K, items), out [item][k] = sum over q of partial [item][q][k], lane t adds q = t, t + 256, ... in
// order, then the workgroup's tree.
__global__ __launch_bounds__(MG_BLOCK) void k_marg_reduce(const double* __restrict__ partial, int64_t nchunks, int K, double* __restrict__ out)
{
    __shared__ double sm[4];
    const int k = blockIdx.x, item = blockIdx.y;
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < nchunks; q += MG_BLOCK) s = __dadd_rn(s, partial[((size_t)item * nchunks + q) * K + k]);
    const double tot = mg_block_sum(s, sm);
    if (threadIdx.x == 0) out[(size_t)item * K + k] = tot;
}

// out [ch][k] = sum [ch][k] / (nvalid [ch] - ddof), NaN when that is not positive
__global__ __launch_bounds__(MG_BLOCK) void k_marg_divide(const double* __restrict__ sum, const unsigned long long* __restrict__ nvalid, int K,
                                                          int64_t total, int ddof, double* __restrict__ out)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t e = (int64_t)blockIdx.x * MG_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * MG_BLOCK) {
        const long long n = (long long)nvalid[e / K] - ddof;
        out[e] = n > 0 ? __ddiv_rn(sum[e], (double)n) : nan;
    }
}

// ---- order statistics ----------------------------------------------------------------------------------------------------------
// a total order on the non-NaN doubles as unsigned integers (-0.0 just below +0.0)
__device__ __forceinline__ unsigned long long mg_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double mg_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// state per (chain, column, rank slot): prefix = the digits found so far, krem = the rank among the values with that prefix,
// leader = the lowest slot of the column with the same prefix (its histogram serves all of them), -1 = no such order statistic
struct MgSelect {
    const double* rows;
    int64_t chain_stride, nrows;
    unsigned long long* prefix;
    unsigned long long* krem;
    int32_t* leader;
    unsigned long long* hist;                // [chain][W][R][256]
    double* ostat;
    int32_t W, R, cpg, pass;                 // cpg: columns per group
};

// grid (column groups, slabs, chains): digit `pass` (0 = most significant) of every value that matches a leader's prefix
__global__ __launch_bounds__(MG_BLOCK) void k_marg_select_hist(const MgSelect P)
{
    extern __shared__ unsigned int mg_lds[];                        // [cpg * R][256]
    __shared__ unsigned long long spre[MG_SEL_SLOTS];
    __shared__ int slead[MG_SEL_SLOTS];
    const int ch = blockIdx.z, W = P.W, R = P.R;
    const int c0 = blockIdx.x * P.cpg, c1 = c0 + P.cpg < W ? c0 + P.cpg : W;
    const int nslot = (c1 - c0) * R;
    for (int e = threadIdx.x; e < nslot * 256; e += MG_BLOCK) mg_lds[e] = 0u;
    for (int e = threadIdx.x; e < nslot; e += MG_BLOCK) {
        const size_t o = ((size_t)ch * W + c0) * R + e;
        spre[e] = P.prefix[o];
        slead[e] = P.leader[o];
    }
    __syncthreads();
    const double* rows = P.rows + (size_t)ch * P.chain_stride;
    const int lane = threadIdx.x & 63;
    const int hi_shift = 64 - 8 * P.pass, lo_shift = 56 - 8 * P.pass;
    for (int64_t base = (int64_t)blockIdx.y * MG_BLOCK; base < P.nrows; base += (int64_t)gridDim.y * MG_BLOCK) {      // uniform trips
        const int64_t r = base + threadIdx.x;
        for (int c = c0; c < c1; ++c) {
            const double v = r < P.nrows ? rows[r * W + c] : __longlong_as_double(0x7ff8000000000000ll);
            const bool num = v == v;
            const unsigned long long key = mg_key(v);
            const int digit = (int)((key >> lo_shift) & 255ull);
            for (int rr = 0; rr < R; ++rr) {
                const int slot = (c - c0) * R + rr;
                if (slead[slot] != rr) continue;                    // uniform
                const bool m = num && (P.pass == 0 || (key >> hi_shift) == spre[slot]);
                const unsigned long long mask = __ballot(m);
                if (mask == 0) continue;
                // the upper digits of a column's values are nearly all equal: a wave whose matching lanes agree adds once
                const int first = __ffsll((long long)mask) - 1;
                const int d0 = __shfl(digit, first);
                if (__all(!m || digit == d0)) {
                    if (lane == first) atomicAdd(mg_lds + slot * 256 + d0, (unsigned int)__popcll(mask));
                } else if (m) {
                    atomicAdd(mg_lds + slot * 256 + digit, 1u);
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* h = P.hist + ((size_t)ch * W + c0) * R * 256;
    for (int e = threadIdx.x; e < nslot * 256; e += MG_BLOCK) { const unsigned int v = mg_lds[e]; if (v) atomicAdd(h + e, (unsigned long long)v); }
}

// grid (chains), one lane per (column, rank): walk the leader's digit histogram to the digit that holds rank krem, extend the
// prefix, elect the leaders of the next pass; after the last pass the prefix is the key of the order statistic
__global__ __launch_bounds__(MG_ADV_BLOCK) void k_marg_select_advance(const MgSelect P)
{
    __shared__ unsigned long long spre[MG_MAXW * MG_R];
    __shared__ int salive[MG_MAXW * MG_R];
    const int ch = blockIdx.x, W = P.W, R = P.R, e = threadIdx.x, n = W * R;
    const size_t o = (size_t)ch * n + (e < n ? e : 0);
    const int c = e / R, rr = e - c * R;
    int lead = e < n ? P.leader[o] : -1;
    unsigned long long pre = 0, k = 0;
    if (lead >= 0) {
        pre = P.prefix[o];
        k = P.krem[o];
        const unsigned long long* h = P.hist + (((size_t)ch * W + c) * R + lead) * 256;
        unsigned long long cum = 0;
        int d = 0;
        for (; d < 256; ++d) {
            const unsigned long long cnt = h[d];
            if (k < cum + cnt) break;
            cum += cnt;
        }
        if (d < 256) { pre = (pre << 8) | (unsigned long long)d; k -= cum; }
        else lead = -1;                                             // a rank beyond the column's values: the host sends none
    }
    if (e < n) { spre[e] = pre; salive[e] = lead >= 0; }
    __syncthreads();
    if (e < n) {
        int nl = -1;
        if (lead >= 0)
            for (int q = 0; q <= rr; ++q)
                if (salive[c * R + q] && spre[c * R + q] == pre) { nl = q; break; }
        P.prefix[o] = pre;
        P.krem[o] = k;
        P.leader[o] = nl;
        if (P.pass == 7) P.ostat[o] = nl >= 0 ? mg_unkey(pre) : __longlong_as_double(0x7ff8000000000000ll);
    }
}

inline unsigned mg_grid(int64_t work_items, int64_t cap)
{
    const int64_t b = (work_items + MG_BLOCK - 1) / MG_BLOCK;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

// workgroups along the rows of one chain so that the whole grid is a few thousand workgroups
inline unsigned mg_slabs(int64_t nrows, int64_t others)
{
    int64_t want = 4096 / (others < 1 ? 1 : others);
    if (want < 1) want = 1;
    const int64_t have = (nrows + 4 * MG_BLOCK - 1) / (4 * MG_BLOCK);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, have), 65535));
}

template <typename F>
hipError_t mg_by_width(int W, F&& f)
{
    if (W <= 8) return f(std::integral_constant<int, 8>());
    if (W <= 12) return f(std::integral_constant<int, 12>());
    return f(std::integral_constant<int, MG_MAXW>());
}

}  // namespace

int gf_marginal_check_args(int nchains, int64_t nrows, int W, const gf_marginal_spec* sp)
{
    if (!sp || nchains < 1 || nchains > 65535 || nrows < 0 || W < 1 || W > MG_MAXW) return GF_ERR_INVALID_ARG;
    if (sp->nbins1 < 1 || sp->nbins2 < 1 || sp->nbins1 > 1024 || sp->nbins2 > 1024 || !sp->edges1 || !sp->edges2) return GF_ERR_INVALID_ARG;
    if (sp->nranks < 0 || sp->nq < 0 || (sp->nranks > 0 && !sp->ranks) || (sp->nq > 0 && !sp->q)) return GF_ERR_INVALID_ARG;
    if (sp->cap1 < 0 || sp->cap2 < 0) return GF_ERR_INVALID_ARG;
    for (int c = 0; c < W; ++c) {
        for (int b = 0; b <= sp->nbins1; ++b) {
            const double e = sp->edges1[(size_t)c * (sp->nbins1 + 1) + b];
            if (!std::isfinite(e) || (b > 0 && !(e > sp->edges1[(size_t)c * (sp->nbins1 + 1) + b - 1]))) return GF_ERR_INVALID_ARG;
        }
        for (int b = 0; b <= sp->nbins2; ++b) {
            const double e = sp->edges2[(size_t)c * (sp->nbins2 + 1) + b];
            if (!std::isfinite(e) || (b > 0 && !(e > sp->edges2[(size_t)c * (sp->nbins2 + 1) + b - 1]))) return GF_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < sp->nq; ++i)
        if (!(sp->q[i] >= 0.0 && sp->q[i] <= 100.0)) return GF_ERR_INVALID_ARG;
    int rc = gf_region_check_args(nchains, sp->nbins1, sp->radius, sp->weights, sp->coverage, sp->ncov, sp->cap1);
    if (rc == GF_OK) rc = gf_region_check_args(nchains, sp->nbins2, sp->radius, sp->weights, sp->coverage, sp->ncov, sp->cap2);
    if (rc != GF_OK) return rc;
    if (sp->nranks + 2 * sp->nq > MG_R)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "marginals: %d ranks + 2 x %d percentiles exceed GF_MARGINAL_MAX_RANKS = %d", sp->nranks, sp->nq, MG_R);
    if ((int64_t)4 * W * sp->nbins1 + (int64_t)4 * sp->nbins2 * sp->nbins2 > MG_LDS_BYTES)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "marginals: %d x %d 1-D bins and one %d x %d pair exceed %d bytes of LDS", W, sp->nbins1, sp->nbins2,
                           sp->nbins2, MG_LDS_BYTES);
    if (nrows >= ((int64_t)1 << 32)) return gf_fail_msg(GF_ERR_UNSUPPORTED, "marginals: 2^32 rows or more per chain");
    if ((nrows + MG_CHUNK - 1) / MG_CHUNK * W > 0x7fffffffll) return gf_fail_msg(GF_ERR_UNSUPPORTED, "marginals: too many rows per chain");
    return GF_OK;
}

int gf_marginal_run(hipStream_t st, const double* d_rows, int64_t chain_stride, int nchains, int64_t nrows, int W, const gf_marginal_spec* sp,
                    const gf_marginal_out* out)
{
    int rc = gf_marginal_check_args(nchains, nrows, W, sp);
    if (rc != GF_OK) return rc;
    if (!out || (nrows > 0 && (!d_rows || ((uintptr_t)d_rows % 8))) || chain_stride < nrows * W) return GF_ERR_INVALID_ARG;
    const int nb1 = sp->nbins1, nb2 = sp->nbins2, npairs = W * (W - 1) / 2, R = sp->nranks + 2 * sp->nq;
    const size_t n_c1 = (size_t)nchains * W * nb1, n_c2 = (size_t)nchains * npairs * nb2 * nb2;
    const int64_t nchunks = std::max<int64_t>(1, (nrows + MG_CHUNK - 1) / MG_CHUNK);
    GfScratch buf(GF_MEM_CACHED);
    double *d_e1 = nullptr, *d_e2 = nullptr, *d_part = nullptr, *d_sum = nullptr, *d_mean = nullptr, *d_part2 = nullptr, *d_sum2 = nullptr, *d_cov = nullptr;
    unsigned long long *d_c1 = nullptr, *d_c2 = nullptr, *d_nvalid = nullptr, *d_ncol = nullptr;
    hipError_t e = buf.get(&d_e1, sizeof(double) * W * (nb1 + 2));
    if (e == hipSuccess) e = buf.get(&d_e2, sizeof(double) * W * (nb2 + 2));
    if (e == hipSuccess) e = buf.get(&d_c1, sizeof(uint64_t) * n_c1);
    if (e == hipSuccess) e = buf.get(&d_c2, sizeof(uint64_t) * n_c2);
    if (e == hipSuccess) e = buf.get(&d_nvalid, sizeof(uint64_t) * nchains * (1 + (size_t)W));
    if (e == hipSuccess) e = buf.get(&d_part, sizeof(double) * nchains * nchunks * W);
    if (e == hipSuccess) e = buf.get(&d_sum, sizeof(double) * nchains * W);
    if (e == hipSuccess) e = buf.get(&d_mean, sizeof(double) * nchains * W);
    if (e == hipSuccess) e = buf.get(&d_part2, sizeof(double) * nchains * nchunks * W * W);
    if (e == hipSuccess) e = buf.get(&d_sum2, sizeof(double) * nchains * W * W);
    if (e == hipSuccess) e = buf.get(&d_cov, sizeof(double) * nchains * W * W);
    if (e != hipSuccess) return gf_hip_fail(e, "marginals: hipMalloc");
    d_ncol = d_nvalid + nchains;
    std::vector<double> h_e1(sp->edges1, sp->edges1 + (size_t)W * (nb1 + 1)), h_e2(sp->edges2, sp->edges2 + (size_t)W * (nb2 + 1));
    for (int c = 0; c < W; ++c) {
        h_e1.push_back(nb1 / (sp->edges1[(size_t)c * (nb1 + 1) + nb1] - sp->edges1[(size_t)c * (nb1 + 1)]));
        h_e2.push_back(nb2 / (sp->edges2[(size_t)c * (nb2 + 1) + nb2] - sp->edges2[(size_t)c * (nb2 + 1)]));
    }
    e = hipMemcpyAsync(d_e1, h_e1.data(), sizeof(double) * h_e1.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_e2, h_e2.data(), sizeof(double) * h_e2.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_c1, 0, sizeof(uint64_t) * n_c1, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_c2, 0, sizeof(uint64_t) * std::max<size_t>(n_c2, 1), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_nvalid, 0, sizeof(uint64_t) * nchains * (1 + (size_t)W), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_part, 0, sizeof(double) * nchains * nchunks * W, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_part2, 0, sizeof(double) * nchains * nchunks * W * W, st);
    if (e != hipSuccess) return gf_hip_fail(e, "marginals: setup");

    // histograms
    MgHist H;
    std::memset(&H, 0, sizeof(H));
    H.rows = d_rows; H.chain_stride = chain_stride; H.nrows = nrows; H.e1 = d_e1; H.e2 = d_e2; H.c1 = d_c1; H.c2 = d_c2;
    H.W = W; H.nb1 = nb1; H.nb2 = nb2; H.npairs = npairs;
    H.ppg = (int)((MG_LDS_BYTES - (int64_t)4 * W * nb1) / ((int64_t)4 * nb2 * nb2));                 // >= 1: checked
    const int ngroups = std::max(1, (npairs + H.ppg - 1) / H.ppg);
    const size_t hist_lds = (size_t)4 * W * nb1 + (size_t)4 * std::min(H.ppg, std::max(npairs, 0)) * nb2 * nb2;
    if (nrows > 0) {
        const dim3 grid((unsigned)ngroups, mg_slabs(nrows, (int64_t)ngroups * nchains), (unsigned)nchains);
        e = mg_by_width(W, [&](auto mw) {
            hipLaunchKernelGGL(k_marg_hist<decltype(mw)::value>, grid, dim3(MG_BLOCK), hist_lds, st, H);
            return hipGetLastError();
        });
        // moments: leaves, the chain's tree, the division; then the same for the centred products
        if (e == hipSuccess)
            e = mg_by_width(W, [&](auto mw) {
                hipLaunchKernelGGL(k_marg_sum<decltype(mw)::value>, dim3((unsigned)nchunks, (unsigned)nchains), dim3(MG_BLOCK), 0, st, d_rows,
                                   chain_stride, nrows, W, nchunks, d_part, d_nvalid, d_ncol);
                return hipGetLastError();
            });
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_marg_reduce, dim3((unsigned)W, (unsigned)nchains), dim3(MG_BLOCK), 0, st, d_part, nchunks, W, d_sum);
        hipLaunchKernelGGL(k_marg_divide, dim3(mg_grid((int64_t)nchains * W, 1024)), dim3(MG_BLOCK), 0, st, d_sum, d_nvalid, W, (int64_t)nchains * W, 0,
                           d_mean);
        e = hipGetLastError();
    }
    if (e == hipSuccess && nrows > 0)
        e = mg_by_width(W, [&](auto mw) {
            hipLaunchKernelGGL(k_marg_cov<decltype(mw)::value>, dim3((unsigned)(nchunks * W), (unsigned)nchains), dim3(MG_BLOCK), 0, st, d_rows,
                               chain_stride, nrows, W, nchunks, d_mean, d_part2);
            return hipGetLastError();
        });
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_marg_reduce, dim3((unsigned)(W * W), (unsigned)nchains), dim3(MG_BLOCK), 0, st, d_part2, nchunks, W * W, d_sum2);
        hipLaunchKernelGGL(k_marg_divide, dim3(mg_grid((int64_t)nchains * W * W, 1024)), dim3(MG_BLOCK), 0, st, d_sum2, d_nvalid, W * W,
                           (int64_t)nchains * W * W, 1, d_cov);
        e = hipGetLastError();
    }
    std::vector<unsigned long long> h_n((size_t)nchains * (1 + (size_t)W));
    if (e == hipSuccess) e = hipMemcpyAsync(h_n.data(), d_nvalid, sizeof(uint64_t) * h_n.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out->counts1) e = hipMemcpyAsync(out->counts1, d_c1, sizeof(uint64_t) * n_c1, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out->counts2 && n_c2) e = hipMemcpyAsync(out->counts2, d_c2, sizeof(uint64_t) * n_c2, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out->mean) e = hipMemcpyAsync(out->mean, d_mean, sizeof(double) * nchains * W, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out->cov) e = hipMemcpyAsync(out->cov, d_cov, sizeof(double) * nchains * W * W, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return gf_hip_fail(e, "marginals: histograms and moments"); }
    const unsigned long long* h_ncol = h_n.data() + nchains;
    for (int ch = 0; ch < nchains; ++ch) {
        if (out->nvalid) out->nvalid[ch] = (int64_t)h_n[ch];
        for (int c = 0; c < W && out->ncol; ++c) out->ncol[(size_t)ch * W + c] = (int64_t)h_ncol[(size_t)ch * W + c];
    }

    // order statistics
    if (R > 0 && (out->ostat || out->orank)) {
        const size_t nst = (size_t)nchains * W * R;
        std::vector<unsigned long long> h_k(nst, 0);
        std::vector<int32_t> h_lead(nst, -1);
        std::vector<int64_t> h_rank(nst, -1);
        for (int ch = 0; ch < nchains; ++ch)
            for (int c = 0; c < W; ++c) {
                const int64_t n = (int64_t)h_ncol[(size_t)ch * W + c];
                int first = -1;
                for (int rr = 0; rr < R; ++rr) {
                    int64_t k = -1;
                    if (rr < sp->nranks) {
                        k = sp->ranks[rr] >= 0 ? sp->ranks[rr] : n + sp->ranks[rr];
                    } else if (n > 0) {
                        // numpy's `linear`: virtual index (n - 1) * (q / 100), its floor and the next one, both n - 1 at the top
                        const double vi = (double)(n - 1) * (sp->q[(rr - sp->nranks) / 2] / 100.);
                        const int64_t lo = vi >= (double)(n - 1) ? n - 1 : (int64_t)std::floor(vi);
                        k = ((rr - sp->nranks) & 1) ? std::min<int64_t>(lo + 1, n - 1) : lo;
                    }
                    const size_t o = ((size_t)ch * W + c) * R + rr;
                    if (k < 0 || k >= n) continue;
                    if (first < 0) first = rr;
                    h_k[o] = (unsigned long long)k;
                    h_lead[o] = first;
                    h_rank[o] = k;
                }
            }
        MgSelect S;
        std::memset(&S, 0, sizeof(S));
        S.rows = d_rows; S.chain_stride = chain_stride; S.nrows = nrows; S.W = W; S.R = R;
        S.cpg = std::max(1, std::min(W, MG_SEL_SLOTS / R));
        e = buf.get(&S.prefix, sizeof(uint64_t) * nst);
        if (e == hipSuccess) e = buf.get(&S.krem, sizeof(uint64_t) * nst);
        if (e == hipSuccess) e = buf.get(&S.leader, sizeof(int32_t) * nst);
        if (e == hipSuccess) e = buf.get(&S.hist, sizeof(uint64_t) * nst * 256);
        if (e == hipSuccess) e = buf.get(&S.ostat, sizeof(double) * nst);
        if (e == hipSuccess) e = hipMemsetAsync(S.prefix, 0, sizeof(uint64_t) * nst, st);
        if (e == hipSuccess) e = hipMemcpyAsync(S.krem, h_k.data(), sizeof(uint64_t) * nst, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(S.leader, h_lead.data(), sizeof(int32_t) * nst, hipMemcpyHostToDevice, st);
        const int ncg = (W + S.cpg - 1) / S.cpg;
        const dim3 grid((unsigned)ncg, mg_slabs(nrows, (int64_t)ncg * nchains), (unsigned)nchains);
        for (int pass = 0; pass < 8 && e == hipSuccess; ++pass) {
            S.pass = pass;
            e = hipMemsetAsync(S.hist, 0, sizeof(uint64_t) * nst * 256, st);
            if (e != hipSuccess) break;
            if (nrows > 0) hipLaunchKernelGGL(k_marg_select_hist, grid, dim3(MG_BLOCK), (size_t)S.cpg * R * 1024, st, S);
            hipLaunchKernelGGL(k_marg_select_advance, dim3((unsigned)nchains), dim3(MG_ADV_BLOCK), 0, st, S);
            e = hipGetLastError();
        }
        if (e == hipSuccess && out->ostat) e = hipMemcpyAsync(out->ostat, S.ostat, sizeof(double) * nst, hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return gf_hip_fail(e, "marginals: order statistics");
        if (out->orank) std::memcpy(out->orank, h_rank.data(), sizeof(int64_t) * nst);
    }

    // regions: every 1-D marginal is a (1, 1, nb1) histogram, every 2-D one (1, nb2, nb2); batches of at most 32768 (grid.y)
    const int ncov = sp->ncov;
    constexpr int64_t BATCH = 32768;
    auto regions = [&](const unsigned long long* d_c, int64_t nmarg, int n1, int n2, int64_t cap, int64_t* thres, int32_t* sat, double* lin,
                       double* lout, double* mass, int32_t* cells, double* dens) -> int {
        if (!thres && !sat && !lin && !lout && !mass && !cells && !dens) return GF_OK;
        const int64_t per = (int64_t)n1 * n2;
        for (int64_t b0 = 0; b0 < nmarg; b0 += BATCH) {
            const int nb = (int)std::min<int64_t>(BATCH, nmarg - b0);
            const int r2 = gf_region_run_shape(st, (const uint64_t*)(d_c + b0 * per), nb, 1, n1, n2, sp->radius, sp->weights, sp->coverage, ncov, cap,
                                               thres ? thres + b0 * ncov : nullptr, sat ? sat + b0 * ncov : nullptr, lin ? lin + b0 * ncov : nullptr,
                                               lout ? lout + b0 * ncov : nullptr, mass ? mass + b0 * ncov : nullptr,
                                               cells ? cells + b0 * cap : nullptr, dens ? dens + b0 * cap : nullptr, nullptr, 1);
            if (r2 != GF_OK) return r2;
        }
        return GF_OK;
    };
    rc = regions(d_c1, (int64_t)nchains * W, 1, nb1, sp->cap1, out->thres1, out->saturated1, out->level_in1, out->level_out1, out->mass1,
                 out->cells1, out->density1);
    if (rc == GF_OK && npairs > 0)
        rc = regions(d_c2, (int64_t)nchains * npairs, nb2, nb2, sp->cap2, out->thres2, out->saturated2, out->level_in2, out->level_out2, out->mass2,
                     out->cells2, out->density2);
    return rc;
}

extern "C" {

int gf_marginals_device(gf_model* m, const double* d_rows, int nchains, int64_t nrows, int width, const gf_marginal_spec* spec,
                        const gf_marginal_out* out)
{
    int rc = gf_marginal_check_args(nchains, nrows, width, spec);
    if (rc != GF_OK) return rc;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);              // sets the device, gives the model its stream
    if (rc != GF_OK) return rc;
    return gf_marginal_run((hipStream_t)stream, d_rows, nrows * width, nchains, nrows, width, spec, out);
}

int gf_marginals(gf_model* m, const double* rows, int64_t nrows, int width, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    int rc = gf_marginal_check_args(1, nrows, width, spec);
    if (rc != GF_OK) return rc;
    if (nrows > 0 && !rows) return GF_ERR_INVALID_ARG;
    const GfCommon* c; const GfBsm* tb; const double* ptab; void* stream; int device;
    rc = gf_model_internal(m, &c, &tb, &ptab, &stream, &device);
    if (rc != GF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    GfScratch buf(GF_MEM_CACHED);
    double* d_rows = nullptr;
    const size_t bytes = sizeof(double) * (size_t)nrows * width;
    hipError_t e = buf.get(&d_rows, bytes);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(d_rows, rows, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_marginals");
    return gf_marginal_run(st, d_rows, nrows * width, 1, nrows, width, spec, out);
}

}  // extern "C"
