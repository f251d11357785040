// gf_weights.hip -- the kernels and launches of the weighted-sample pipeline that gf_weights.h describes; arithmetic
// and summation order are gf_nested_post.hpp's.  All runs go through one set of launches, blockIdx.y = run.
//   k_np_leaf<STAGE>   one workgroup per leaf of 4096 points (STAGE_COV: per leaf and column): max lnw | e = exp(lnw - m), sums of e
//                      and e^2 | p = e / S, sums of p, p^2, p theta | sums of p (theta_a - mean_a)(theta_b - mean_b)
//   k_np_run<STAGE>    one workgroup per run: the leaves of the run summed, and what follows the sums
//   k_np_scan_totals, _prefix, _add    the inclusive prefix C of p: block totals, their prefix, the sum of both; no workgroup waits
//   k_np_resample, k_np_rows           one lane per output row: the binary search of t_k in the run's C; the rows, lanes on columns
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_nested_post.hpp"
#include "gf_weights.h"

namespace {
using namespace gfnp;

constexpr int NP_BLOCK = LANES;
constexpr int NP_WAVE = 64;
enum { STAGE_MAX = 0, STAGE_EXP = 1, STAGE_MOM = 2, STAGE_COV = 3 };
enum { ST_M = GF_WST_M, ST_S = GF_WST_S, ST_S2 = GF_WST_S2, ST_ESS = GF_WST_ESS, ST_SP = GF_WST_SP, ST_SP2 = GF_WST_SP2, ST_FACT = GF_WST_FACT,
       NP_STAT = GF_WEIGHT_STAT };
static_assert(LEAF == GF_WEIGHT_LEAF && MAX_DIM == GF_MAX_DIM && NP_WAVE == GF_WEIGHT_TOT_PER_LEAF, "gf_weights.h states the header's sizes");
constexpr int np_stage_k(int stage) { return stage == STAGE_MAX ? 1 : stage == STAGE_EXP ? 2 : stage == STAGE_MOM ? 2 + MAX_DIM : MAX_DIM * MAX_DIM; }

using NpRun = GfWeightRun;
using NpArgs = GfWeightArgs;
static_assert(np_stage_k(STAGE_COV) == GF_WEIGHT_PART_COV && np_stage_k(STAGE_MOM) == GF_WEIGHT_PART, "gf_weights.h states the stages' sizes");

// the fold of the workgroup's 256 lane values (gf_nested_post.hpp fold_lanes); valid in every lane.  `sm`: 4 doubles of LDS
template <bool MAX>
__device__ __forceinline__ double np_fold(double s, double* sm)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_down(s, o);
        s = MAX ? (t > s ? t : s) : add(s, t);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (MAX) { const double p = sm[0] > sm[1] ? sm[0] : sm[1], q = sm[2] > sm[3] ? sm[2] : sm[3]; return p > q ? p : q; }
    return add(add(add(sm[0], sm[1]), sm[2]), sm[3]);
}

// grid (maxleaves, R); STAGE_COV: (maxleaves * ndim, R), column a = blockIdx.x % ndim
template <int STAGE>
__global__ __launch_bounds__(NP_BLOCK) void k_np_leaf(const NpArgs a)
{
    __shared__ double sm[4];
    constexpr int K = np_stage_k(STAGE), NS = STAGE == STAGE_MAX ? 1 : STAGE == STAGE_EXP ? 2 : STAGE == STAGE_MOM ? 2 + MAX_DIM : MAX_DIM;
    const int r = blockIdx.y, ndim = a.ndim;
    const NpRun R = a.runs[r];
    const int64_t leaf = STAGE == STAGE_COV ? blockIdx.x / ndim : blockIdx.x;
    const int ca = STAGE == STAGE_COV ? (int)(blockIdx.x - leaf * ndim) : 0;
    if (leaf * LEAF >= R.n) return;                                   // uniform
    const double* st = a.stat + (size_t)r * NP_STAT;
    const double m = STAGE == STAGE_EXP ? st[ST_M] : STAGE == STAGE_MOM ? st[ST_S] : 0.0;
    double s[NS], mean[MAX_DIM];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = STAGE == STAGE_MAX ? neg_inf() : 0.0;
    if (STAGE == STAGE_COV) {
#pragma unroll
        for (int c = 0; c < MAX_DIM; ++c) mean[c] = c < ndim ? a.mean[r * MAX_DIM + c] : 0.0;
    }
    const double ma = STAGE == STAGE_COV ? a.mean[r * MAX_DIM + ca] : 0.0;
    for (int j = 0; j < LEAF / NP_BLOCK; ++j) {
        const int64_t i = leaf * LEAF + j * NP_BLOCK + threadIdx.x;
        if (i >= R.n) break;
        const int64_t g = R.off + i;
        if constexpr (STAGE == STAGE_MAX) {
            const double v = a.lnw[g];
            s[0] = v > s[0] ? v : s[0];
        } else if constexpr (STAGE == STAGE_EXP) {
            const double e = weight(a.lnw[g], m);
            a.w[g] = e;
            s[0] = add(s[0], e);
            s[1] = add(s[1], square(e));
        } else if constexpr (STAGE == STAGE_MOM) {
            const double p = div(a.w[g], m);
            a.w[g] = p;
            s[0] = add(s[0], p);
            s[1] = add(s[1], square(p));
            const double* x = a.theta + (R.toff + i) * ndim;
#pragma unroll
            for (int c = 0; c < MAX_DIM; ++c)
                if (c < ndim) s[2 + c] = add(s[2 + c], term_mean(p, x[c]));
        } else {
            const double p = a.w[g];
            const double* x = a.theta + (R.toff + i) * ndim;
            const double xa = x[ca];
#pragma unroll
            for (int c = 0; c < MAX_DIM; ++c)
                if (c < ndim) s[c] = add(s[c], term_cov(p, xa, ma, x[c], mean[c]));
        }
    }
    double* out = a.part + ((size_t)r * a.maxleaves + leaf) * K + (STAGE == STAGE_COV ? ca * MAX_DIM : 0);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        if (STAGE < STAGE_MOM || k < 2 * (STAGE == STAGE_MOM) + ndim) {            // uniform
            const double tot = np_fold<STAGE == STAGE_MAX>(s[k], sm);
            if (threadIdx.x == 0) out[k] = tot;
        }
    }
}

// grid (R): the run's leaves summed (lane t takes the leaves t, t + 256, ... in order, then the fold), and what follows the sums
template <int STAGE>
__global__ __launch_bounds__(NP_BLOCK) void k_np_run(const NpArgs a)
{
    __shared__ double sm[4];
    __shared__ double res[MAX_DIM * MAX_DIM];
    constexpr int K = np_stage_k(STAGE);
    const int r = blockIdx.x, ndim = a.ndim, tid = threadIdx.x;
    const NpRun R = a.runs[r];
    double* st = a.stat + (size_t)r * NP_STAT;
    if (R.n == 0) {                                                    // no posterior
        if (STAGE == STAGE_MAX && tid < NP_STAT) st[tid] = tid == ST_ESS ? 0.0 : nan();
        if (STAGE == STAGE_MOM && tid < MAX_DIM) a.mean[r * MAX_DIM + tid] = nan();
        if (STAGE == STAGE_COV) a.cov[(size_t)r * MAX_DIM * MAX_DIM + tid] = nan();
        return;
    }
    const int64_t leaves = (R.n + LEAF - 1) / LEAF;
    const int nk = STAGE == STAGE_COV ? ndim * ndim : STAGE == STAGE_MOM ? 2 + ndim : K;
    for (int q = 0; q < nk; ++q) {
        const int k = STAGE == STAGE_COV ? (q / ndim) * MAX_DIM + q % ndim : q;
        double s = STAGE == STAGE_MAX ? neg_inf() : 0.0;
        for (int64_t l = tid; l < leaves; l += NP_BLOCK) {
            const double v = a.part[((size_t)r * a.maxleaves + l) * K + k];
            s = STAGE == STAGE_MAX ? (v > s ? v : s) : add(s, v);
        }
        const double tot = np_fold<STAGE == STAGE_MAX>(s, sm);
        if (tid == 0) res[k] = tot;
    }
    __syncthreads();
    if (STAGE == STAGE_MAX) {
        if (tid == 0) st[ST_M] = res[0];
    } else if (STAGE == STAGE_EXP) {
        if (tid == 0) { st[ST_S] = res[0]; st[ST_S2] = res[1]; st[ST_ESS] = kish_ess(res[0], res[1]); }
    } else if (STAGE == STAGE_MOM) {
        if (tid == 0) { st[ST_SP] = res[0]; st[ST_SP2] = res[1]; st[ST_FACT] = cov_factor(res[0], res[1]); }
        if (tid < ndim) a.mean[r * MAX_DIM + tid] = a.fixed[tid] ? a.theta[R.toff * ndim + tid] : div(res[2 + tid], res[0]);
    } else {
        const int ca = tid / MAX_DIM, cb = tid % MAX_DIM;
        if (ca < ndim && cb < ndim)
            a.cov[(size_t)r * MAX_DIM * MAX_DIM + tid] = (a.fixed[ca] || a.fixed[cb]) ? 0.0 : div(res[tid], st[ST_FACT]);
    }
}

// ---- the prefix: a wave takes 64 blocks of 64 points (one leaf) through LDS, lane l the block l in order ---------------------------
constexpr int NP_TILE_STRIDE = SCAN_BLOCK + 1;      // odd: lane l's row starts in its own bank

// the tile of leaf `leaf` of p, 0 beyond the run's points; returns the points of lane l's block
__device__ __forceinline__ int np_load_tile(const NpArgs& a, const NpRun& R, int64_t leaf, double* tile)
{
    const int lane = threadIdx.x;
    for (int j = 0; j < NP_WAVE; ++j) {
        const int64_t i = leaf * LEAF + j * SCAN_BLOCK + lane;
        tile[j * NP_TILE_STRIDE + lane] = i < R.n ? a.w[R.off + i] : 0.0;
    }
    __syncthreads();
    const int64_t left = R.n - (leaf * LEAF + (int64_t)lane * SCAN_BLOCK);
    return left <= 0 ? 0 : left < SCAN_BLOCK ? (int)left : SCAN_BLOCK;
}

// grid (maxleaves, R), 64 lanes: T_b of every block
__global__ __launch_bounds__(NP_WAVE) void k_np_scan_totals(const NpArgs a)
{
    __shared__ double tile[NP_WAVE * NP_TILE_STRIDE];
    const int r = blockIdx.y, lane = threadIdx.x;
    const NpRun R = a.runs[r];
    const int64_t leaf = blockIdx.x;
    if (leaf * LEAF >= R.n) return;
    const int cnt = np_load_tile(a, R, leaf, tile);
    if (cnt == 0) return;
    const double* row = tile + lane * NP_TILE_STRIDE;
    double run = row[0];
    for (int c = 1; c < cnt; ++c) run = add(run, row[c]);
    a.tot[(size_t)r * a.maxleaves * NP_WAVE + leaf * NP_WAVE + lane] = run;
}

// grid (R), 64 lanes: P_b = P_{b-1} + T_b in order of b, in place; the lanes move 64 totals at a time through LDS, lane 0 adds
__global__ __launch_bounds__(NP_WAVE) void k_np_scan_prefix(const NpArgs a)
{
    __shared__ double t[NP_WAVE];
    const int r = blockIdx.x, lane = threadIdx.x;
    const NpRun R = a.runs[r];
    const int64_t nblocks = (R.n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    double* tot = a.tot + (size_t)r * a.maxleaves * NP_WAVE;
    double before = 0.0;
    for (int64_t b0 = 0; b0 < nblocks; b0 += NP_WAVE) {               // uniform
        if (b0 + lane < nblocks) t[lane] = tot[b0 + lane];
        __syncthreads();
        if (lane == 0) {
            const int m = nblocks - b0 < NP_WAVE ? (int)(nblocks - b0) : NP_WAVE;
            for (int j = 0; j < m; ++j) {
                before = b0 + j == 0 ? t[j] : add(before, t[j]);
                t[j] = before;
            }
        }
        __syncthreads();
        if (b0 + lane < nblocks) tot[b0 + lane] = t[lane];
        __syncthreads();
    }
}

// grid (maxleaves, R), 64 lanes: C_i = P_{b-1} + L_i
__global__ __launch_bounds__(NP_WAVE) void k_np_scan_add(const NpArgs a)
{
    __shared__ double tile[NP_WAVE * NP_TILE_STRIDE];
    const int r = blockIdx.y, lane = threadIdx.x;
    const NpRun R = a.runs[r];
    const int64_t leaf = blockIdx.x;
    if (leaf * LEAF >= R.n) return;
    const int cnt = np_load_tile(a, R, leaf, tile);
    const int64_t b = leaf * NP_WAVE + lane;
    if (cnt > 0) {
        const double before = b > 0 ? a.tot[(size_t)r * a.maxleaves * NP_WAVE + b - 1] : 0.0;
        double* row = tile + lane * NP_TILE_STRIDE;
        double run = row[0];
        for (int c = 0; c < cnt; ++c) {
            if (c > 0) run = add(run, row[c]);
            row[c] = b == 0 ? run : add(before, run);
        }
    }
    __syncthreads();
    for (int j = 0; j < NP_WAVE; ++j) {
        const int64_t i = leaf * LEAF + j * SCAN_BLOCK + lane;
        if (i < R.n) a.C[R.off + i] = tile[j * NP_TILE_STRIDE + lane];
    }
}

// grid (ceil(N / 256), R): index [R][N], -1 for a run without a posterior
__global__ __launch_bounds__(NP_BLOCK) void k_np_resample(const NpArgs a, int64_t N, int64_t* __restrict__ index)
{
    const int r = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x;
    if (k >= N) return;
    const NpRun R = a.runs[r];
    int64_t idx = -1;
    if (R.n > 0) idx = resample_index(a.C + R.off, R.n, resample_t(k, resample_offset(a.seed, a.ids[r]), N));
    index[(int64_t)r * N + k] = idx;
}

// grid (ceil(N * width / 256), runs from run0 on): out [R][N][width], theta in the columns from `first` on (those before are left
// as they are); a row without a point is NaN in every column
__global__ __launch_bounds__(NP_BLOCK) void k_np_rows(const NpArgs a, int64_t N, const int64_t* __restrict__ index, int run0, int width,
                                                      int first, double* __restrict__ out)
{
    const int r = run0 + blockIdx.y, ndim = a.ndim;
    const int64_t e = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x;
    if (e >= N * width) return;
    const int64_t k = e / width;
    const int c = (int)(e - k * width);
    const int64_t idx = index[(int64_t)r * N + k];
    double* dst = out + ((int64_t)r * N) * width + e;
    if (idx < 0) *dst = nan();
    else if (c >= first) *dst = a.theta[(a.runs[r].toff + idx) * ndim + (c - first)];
}

}  // namespace

// ---- gf_weights.h: the launches ------------------------------------------------------------------------------------------------------
hipError_t gf_weights_launch(const GfWeightArgs& a, int R, bool moments, bool prefix, hipStream_t st)
{
    const dim3 leaves((unsigned)a.maxleaves, (unsigned)R), runs((unsigned)R);
    hipLaunchKernelGGL(k_np_leaf<STAGE_MAX>, leaves, dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_run<STAGE_MAX>, runs, dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_leaf<STAGE_EXP>, leaves, dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_run<STAGE_EXP>, runs, dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_leaf<STAGE_MOM>, leaves, dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_run<STAGE_MOM>, runs, dim3(NP_BLOCK), 0, st, a);
    if (moments) {
        hipLaunchKernelGGL(k_np_leaf<STAGE_COV>, dim3((unsigned)(a.maxleaves * a.ndim), (unsigned)R), dim3(NP_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_np_run<STAGE_COV>, runs, dim3(NP_BLOCK), 0, st, a);
    }
    if (prefix) {
        hipLaunchKernelGGL(k_np_scan_totals, leaves, dim3(NP_WAVE), 0, st, a);
        hipLaunchKernelGGL(k_np_scan_prefix, runs, dim3(NP_WAVE), 0, st, a);
        hipLaunchKernelGGL(k_np_scan_add, leaves, dim3(NP_WAVE), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t gf_weights_resample(const GfWeightArgs& a, int R, int64_t N, int64_t* d_index, hipStream_t st)
{
    const unsigned blocks = (unsigned)((N + NP_BLOCK - 1) / NP_BLOCK);
    hipLaunchKernelGGL(k_np_resample, dim3(blocks, (unsigned)R), dim3(NP_BLOCK), 0, st, a, N, d_index);
    return hipGetLastError();
}

hipError_t gf_weights_rows(const GfWeightArgs& a, int64_t N, const int64_t* d_index, int run0, int nruns, int width, int first, double* d_out,
                           hipStream_t st)
{
    const unsigned blocks = (unsigned)((N * width + NP_BLOCK - 1) / NP_BLOCK);
    hipLaunchKernelGGL(k_np_rows, dim3(blocks, (unsigned)nruns), dim3(NP_BLOCK), 0, st, a, N, d_index, run0, width, first, d_out);
    return hipGetLastError();
}
