// gf_nested_post.hip -- the posterior of every run of a nested sampler (gf_nested.hip), computed where the runs' points lie: MultiNest,
// which the sampler stands in for (golemflavor/mn.py:89-101), writes its weighted samples, post_equal_weights and stats beside the
// evidence.  The arithmetic and the order of every sum are gf_nested_post.hpp's; here are the launches.  All runs go
// through one set of them, blockIdx.y = run; a run without a posterior (not finished, failed, ln Z = -inf) has no points.
//   k_np_gather        the iteration-major dead points and the live set -> per-run compact lnw [n] and full-width theta [n][ndim]
//   k_np_leaf<STAGE>   one workgroup per leaf of 4096 points (STAGE_COV: per leaf and column): max lnw | e = exp(lnw - m), sums of e
//                      and e^2 | p = e / S, sums of p, p^2, p theta | sums of p (theta_a - mean_a)(theta_b - mean_b)
//   k_np_run<STAGE>    one workgroup per run: the leaves of the run summed, and what follows the sums
//   k_np_scan_totals, k_np_scan_prefix, k_np_scan_add      the inclusive prefix C of p: block totals, their prefix, the sum of both --
//                      three launches, no workgroup waits for another
//   k_np_resample      one lane per output row: the binary search of t_k in the run's C
//   k_np_rows          the rows, consecutive lanes on consecutive columns
// Only k_np_gather reads the sampler's view; the others take a GfWeightArgs (gf_weights.h) and are launched through gf_weights_launch,
// gf_weights_resample and gf_weights_rows, here and from gf_reweight.hip (a stored chain's targets as runs that share one theta).
// The equal-weight rows [nruns][nrows][width] then go through the reductions the MCMC chains go through (gf_marginal.hip,
// gf_elements.hip, gf_region.hip) with nchains = nruns.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"                    // (after gf_devcache.h: GfScratch allocates through the cache)
#include "gf_elements.h"
#include "gf_interval.h"
#include "gf_marginal.h"
#include "gf_nested_post.hpp"
#include "gf_region.h"
#include "gf_spectrum.h"
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

// what the kernels see (gf_weights.h): only k_np_gather reads the sampler's view
using NpRun = GfWeightRun;
using NpArgs = GfWeightArgs;
static_assert(np_stage_k(STAGE_COV) == GF_WEIGHT_PART_COV && np_stage_k(STAGE_MOM) == GF_WEIGHT_PART, "gf_weights.h states the stages' sizes");

__global__ __launch_bounds__(NP_BLOCK) void k_np_gather(const NpArgs a, const GfNestedView v, double* __restrict__ lnw, double* __restrict__ theta)
{
    const int r = blockIdx.y, ndim = v.ndim, D = v.nscan, B = v.batch, K = v.nlive;
    const NpRun R = a.runs[r];
    const int64_t e = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x;
    if (e >= R.n * ndim) return;
    const int64_t i = e / ndim;
    const int c = (int)(e - i * ndim);
    int64_t src;                                  // the point's place in the dead or in the live arrays
    const bool dead = i < R.nd;
    if (dead) { const int64_t it = i / B; src = (it * v.nruns + r) * B + (i - it * B); }
    else src = (int64_t)r * K + (i - R.nd);
    const int sl = v.slot[c];
    double x;
    if (sl >= 0) {
        const double u = (dead ? v.d_dead_u : v.d_live_u)[src * D + sl];
        x = cube_theta(v.d_commons[r].lo[c], v.d_commons[r].hi[c], u);
    } else {
        x = v.d_bases[r * MAX_DIM + c];
    }
    theta[(R.toff + i) * ndim + c] = x;
    if (c == 0) lnw[R.off + i] = dead ? v.d_dead_w[src] : live_lnw(R.lnw0, v.d_live_l[src]);
}

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

// ---- gf_weights.h: the launches, for this file's runs and for gf_reweight.hip's ---------------------------------------------------
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

namespace {
// ---- host --------------------------------------------------------------------------------------------------------------------------
struct NpWork {
    GfScratch buf;
    NpArgs a = {};
    GfNestedView v = {};
    std::vector<GfNestedRunState> state;
    std::vector<NpRun> runs;
    int64_t total = 0, maxn = 0;
};

int np_alloc_fail(const char* who, size_t bytes)
{
    return gf_fail_msg(GF_ERR_ALLOC, "%s: %zu bytes of device scratch were not granted", who, bytes);
}

template <typename T>
bool np_get(NpWork& w, T** p, size_t bytes, size_t* failed)
{
    if (w.buf.get(p, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    *failed = bytes;
    return false;
}

// gather, weights and (moments) mean and covariance, (prefix) C.  Everything is enqueued on the sampler's stream; no sync at the end.
int np_prepare(gf_nested* s, NpWork& w, bool moments, bool prefix, const char* who)
{
    NpArgs& a = w.a;
    GfNestedView& v = w.v;
    int rc = gf_internal_nested_view(s, &v, nullptr);
    if (rc != GF_OK) return rc;
    const int R = v.nruns;
    w.state.resize(R);
    w.runs.resize(R);
    rc = gf_internal_nested_view(s, &v, w.state.data());
    if (rc != GF_OK) return rc;
    for (int r = 0; r < R; ++r) {
        const GfNestedRunState& x = w.state[r];
        NpRun& q = w.runs[r];
        const bool ok = x.done && !x.failed && x.lnz > -HUGE_VAL;
        q.off = q.toff = w.total;
        q.nd = ok ? x.iter * v.batch : 0;
        q.n = ok ? q.nd + v.nlive : 0;
        q.lnw0 = x.lnx - std::log((double)v.nlive);          // gf_nested_get_dead's expression
        w.total += q.n;
        w.maxn = std::max(w.maxn, q.n);
    }
    a.ndim = v.ndim;
    for (int c = 0; c < MAX_DIM; ++c) a.fixed[c] = v.slot[c] < 0;
    a.seed = v.seed;
    a.ids = v.d_run_ids;
    a.maxleaves = std::max<int64_t>(1, (w.maxn + LEAF - 1) / LEAF);
    if (a.maxleaves * std::max(1, v.ndim) > 0x7fffffffll) return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: too many points per run", who);
    const size_t T = (size_t)w.total, K = moments ? MAX_DIM * MAX_DIM : 2 + MAX_DIM;
    NpRun* d_runs = nullptr;
    double *d_lnw = nullptr, *d_theta = nullptr;
    size_t bad = 0;
    const bool got = np_get(w, &d_runs, sizeof(NpRun) * R, &bad) && np_get(w, &d_lnw, sizeof(double) * T, &bad) &&
                     np_get(w, &d_theta, sizeof(double) * T * v.ndim, &bad) && np_get(w, &a.w, sizeof(double) * T, &bad) &&
                     np_get(w, &a.part, sizeof(double) * R * a.maxleaves * K, &bad) && np_get(w, &a.stat, sizeof(double) * R * NP_STAT, &bad) &&
                     np_get(w, &a.mean, sizeof(double) * R * MAX_DIM, &bad) && np_get(w, &a.cov, sizeof(double) * R * MAX_DIM * MAX_DIM, &bad) &&
                     (!prefix || (np_get(w, &a.C, sizeof(double) * T, &bad) && np_get(w, &a.tot, sizeof(double) * R * a.maxleaves * NP_WAVE, &bad)));
    if (!got) return np_alloc_fail(who, bad);
    a.runs = d_runs;
    a.lnw = d_lnw;
    a.theta = d_theta;
    hipStream_t st = v.stream;
    GF_HIP(hipMemcpyAsync(d_runs, w.runs.data(), sizeof(NpRun) * R, hipMemcpyHostToDevice, st));
    const unsigned gblocks = (unsigned)std::max<int64_t>(1, (w.maxn * v.ndim + NP_BLOCK - 1) / NP_BLOCK);
    hipLaunchKernelGGL(k_np_gather, dim3(gblocks, (unsigned)R), dim3(NP_BLOCK), 0, st, a, v, d_lnw, d_theta);
    GF_HIP(gf_weights_launch(a, R, moments, prefix, st));
    return GF_OK;
}

hipError_t np_launch_rows(const NpWork& w, int64_t N, const int64_t* d_index, int run0, int nruns, int width, int first, double* d_out)
{
    return gf_weights_rows(w.a, N, d_index, run0, nruns, width, first, d_out, w.v.stream);
}

// Every run's N theta rows into d_theta [R][N][ndim] (d_index [R][N] filled), then run r's slice propagated with its model into
// d_fr [.][3] and d_st (per_run: [R][N] each, else one run's, reused) followed by after(r, theta_r, fr_r, st_r); a run without a
// posterior is not propagated: after_none(r).  Enqueued on the sampler's stream, which is synchronised at the end.
template <class After, class AfterNone>
int np_propagated(gf_nested* s, NpWork& w, int64_t N, int64_t* d_index, double* d_theta, double* d_fr, int32_t* d_st, bool per_run, const char* who,
                  After after, AfterNone after_none)
{
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    hipError_t e = gf_weights_resample(w.a, v.nruns, N, d_index, st);
    if (e == hipSuccess) e = np_launch_rows(w, N, d_index, 0, v.nruns, v.ndim, 0, d_theta);
    int rc = GF_OK;
    gf_internal_full_arbitration_grids(v.device, st, 1);              // the runs of a scan differ (gf_postprocess.hip for_each_chain)
    for (int r = 0; r < v.nruns && rc == GF_OK && e == hipSuccess; ++r) {
        const size_t at = per_run ? (size_t)r * N : 0;
        double* th = d_theta + (size_t)r * N * v.ndim;
        if (w.runs[r].n == 0) { e = after_none(r); continue; }
        rc = gf_model_propagate_on(v.models[r], st, th, GF_LAYOUT_AOS, N, d_fr + at * 3, d_st + at);
        if (rc == GF_OK) e = after(r, th, d_fr + at * 3, d_st + at);
    }
    gf_internal_full_arbitration_grids(v.device, st, 0);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, who);
    return gf_internal_check_overflow(v.device, st);
}

// the equal-weight rows of every run into d_rows [R][N][(with_fr ? 3 : 0) + ndim], d_index [R][N] (NULL: scratch); synchronous
int np_rows(gf_nested* s, int64_t N, int with_fr, double* d_rows, int64_t* d_index, const char* who)
{
    if (!s || N < 1 || !d_rows) return GF_ERR_INVALID_ARG;
    NpWork w;
    int rc = np_prepare(s, w, false, true, who);
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    const size_t RN = (size_t)v.nruns * N;
    size_t bad = 0;
    if (!d_index && !np_get(w, &d_index, sizeof(int64_t) * RN, &bad)) return np_alloc_fail(who, bad);
    if (!with_fr) {
        hipError_t e = gf_weights_resample(w.a, v.nruns, N, d_index, st);
        if (e == hipSuccess) e = np_launch_rows(w, N, d_index, 0, v.nruns, v.ndim, 0, d_rows);
        const hipError_t e2 = hipStreamSynchronize(st);
        if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, who);
        return GF_OK;
    }
    double *d_theta = nullptr, *d_fr = nullptr;
    int32_t* d_st = nullptr;
    if (!np_get(w, &d_theta, sizeof(double) * RN * v.ndim, &bad) || !np_get(w, &d_fr, sizeof(double) * RN * 3, &bad) ||
        !np_get(w, &d_st, sizeof(int32_t) * RN, &bad))
        return np_alloc_fail(who, bad);
    const int width = 3 + v.ndim;
    return np_propagated(s, w, N, d_index, d_theta, d_fr, d_st, true, who,
                         [&](int r, const double* th, const double* fr, const int32_t* stt) {
                             return gf_launch_join_rows(fr, stt, th, v.ndim, N, d_rows + (size_t)r * N * width, v.cus, st);
                         },
                         [&](int r) { return np_launch_rows(w, N, d_index, r, 1, width, 3, d_rows); });
}

}  // namespace

extern "C" {

int gf_nested_posterior(gf_nested* s, int64_t* npoints, double* ess, double* lnz_check, double* mean, double* cov)
{
    if (!s) return GF_ERR_INVALID_ARG;
    NpWork w;
    const int rc = np_prepare(s, w, true, false, "gf_nested_posterior");
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    const int R = v.nruns, nd = v.ndim;
    std::vector<double> h_stat((size_t)R * NP_STAT), h_mean((size_t)R * MAX_DIM), h_cov((size_t)R * MAX_DIM * MAX_DIM);
    hipError_t e = hipMemcpyAsync(h_stat.data(), w.a.stat, sizeof(double) * h_stat.size(), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_mean.data(), w.a.mean, sizeof(double) * h_mean.size(), hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_cov.data(), w.a.cov, sizeof(double) * h_cov.size(), hipMemcpyDeviceToHost, v.stream);
    const hipError_t e2 = hipStreamSynchronize(v.stream);
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, "gf_nested_posterior");
    for (int r = 0; r < R; ++r) {
        const double* q = h_stat.data() + (size_t)r * NP_STAT;
        if (npoints) npoints[r] = w.runs[r].n;
        if (ess) ess[r] = q[ST_ESS];
        if (lnz_check) lnz_check[r] = w.runs[r].n ? q[ST_M] + std::log(q[ST_S]) : gfnp::nan();      // the host's log: a diagnostic
        for (int a = 0; a < nd; ++a) {
            if (mean) mean[(size_t)r * nd + a] = h_mean[(size_t)r * MAX_DIM + a];
            for (int b = 0; b < nd && cov; ++b) cov[((size_t)r * nd + a) * nd + b] = h_cov[((size_t)r * MAX_DIM + a) * MAX_DIM + b];
        }
    }
    return GF_OK;
}

int gf_nested_posterior_rows_device(gf_nested* s, int64_t nrows, int with_fr, double* d_rows)
{
    return np_rows(s, nrows, with_fr, d_rows, nullptr, "gf_nested_posterior_rows_device");
}

int gf_nested_posterior_rows(gf_nested* s, int64_t nrows, int with_fr, double* rows, int64_t* index)
{
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1 || !rows) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(v.device));
    const size_t RN = (size_t)v.nruns * nrows, width = (with_fr ? 3 : 0) + (size_t)v.ndim;
    GfScratch buf;
    double* d_rows = nullptr;
    int64_t* d_index = nullptr;
    if (buf.get(&d_rows, sizeof(double) * RN * width) != hipSuccess) return np_alloc_fail("gf_nested_posterior_rows", sizeof(double) * RN * width);
    if (buf.get(&d_index, sizeof(int64_t) * RN) != hipSuccess) return np_alloc_fail("gf_nested_posterior_rows", sizeof(int64_t) * RN);
    int rc = np_rows(s, nrows, with_fr, d_rows, d_index, "gf_nested_posterior_rows");
    if (rc == GF_OK) rc = gf_internal_d2h(v.device, v.stream, rows, d_rows, sizeof(double) * RN * width);
    if (rc == GF_OK && index) {
        GF_HIP(hipMemcpyAsync(index, d_index, sizeof(int64_t) * RN, hipMemcpyDeviceToHost, v.stream));
        GF_HIP(hipStreamSynchronize(v.stream));
    }
    return rc;
}

int gf_nested_marginals(gf_nested* s, int64_t nrows, int with_fr, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1 || !out) return GF_ERR_INVALID_ARG;
    const int width = (with_fr ? 3 : 0) + v.ndim;
    int rc = gf_marginal_check_args(v.nruns, nrows, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    GfScratch buf;
    double* d_rows = nullptr;
    const size_t bytes = sizeof(double) * (size_t)v.nruns * nrows * width;
    if (buf.get(&d_rows, bytes) != hipSuccess) return np_alloc_fail("gf_nested_marginals", bytes);
    rc = np_rows(s, nrows, with_fr, d_rows, nullptr, "gf_nested_marginals");
    return rc != GF_OK ? rc : gf_marginal_run(v.stream, d_rows, nrows * width, v.nruns, nrows, width, spec, out);
}

// the column intervals (gf_interval.hip, nchains = nruns) of gf_nested_posterior_rows_device's rows, which stay on the device
int gf_nested_intervals(gf_nested* s, int64_t nrows, int with_fr, const gf_interval_spec* spec, const gf_interval_out* out)
{
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1 || !spec || !out) return GF_ERR_INVALID_ARG;
    const int width = (with_fr ? 3 : 0) + v.ndim;
    int rc = gf_interval_check_args(v.nruns, nrows, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    GfScratch buf;
    double* d_rows = nullptr;
    const size_t bytes = sizeof(double) * (size_t)v.nruns * nrows * width;
    if (buf.get(&d_rows, bytes) != hipSuccess) return np_alloc_fail("gf_nested_intervals", bytes);
    rc = np_rows(s, nrows, with_fr, d_rows, nullptr, "gf_nested_intervals");
    return rc != GF_OK ? rc : gf_interval_run(v.stream, d_rows, nrows * width, v.nruns, nrows, width, spec, out, nullptr);
}

// the energy-resolved composition (gf_spectrum.hip) of every run's equal-weight rows, run after run through one bin-major slab; a run
// without a posterior is not evaluated: nvalid 0, NaN moments and order statistics, rank -1, empty histograms
int gf_nested_spectrum(gf_nested* s, int64_t nrows, const gf_spectrum_spec* spec, const gf_spectrum_out* out)
{
    GfNestedView v0;
    if (gf_internal_nested_view(s, &v0, nullptr) != GF_OK || nrows < 1) return GF_ERR_INVALID_ARG;
    int nbins_e = -1;
    for (int r = 0; r < v0.nruns; ++r) {
        const int nb = gf_model_nbins(v0.models[r]);
        if (nb < 1) return GF_ERR_UNSUPPORTED;
        if (nbins_e >= 0 && nb != nbins_e) return gf_fail_msg(GF_ERR_INVALID_ARG, "spectrum: run %d has %d energy bins, run 0 has %d", r, nb, nbins_e);
        nbins_e = nb;
    }
    int rc = gf_spectrum_check_args(nbins_e, nrows, spec, out);
    if (rc != GF_OK) return rc;
    NpWork w;
    rc = np_prepare(s, w, false, true, "gf_nested_spectrum");
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    const size_t RN = (size_t)v.nruns * nrows;
    int64_t* d_index = nullptr; double *d_theta = nullptr, *d_slab = nullptr; int32_t* d_st = nullptr;
    size_t bad = 0;
    if (!np_get(w, &d_index, sizeof(int64_t) * RN, &bad) || !np_get(w, &d_theta, sizeof(double) * RN * v.ndim, &bad) ||
        !np_get(w, &d_slab, sizeof(double) * 3 * (size_t)nrows * nbins_e, &bad) || !np_get(w, &d_st, sizeof(int32_t) * (size_t)nrows, &bad))
        return np_alloc_fail("gf_nested_spectrum", bad);
    const int nb1 = spec->nbins1, R2 = 2 * spec->nq;
    int rs = GF_OK;
    rc = np_propagated(s, w, nrows, d_index, d_theta, d_slab, d_st, false, "gf_nested_spectrum",
                       [&](int r, const double* th, const double*, const int32_t*) {
                           rs = gf_model_bins_on(v.models[r], st, th, GF_LAYOUT_AOS, nrows, d_slab, 1, d_st);
                           if (rs == GF_OK) rs = gf_spectrum_reduce(st, d_slab, nbins_e, nrows, spec, out, r);
                           return rs == GF_OK ? hipSuccess : hipErrorUnknown;
                       },
                       [&](int r) {
                           const size_t at = (size_t)r * nbins_e;
                           for (size_t i = 0; i < (size_t)nbins_e; ++i) {
                               if (out->nvalid) out->nvalid[at + i] = 0;
                               for (int j = 0; j < 3 && out->mean; ++j) out->mean[(at + i) * 3 + j] = gfnp::nan();
                               for (int j = 0; j < 9 && out->cov; ++j) out->cov[(at + i) * 9 + j] = gfnp::nan();
                               for (int j = 0; j < 3 * R2 && out->ostat; ++j) out->ostat[(at + i) * 3 * R2 + j] = gfnp::nan();
                               for (int j = 0; j < 3 * R2 && out->orank; ++j) out->orank[(at + i) * 3 * R2 + j] = -1;
                               for (int j = 0; j < 3 * nb1 && out->counts; ++j) out->counts[(at + i) * 3 * nb1 + j] = 0;
                           }
                           return hipSuccess;
                       });
    return rs != GF_OK ? rs : rc;
}

int gf_nested_element_marginals(gf_nested* s, int64_t nrows, const gf_element_plan* plan, const gf_marginal_spec* spec, const gf_marginal_out* out)
{
    GfNestedView v;
    if (gf_internal_nested_view(s, &v, nullptr) != GF_OK || nrows < 1 || !out) return GF_ERR_INVALID_ARG;
    const int width = gf_element_plan_width(plan, v.ndim);
    if (width < 0) return GF_ERR_INVALID_ARG;
    int rc = gf_marginal_check_args(v.nruns, nrows, width, spec);
    if (rc != GF_OK) return rc;
    GF_HIP(hipSetDevice(v.device));
    GfScratch buf;
    double *d_theta = nullptr, *d_rows = nullptr;
    const size_t RN = (size_t)v.nruns * nrows;
    if (buf.get(&d_theta, sizeof(double) * RN * v.ndim) != hipSuccess) return np_alloc_fail("gf_nested_element_marginals", sizeof(double) * RN * v.ndim);
    if (buf.get(&d_rows, sizeof(double) * RN * width) != hipSuccess) return np_alloc_fail("gf_nested_element_marginals", sizeof(double) * RN * width);
    rc = np_rows(s, nrows, 0, d_theta, nullptr, "gf_nested_element_marginals");
    if (rc != GF_OK) return rc;
    const hipError_t e = gf_element_run(v.stream, d_theta, nrows * v.ndim, v.nruns, nrows, v.ndim, plan, d_rows, nrows * width, v.cus);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_nested_element_marginals");
    return gf_marginal_run(v.stream, d_rows, nrows * width, v.nruns, nrows, width, spec, out);
}

int gf_nested_regions(gf_nested* s, int64_t nrows, int nbins, int radius, const double* weights, const double* coverage, int ncov, int64_t cap,
                      int64_t* thres, int32_t* saturated, double* level_in, double* level_out, double* mass, int32_t* cells, double* density)
{
    if (!s || nrows < 1) return GF_ERR_INVALID_ARG;
    const char* who = "gf_nested_regions";
    NpWork w;
    {
        GfNestedView v;
        if (gf_internal_nested_view(s, &v, nullptr) != GF_OK) return GF_ERR_INVALID_ARG;
        const int rc = gf_region_check_args(v.nruns, nbins, radius, weights, coverage, ncov, cap);
        if (rc != GF_OK) return rc;
        GF_HIP(hipSetDevice(v.device));
    }
    int rc = np_prepare(s, w, false, true, who);
    if (rc != GF_OK) return rc;
    const GfNestedView& v = w.v;
    hipStream_t st = v.stream;
    const size_t RN = (size_t)v.nruns * nrows, nbin3 = (size_t)nbins * nbins * nbins;
    int64_t* d_index = nullptr;
    double *d_theta = nullptr, *d_fr = nullptr;
    int32_t* d_st = nullptr;
    uint64_t* d_c = nullptr;
    size_t bad = 0;
    if (!np_get(w, &d_index, sizeof(int64_t) * RN, &bad) || !np_get(w, &d_theta, sizeof(double) * RN * v.ndim, &bad) ||
        !np_get(w, &d_fr, sizeof(double) * nrows * 3, &bad) || !np_get(w, &d_st, sizeof(int32_t) * nrows, &bad) ||
        !np_get(w, &d_c, sizeof(uint64_t) * nbin3 * v.nruns, &bad))
        return np_alloc_fail(who, bad);
    GF_HIP(hipMemsetAsync(d_c, 0, sizeof(uint64_t) * nbin3 * v.nruns, st));
    rc = np_propagated(s, w, nrows, d_index, d_theta, d_fr, d_st, false, who,
                       [&](int r, const double*, double* fr, const int32_t* stt) {
                           const hipError_t ea = gf_launch_mask_fr(fr, stt, nrows, st);
                           return ea != hipSuccess ? ea : gf_launch_flavor_hist(fr, nrows, nbins, (unsigned long long*)(d_c + (size_t)r * nbin3), v.cus, st);
                       },
                       [](int) { return hipSuccess; });
    if (rc != GF_OK) return rc;
    return gf_region_run(st, d_c, v.nruns, nbins, radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass, cells, density,
                         nullptr);
}

}  // extern "C"
