// gf_nested.hip -- device-resident nested sampler: the evidence of golemflavor/mn.py (MultiNest at every new-physics scale of
// scripts/sens.py) with the constrained-replacement walks run as device walkers.
//
// Every run r (one posterior, one gf_model) keeps K live points in the unit cube of its scanned columns; the prior is uniform
// on that cube (mn.py:22-23 CubePrior is a no-op) and the log-likelihood is the full ln_prob of theta(u), theta_i = (hi_i - lo_i)
// u_i + lo_i on the scanned columns (mn.py:35-36), the paramset's value elsewhere.  One iteration of a run:
//   k_ns_select  (one workgroup per run)  sorts the live lnL in LDS, removes the b lowest -- the j-th removed point sees
//                K - j live points: ln X_{i+1} = ln X_i - 1/(K - j), weight L_i (X_i - X_{i+1}) (dynamic nested sampling,
//                Higson et al. 2019) -- appends them to the dead points, updates ln Z, H and max lnL, sets L* = the highest
//                removed lnL, forms the survivors' covariance and its Cholesky factor C (fp64), and draws each replacement's
//                start among the survivors above L*.  It also applies the termination rule ln(Z + L_max X) - ln Z < tol and
//                then adds the live set's X mean(L_live).
//                Where the likelihood is zero (lnL = -inf) the live points tie on a plateau; replacements never land on it, so
//                its points are removed without replacement across iterations: the i-th -inf point of the run (they all come
//                first) sees K - i live points (Fowlie, Handley & Su 2021), and their compression variance sum 1/(K - i)^2
//                is added to the error of ln Z.
//   k_ns_walk    (x walks) one Metropolis step of every replacement walker of every live run: u' = u + s C z, z ~ N(0, I); a
//                step outside the cube is rejected unevaluated, otherwise it is accepted iff lnq > L*.  Proposals whose
//                unitarity verdict the in-kernel tiers cannot settle are parked and settled by the emulated-x87 team
//                (k_stretch_settle<Team9, true>, gf_unitarity.hip) before the next step.
//   k_ns_commit  (one workgroup per run) writes the replacements into the freed slots and adapts s towards an acceptance
//                of 0.5.
// Random numbers: Philox4x32-10, key = seed, counter = (global run id, iteration, replacement slot, step): a run's result does
// not depend on the other runs of the launch or on the launch shape.  The host loop reads the per-run done flags back every
// few iterations; it is not captured into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <new>
#include <vector>

#include "../../include/golemflavor_hip.h"
#include "gf_consts.h"

extern "C" const char* gf_internal_env(const char* name, int affects_results);   // gf_capi.hip: getenv with a record
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_launch.h"
#include "gf_propose.hpp"

namespace {
using namespace gfdev;

constexpr int NS_MAX_LIVE = 4096;       // live points per run: k_ns_select sorts them in LDS
constexpr int NS_SEL_BLOCK = 1024;
constexpr uint32_t NS_INIT_ITER = 0xFFFFFFFFu;      // iteration word of the initial draws
constexpr uint32_t NS_START_STEP = 0xFFFFFFFFu;     // step word of a replacement's start pick

struct NsRun {
    double lnx, lnz, h, lmax, scale;
    double pvar;            // compression variance of the plateau removals, sum 1/n^2
    int64_t nplat;          // plateau (lnL = -inf) points removed so far
    int64_t iter;           // completed removal iterations
    int64_t nevals;         // likelihood evaluations
    int32_t done, failed;   // failed: on_nonunitary == raise and a proposal the reference would have raised on
};

struct NsArgs {
    const GfCommon* commons;        // [R]
    const GfBsm* const* tbs;        // [R]
    const double* const* ptabs;     // [R]
    const uint64_t* run_ids;        // [R] Philox counter word 0
    const double* bases;            // [R][GF_MAX_DIM] values of the columns that are not scanned
    NsRun* runs;                    // [R]
    double* lstar;                  // [R]
    uint32_t* nonunit;              // [R]
    double* live_u;                 // [R][K][D]
    double* live_l;                 // [R][K]
    double* chol;                   // [R][D][D] lower
    int32_t* freed;                 // [R][B]
    double* wu;                     // [R][B][D]
    double* wl;                     // [R][B]
    uint32_t* wacc;                 // [R][B]
    uint32_t* wev;                  // [R][B]
    double* prop_u;                 // [R][B][D] parked proposals
    GfArbQueue* pq;                 // capacity R * B
    double* pend_rows;              // [R * B][GF_PEND_STRIDE]
    double* dead_l;                 // [cap][R][B] (iteration-major: growing the buffer is one copy)
    double* dead_w;                 // [cap][R][B] log-weights
    double* dead_u;                 // [cap][R][B][D]
    double* theta;                  // [R][K][ndim] initial points (k_ns_init)
    int32_t* status;                // [R][K]
    uint64_t seed;
    double tol;
    int32_t nruns, nlive, batch, nscan, ndim, walks, raise, step;
    int32_t slot[GF_MAX_DIM];       // column -> scanned slot, -1 = fixed
    int32_t nbins_max;
};

__device__ __forceinline__ void ns_uniform2(const NsArgs& a, int r, uint32_t it, uint32_t slot, uint32_t step, double out[2])
{
    uint32_t q[4];
    const uint64_t key = a.seed, id = a.run_ids[r];
    philox_block((uint32_t)id, it, slot, step, (uint32_t)key, (uint32_t)(key >> 32) ^ (uint32_t)(id >> 32), q);
    out[0] = ((double)(q[0] >> 5) * 67108864.0 + (double)(q[1] >> 6)) * (1.0 / 9007199254740992.0);
    out[1] = ((double)(q[2] >> 5) * 67108864.0 + (double)(q[3] >> 6)) * (1.0 / 9007199254740992.0);
}

// theta of cube point u for run r: mn.py:35-39, the product and the sum each rounded (as k_cube_to_theta)
__device__ __forceinline__ void ns_cube_to_theta(const NsArgs& a, const GfCommon& c, int r, const double* u, double* row)
{
    for (int d = 0; d < a.ndim; ++d) {
        const int sl = a.slot[d];
        row[d] = sl >= 0 ? __dadd_rn(__dmul_rn(c.hi[d] - c.lo[d], u[sl]), c.lo[d]) : a.bases[r * GF_MAX_DIM + d];
    }
}

// K cube points per run, drawn uniformly (counter (run id, NS_INIT_ITER, point, pair of coordinates)) and mapped to theta;
// the bulk lnprob path evaluates them next, with its own unitarity arbitration
__global__ __launch_bounds__(GF_BLOCK) void k_ns_init(const NsArgs a)
{
    const int r = blockIdx.y;
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    if (i >= a.nlive) return;
    double u[GF_MAX_DIM];
    for (int p = 0; 2 * p < a.nscan; ++p) {
        double v[2];
        ns_uniform2(a, r, NS_INIT_ITER, (uint32_t)i, (uint32_t)p, v);
        u[2 * p] = v[0];
        if (2 * p + 1 < a.nscan) u[2 * p + 1] = v[1];
    }
    double* lu = a.live_u + ((int64_t)r * a.nlive + i) * a.nscan;
    for (int d = 0; d < a.nscan; ++d) lu[d] = u[d];
    ns_cube_to_theta(a, a.commons[r], r, u, a.theta + ((int64_t)r * a.nlive + i) * a.ndim);
}

// after the bulk evaluation: a point the reference would have raised on is outside the support (-inf) and counted; NaN too
__global__ __launch_bounds__(GF_BLOCK) void k_ns_init_fix(const NsArgs a)
{
    const int r = blockIdx.y;
    const int i = blockIdx.x * GF_BLOCK + threadIdx.x;
    if (i >= a.nlive) return;
    const int64_t j = (int64_t)r * a.nlive + i;
    const double l = a.live_l[j];
    if (a.status[j] == ST_NON_UNITARY) { a.live_l[j] = -gf_inf(); atomicAdd(&a.nonunit[r], 1u); }
    else if (l != l) a.live_l[j] = -gf_inf();
}

__device__ __forceinline__ bool ns_less(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// ln(exp(x) + exp(y)) with -inf handled
__device__ __forceinline__ double ns_logaddexp(double x, double y)
{
    if (x == -gf_inf()) return y;
    if (y == -gf_inf()) return x;
    const double m = x > y ? x : y;
    return m + log1p(exp(-fabs(x - y)));
}

// Z += exp(lnw), with H (the information) updated as in Skilling 2006: H' = (w L) / Z' + Z / Z' (H + ln Z) - ln Z'
__device__ __forceinline__ void ns_accumulate(NsRun& R, double lnl, double lnw)
{
    if (lnw == -gf_inf()) return;
    const double lnz_new = ns_logaddexp(R.lnz, lnw);
    if (R.lnz == -gf_inf()) R.h = exp(lnw - lnz_new) * lnl - lnz_new;
    else R.h = exp(lnw - lnz_new) * lnl + exp(R.lnz - lnz_new) * (R.h + R.lnz) - lnz_new;
    R.lnz = lnz_new;
}

__global__ __launch_bounds__(NS_SEL_BLOCK) void k_ns_select(const NsArgs a)
{
    __shared__ double key[NS_MAX_LIVE];
    __shared__ int idx[NS_MAX_LIVE];
    __shared__ double mean[GF_MAX_DIM];
    __shared__ double cov[GF_MAX_DIM * GF_MAX_DIM];
    __shared__ double part[NS_SEL_BLOCK];
    __shared__ int skip, first;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int K = a.nlive, B = a.batch, D = a.nscan;
    NsRun* run = a.runs + r;
    if (tid == 0) {
        int s = run->done;
        if (!s && a.raise && a.nonunit[r] != 0u) { run->failed = 1; run->done = 1; s = 1; }     // sens.py:283-285 re-raises
        skip = s;
    }
    __syncthreads();
    if (skip) return;
    const double* ll = a.live_l + (int64_t)r * K;
    const double* lu = a.live_u + (int64_t)r * K * D;
    for (int i = tid; i < NS_MAX_LIVE; i += NS_SEL_BLOCK) {
        double v = i < K ? ll[i] : gf_inf();
        if (v != v) v = -gf_inf();
        key[i] = v; idx[i] = i;
    }
    __syncthreads();
    // bitonic sort by (lnL, slot): a total order, so the result does not depend on the thread schedule
    for (int k = 2; k <= NS_MAX_LIVE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < NS_MAX_LIVE; i += NS_SEL_BLOCK) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const bool gt = ns_less(key[l], idx[l], key[i], idx[i]);
                    if (gt == up) {
                        const double tk = key[i]; key[i] = key[l]; key[l] = tk;
                        const int ti = idx[i]; idx[i] = idx[l]; idx[l] = ti;
                    }
                }
            }
            __syncthreads();
        }
    const int64_t it = run->iter;
    if (tid == 0) {
        NsRun R = *run;
        const double lmax_live = key[K - 1];
        if (lmax_live > R.lmax) R.lmax = lmax_live;
        // MultiNest's evidence tolerance: what the live set could still add is below tol.  A live set without one point of
        // non-zero likelihood (the Gaussian likelihood underflows to -inf far from the measured composition, llh.py:32-54)
        // can add nothing either: the run ends, with ln Z = -inf if no point ever had a finite lnL.
        const bool stop = lmax_live == -gf_inf() ||
                          (R.lnz != -gf_inf() && ns_logaddexp(R.lnz, lmax_live + R.lnx) - R.lnz < a.tol);
        if (stop) {
            // X_i mean(L_live): every live point with weight X_i / K, in ascending lnL
            const double lnw0 = R.lnx - log((double)K);
            for (int m = 0; m < K; ++m) ns_accumulate(R, key[m], key[m] + lnw0);
            R.done = 1;
        } else {
            double* dl = a.dead_l + (it * a.nruns + r) * B;
            double* dw = a.dead_w + (it * a.nruns + r) * B;
            for (int j = 0; j < B; ++j) {
                // a plateau point sees the K - i live points left of the i-th removal: fewer than K - j from the second batch
                // on (no replacement lands on the plateau, so it never gains a point back); K - i >= 1 since a live set
                // of K plateau points stops the run
                const bool plat = key[j] == -gf_inf();
                const double dx = 1.0 / (double)(plat ? K - R.nplat : K - j);
                const double lnw = key[j] + R.lnx + log(-expm1(-dx));     // ln(X_i - X_{i+1}) = ln X_i + ln(1 - e^{-1/n})
                ns_accumulate(R, key[j], lnw);
                dl[j] = key[j];
                dw[j] = lnw;
                R.lnx -= dx;
                if (plat) { R.nplat += 1; R.pvar += dx * dx; }
            }
            const double ls = key[B - 1];
            a.lstar[r] = ls;
            // the first survivor above L* (binary search of the sorted keys); a walk started on a point tied at L* might
            // commit it unmoved.  Only if every survivor ties a finite L* are they all start points.
            int lo = B, hi = K;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] > ls) hi = mid; else lo = mid + 1; }
            first = lo < K ? lo : B;
        }
        *run = R;
        skip = R.done;
    }
    __syncthreads();
    if (skip) return;
    // removed points' coordinates; freed slots
    for (int e = tid; e < B * D; e += NS_SEL_BLOCK) {
        const int j = e / D, d = e - j * D;
        a.dead_u[((it * a.nruns + r) * B + j) * D + d] = lu[(int64_t)idx[j] * D + d];
    }
    for (int j = tid; j < B; j += NS_SEL_BLOCK) a.freed[(int64_t)r * B + j] = idx[j];
    // survivors' mean and covariance.  The sums gather rows of live_u at random: a thread that summed a whole entry would wait
    // out ns dependent-latency loads, so every entry is split into fixed slices of the sorted survivors, one thread each, and
    // the slices are added in slice order: a fixed summation order, whatever the schedule.
    const int ns = K - B;
    {
        const int sl_n = NS_SEL_BLOCK / D;
        if (tid < D * sl_n) {
            const int d = tid % D, sl = tid / D;
            double s = 0.0;
#pragma unroll 4
            for (int m = B + sl; m < K; m += sl_n) s += lu[(int64_t)idx[m] * D + d];
            part[tid] = s;
        }
        __syncthreads();
        if (tid < D) {
            double s = 0.0;
            for (int sl = 0; sl < sl_n; ++sl) s += part[sl * D + tid];
            mean[tid] = s / (double)ns;
        }
        __syncthreads();
    }
    {
        const int ne = D * (D + 1) / 2, sl_n = NS_SEL_BLOCK / ne;
        if (tid < ne * sl_n) {
            const int e = tid % ne, sl = tid / ne;
            int p = 0, q = e;
            while (q > p) { q -= p + 1; ++p; }                  // e = p (p + 1) / 2 + q, q <= p
            double s = 0.0;
#pragma unroll 4
            for (int m = B + sl; m < K; m += sl_n) {
                const double* x = lu + (int64_t)idx[m] * D;
                s += (x[p] - mean[p]) * (x[q] - mean[q]);
            }
            part[tid] = s;
        }
        __syncthreads();
        if (tid < ne) {
            int p = 0, q = tid;
            while (q > p) { q -= p + 1; ++p; }
            double s = 0.0;
            for (int sl = 0; sl < sl_n; ++sl) s += part[sl * ne + tid];
            cov[p * D + q] = ns > 1 ? s / (double)(ns - 1) : 0.0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* L = a.chol + (int64_t)r * D * D;
        for (int p = 0; p < D; ++p) {
            for (int q = 0; q <= p; ++q) {
                double s = cov[p * D + q];
                for (int k = 0; k < q; ++k) s -= L[p * D + k] * L[q * D + k];
                if (p == q) L[p * D + p] = sqrt(s > 1e-24 ? s : 1e-24);     // a degenerate direction keeps a tiny step
                else L[p * D + q] = s / L[q * D + q];
            }
            for (int q = p + 1; q < D; ++q) L[p * D + q] = 0.0;
        }
    }
    // start points: a survivor above L* drawn uniformly (counter (run id, iteration, slot, NS_START_STEP))
    const int m0 = first;
    for (int j = tid; j < B; j += NS_SEL_BLOCK) {
        double v[2];
        ns_uniform2(a, r, (uint32_t)it, (uint32_t)j, NS_START_STEP, v);
        int m = m0 + (int)(v[0] * (double)(K - m0));
        if (m >= K) m = K - 1;
        const int src = idx[m];
        const int64_t w = (int64_t)r * B + j;
        for (int d = 0; d < D; ++d) a.wu[w * D + d] = lu[(int64_t)src * D + d];
        a.wl[w] = ll[src];
        a.wacc[w] = 0u;
        a.wev[w] = 0u;
    }
}

// One Metropolis step of every replacement walker (blockIdx.y = run).  LPW lanes hold one walker and split its energy bins
// (flux_average), computing everything else redundantly and identically: the lane count does not change a bit.
template <int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK) void k_ns_walk(const NsArgs a)
{
    const int r = blockIdx.y;
    if (a.runs[r].done) return;
    extern __shared__ __attribute__((aligned(16))) double fdyn[];
    double* fgrp = LPW > 1 ? fdyn + (threadIdx.x / LPW) * GF_FGRP_DOUBLES(a.nbins_max, LPW) : nullptr;
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * GF_MAX_DIM];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    const GfCommon& c = a.commons[r];
    const GfBsm* tb = a.tbs[r];
    const double* ptab = a.ptabs[r];
    double* ttab = ctab + GF_MAX_DIM * 4;
    if (threadIdx.x < GF_MAX_DIM * 4) ctab[threadIdx.x] = ptab[threadIdx.x];
    if (MODE == MODE_BSM_GAUSS && threadIdx.x >= 64 && threadIdx.x < 64 + 18) {
        const int k = threadIdx.x - 64, e = k >> 1;
        const int id = e == 0 ? 0 : e == 1 ? 4 : e == 2 ? 8 : e <= 4 ? 1 : e <= 6 ? 2 : 5;
        const bool im = e == 4 || e == 6 || e == 8;
        const double* srcp = (k & 1) ? (im ? tb->t2_im : tb->t2_re) : (im ? tb->t1_im : tb->t1_re);
        ttab[k] = srcp[id];
    }
    __syncthreads();
    const int t = blockIdx.x * GF_BLOCK + threadIdx.x;
    const int k = t / LPW, sub = t % LPW;
    if (k >= a.batch) return;
    const int D = a.nscan;
    const int64_t w = (int64_t)r * a.batch + k;
    const uint32_t it = (uint32_t)a.runs[r].iter;
    const double scale = a.runs[r].scale;
    const double lstar = a.lstar[r];
    double u[GF_MAX_DIM], z[GF_MAX_DIM];
    for (int p = 0; 2 * p < D; ++p) {
        double v[2];
        ns_uniform2(a, r, it, (uint32_t)k, ((uint32_t)p << 24) | (uint32_t)a.step, v);
        // Box-Muller on (1 - v0, v1): the radius stays finite
        const double rad = sqrt(-2.0 * log(1.0 - v[0]));
        double sn, cs;
        sincospi(2.0 * v[1], &sn, &cs);
        z[2 * p] = rad * cs;
        if (2 * p + 1 < D) z[2 * p + 1] = rad * sn;
    }
    const double* L = a.chol + (int64_t)r * D * D;
    bool inside = true;
    for (int p = 0; p < D; ++p) {
        double y = 0.0;
        for (int q = 0; q <= p; ++q) y = fma(L[p * D + q], z[q], y);
        u[p] = fma(scale, y, a.wu[w * D + p]);
        inside = inside && u[p] >= 0.0 && u[p] <= 1.0;
    }
    if (!inside) return;                                     // rejected without evaluating
    const int lane = threadIdx.x & (GF_WAVE - 1);
    double* row = tiles[threadIdx.x / GF_WAVE] + lane * GF_MAX_DIM;
    ns_cube_to_theta(a, c, r, u, row);
    int st;
    unsigned long long pending;
    const double lnq = proposal_lnprob<0, MODE, LPW>(c, tb, ctab, ttab, row, a.ndim, st, sub, fgrp, pending);
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    if (MODE == MODE_BSM_GAUSS && pending != 0ull) {
        // undecided unitarity: park; k_stretch_settle<Team9, true> settles and completes this step
        double* dst = a.pend_rows + (size_t)w * GF_PEND_STRIDE;
        for (int d = 0; d < a.ndim; ++d) dst[d] = row[d];
        dst[GF_MAX_DIM] = lnq;
        for (int d = 0; d < D; ++d) a.prop_u[w * D + d] = u[d];
        const unsigned int at = atomicAdd(&a.pq->count, 1u);
        if (at < a.pq->cap) {
            GfArbItem item;
            item.walker = (unsigned long long)w;
            item.mask = pending;
            a.pq->items[at] = item;
        } else {
            a.pq->overflow = 1u;                             // capacity = every walker of a step: cannot happen
        }
        return;
    }
    a.wev[w] += 1u;
    if (st == ST_NON_UNITARY) { atomicAdd(&a.nonunit[r], 1u); return; }
    if (lnq > lstar) {                                       // false for NaN and -inf
        for (int d = 0; d < D; ++d) a.wu[w * D + d] = u[d];
        a.wl[w] = lnq;
        a.wacc[w] += 1u;
    }
}

// replacements into the freed slots; s <- s exp(2 (acceptance - 0.5)); evaluation count
__global__ __launch_bounds__(GF_BLOCK) void k_ns_commit(const NsArgs a)
{
    __shared__ unsigned long long sacc[GF_BLOCK], sev[GF_BLOCK];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (a.runs[r].done) return;
    const int B = a.batch, D = a.nscan;
    unsigned long long acc = 0, ev = 0;
    for (int j = tid; j < B; j += GF_BLOCK) {
        const int64_t w = (int64_t)r * B + j;
        const int64_t slot = (int64_t)r * a.nlive + a.freed[w];
        for (int d = 0; d < D; ++d) a.live_u[slot * D + d] = a.wu[w * D + d];
        a.live_l[slot] = a.wl[w];
        acc += a.wacc[w];
        ev += a.wev[w];
    }
    sacc[tid] = acc; sev[tid] = ev;
    __syncthreads();
    for (int o = GF_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) { sacc[tid] += sacc[tid + o]; sev[tid] += sev[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        NsRun* run = a.runs + r;
        const double frac = (double)sacc[0] / ((double)B * (double)a.walks);
        double s = run->scale * exp(2.0 * (frac - 0.5));
        run->scale = s < 1e-6 ? 1e-6 : (s > 10.0 ? 10.0 : s);
        run->nevals += (int64_t)sev[0];
        run->iter += 1;
    }
}

template <int MODE, int LPW>
hipError_t launch_walk(const NsArgs& a, hipStream_t st)
{
    const size_t lds = LPW > 1 ? (size_t)(GF_BLOCK / LPW) * GF_FGRP_DOUBLES(a.nbins_max, LPW) * sizeof(double) : 0;
    const dim3 grid((unsigned)(((int64_t)a.batch * LPW + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL((k_ns_walk<MODE, LPW>), grid, dim3(GF_BLOCK), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_walk_any(int mode, int lpw, const NsArgs& a, hipStream_t st)
{
    switch (mode) {
    case MODE_PRIOR_ONLY: return launch_walk<MODE_PRIOR_ONLY, 1>(a, st);
    case MODE_SM_GAUSS: return launch_walk<MODE_SM_GAUSS, 1>(a, st);
    default:
        switch (lpw) {
        case 4: return launch_walk<MODE_BSM_GAUSS, 4>(a, st);
        case 16: return launch_walk<MODE_BSM_GAUSS, 16>(a, st);
        default: return launch_walk<MODE_BSM_GAUSS, 1>(a, st);
        }
    }
}

}  // namespace

// accessors implemented in gf_capi.hip (gf_model is private to it)
extern "C" {
int gf_model_internal(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, void** stream, int* device);
int gf_model_constants(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, int* device, int* cus,
                       int* nbins);
void gf_internal_set_error(const char* msg);
int gf_model_lnprob_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_lnprob,
                       double* d_fr, int32_t* d_status);
}

struct gf_nested {
    gf_model** models = nullptr;        // [nruns]; models[0]'s stream carries every launch
    hipStream_t stream = nullptr;
    int device = 0, cus = 256, mode = 0;
    int initialised = 0;
    int64_t dead_cap = 0;               // iterations the dead buffers hold
    int64_t launched = 0;               // iterations enqueued so far (an upper bound of every run's iteration count)
    NsArgs a = {};
    GfSettleArgs sa = {};
    GfStepState* d_state = nullptr;     // the settle kernel's step state: zeros (no stored chain)
    unsigned int* d_ctl = nullptr;
    GfCommon* d_commons = nullptr;
    const GfBsm** d_tbs = nullptr;
    const double** d_ptabs = nullptr;
    uint64_t* d_run_ids = nullptr;
    double* d_bases = nullptr;
};

namespace {
thread_local char g_nerr[256] = "";
int nfail(hipError_t e, const char* what)
{
    std::snprintf(g_nerr, sizeof(g_nerr), "%s: %s", what, hipGetErrorString(e));
    gf_internal_set_error(g_nerr);
    return GF_ERR_HIP;
}
int nmsg(int rc, const char* msg)
{
    std::snprintf(g_nerr, sizeof(g_nerr), "%s", msg);
    gf_internal_set_error(g_nerr);
    return rc;
}
#define GFN_HIP(call)                                   \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return nfail(e_, #call);  \
    } while (0)

// grow the dead buffers (iteration-major) to hold `need` iterations
int ns_grow_dead(gf_nested* s, int64_t need)
{
    if (need <= s->dead_cap) return GF_OK;
    int64_t cap = s->dead_cap > 0 ? s->dead_cap : 64;
    while (cap < need) cap *= 2;
    const size_t per = (size_t)s->a.nruns * s->a.batch;
    double *l = nullptr, *w = nullptr, *u = nullptr;
    GFN_HIP(hipMalloc((void**)&l, sizeof(double) * per * cap));
    GFN_HIP(hipMalloc((void**)&w, sizeof(double) * per * cap));
    GFN_HIP(hipMalloc((void**)&u, sizeof(double) * per * s->a.nscan * cap));
    if (s->dead_cap > 0) {
        GFN_HIP(hipMemcpyAsync(l, s->a.dead_l, sizeof(double) * per * s->dead_cap, hipMemcpyDeviceToDevice, s->stream));
        GFN_HIP(hipMemcpyAsync(w, s->a.dead_w, sizeof(double) * per * s->dead_cap, hipMemcpyDeviceToDevice, s->stream));
        GFN_HIP(hipMemcpyAsync(u, s->a.dead_u, sizeof(double) * per * s->a.nscan * s->dead_cap, hipMemcpyDeviceToDevice, s->stream));
        GFN_HIP(hipStreamSynchronize(s->stream));
        (void)hipFree(s->a.dead_l); (void)hipFree(s->a.dead_w); (void)hipFree(s->a.dead_u);
    }
    s->a.dead_l = l; s->a.dead_w = w; s->a.dead_u = u;
    s->dead_cap = cap;
    return GF_OK;
}

int ns_init(gf_nested* s)
{
    NsArgs& a = s->a;
    const dim3 grid((unsigned)((a.nlive + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(k_ns_init, grid, dim3(GF_BLOCK), 0, s->stream, a);
    GFN_HIP(hipGetLastError());
    for (int r = 0; r < a.nruns; ++r) {
        const int rc = gf_model_lnprob_on(s->models[r], s->stream, a.theta + (size_t)r * a.nlive * a.ndim, GF_LAYOUT_AOS, a.nlive,
                                          a.live_l + (size_t)r * a.nlive, nullptr, a.status + (size_t)r * a.nlive);
        if (rc != GF_OK) return rc;
    }
    hipLaunchKernelGGL(k_ns_init_fix, grid, dim3(GF_BLOCK), 0, s->stream, a);
    GFN_HIP(hipGetLastError());
    s->initialised = 1;
    return GF_OK;
}
}  // namespace

extern "C" {

int gf_nested_create(gf_model* const* models, int nruns, int nscan, const int32_t* cols, const double* bases, int nlive, int batch,
                     int walks, uint64_t seed, int on_nonunitary, gf_nested** out)
{
    if (!models || !cols || !bases || !out || nruns < 1 || nruns > 65535 || nscan < 1 || nscan > GF_MAX_DIM || nlive < 2 ||
        nlive > NS_MAX_LIVE || batch < 1 || batch >= nlive || walks < 1 || (on_nonunitary != 0 && on_nonunitary != 1))
        return GF_ERR_INVALID_ARG;
    *out = nullptr;
    const GfCommon* c0; const GfBsm* tb0; const double* pt0; void* stream0; int device0;
    if (!models[0] || gf_model_internal(models[0], &c0, &tb0, &pt0, &stream0, &device0) != GF_OK) return GF_ERR_INVALID_ARG;
    const int ndim = c0->ndim;
    std::vector<int32_t> slot(GF_MAX_DIM, -1);
    for (int k = 0; k < nscan; ++k) {
        if (cols[k] < 0 || cols[k] >= ndim || slot[cols[k]] >= 0) return GF_ERR_INVALID_ARG;
        slot[cols[k]] = k;
    }
    std::vector<GfCommon> hc(nruns);
    std::vector<const GfBsm*> htb(nruns);
    std::vector<const double*> hpt(nruns);
    std::vector<double> hb((size_t)nruns * GF_MAX_DIM, 0.0);
    int cus = 256, nbins_max = 0;
    for (int r = 0; r < nruns; ++r) {
        const GfCommon* c; int device, nb;
        if (!models[r] || gf_model_constants(models[r], &c, &htb[r], &hpt[r], &device, &cus, &nb) != GF_OK || device != device0 ||
            c->ndim != ndim || c->mode != c0->mode)
            return nmsg(GF_ERR_INVALID_ARG, "gf_nested_create: every model must share device, ndim and mode with model 0");
        hc[r] = *c;
        if (nb > nbins_max) nbins_max = nb;
        for (int d = 0; d < ndim; ++d) hb[(size_t)r * GF_MAX_DIM + d] = bases[(size_t)r * ndim + d];
    }
    gf_nested* s = new (std::nothrow) gf_nested();
    if (!s) return GF_ERR_ALLOC;
    s->models = new (std::nothrow) gf_model*[nruns];
    if (!s->models) { delete s; return GF_ERR_ALLOC; }
    for (int r = 0; r < nruns; ++r) s->models[r] = models[r];
    s->stream = (hipStream_t)stream0; s->device = device0; s->cus = cus; s->mode = c0->mode;
    NsArgs& a = s->a;
    a.seed = seed; a.tol = 0.01;
    a.nruns = nruns; a.nlive = nlive; a.batch = batch; a.nscan = nscan; a.ndim = ndim; a.walks = walks; a.raise = on_nonunitary == 0;
    a.nbins_max = nbins_max;
    for (int d = 0; d < GF_MAX_DIM; ++d) a.slot[d] = slot[d];
    const size_t R = nruns, K = nlive, B = batch, D = nscan, W = R * B;
    hipError_t e = hipSetDevice(device0);
    hipStream_t st = s->stream;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    al((void**)&s->d_commons, sizeof(GfCommon) * R);
    al((void**)&s->d_tbs, sizeof(void*) * R);
    al((void**)&s->d_ptabs, sizeof(void*) * R);
    al((void**)&s->d_run_ids, sizeof(uint64_t) * R);
    al((void**)&s->d_bases, sizeof(double) * R * GF_MAX_DIM);
    al((void**)&a.runs, sizeof(NsRun) * R);
    al((void**)&a.lstar, sizeof(double) * R);
    al((void**)&a.nonunit, sizeof(uint32_t) * R);
    al((void**)&a.live_u, sizeof(double) * R * K * D);
    al((void**)&a.live_l, sizeof(double) * R * K);
    al((void**)&a.chol, sizeof(double) * R * D * D);
    al((void**)&a.freed, sizeof(int32_t) * W);
    al((void**)&a.wu, sizeof(double) * W * D);
    al((void**)&a.wl, sizeof(double) * W);
    al((void**)&a.wacc, sizeof(uint32_t) * W);
    al((void**)&a.wev, sizeof(uint32_t) * W);
    al((void**)&a.prop_u, sizeof(double) * W * D);
    al((void**)&a.theta, sizeof(double) * R * K * ndim);
    al((void**)&a.status, sizeof(int32_t) * R * K);
    al((void**)&s->d_state, sizeof(GfStepState));
    if (s->mode == MODE_BSM_GAUSS) {
        al((void**)&a.pq, sizeof(GfArbQueue) + sizeof(GfArbItem) * W);
        al((void**)&a.pend_rows, sizeof(double) * W * GF_PEND_STRIDE);
        al((void**)&s->d_ctl, sizeof(unsigned int) * 2 * W);
    }
    std::vector<NsRun> hr(R);
    std::vector<uint64_t> ids(R);
    for (size_t r = 0; r < R; ++r) {
        NsRun& x = hr[r];
        x.lnx = 0.0; x.lnz = -HUGE_VAL; x.h = 0.0; x.lmax = -HUGE_VAL; x.scale = 1.0; x.pvar = 0.0; x.nplat = 0;
        x.iter = 0; x.nevals = (int64_t)K; x.done = 0; x.failed = 0;
        ids[r] = r;
    }
    GfArbQueue qh;
    std::memset(&qh, 0, sizeof(qh));
    qh.cap = (unsigned int)W;
    auto up = [&](void* dst, const void* src, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
    up(s->d_commons, hc.data(), sizeof(GfCommon) * R);
    up((void*)s->d_tbs, htb.data(), sizeof(void*) * R);
    up((void*)s->d_ptabs, hpt.data(), sizeof(void*) * R);
    up(s->d_run_ids, ids.data(), sizeof(uint64_t) * R);
    up(s->d_bases, hb.data(), sizeof(double) * R * GF_MAX_DIM);
    up(a.runs, hr.data(), sizeof(NsRun) * R);
    if (e == hipSuccess) e = hipMemsetAsync(a.nonunit, 0, sizeof(uint32_t) * R, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.lstar, 0, sizeof(double) * R, st);
    GfStepState hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.thin = 1;
    up(s->d_state, &hs, sizeof(hs));
    if (s->mode == MODE_BSM_GAUSS) {
        up(a.pq, &qh, offsetof(GfArbQueue, items));
        if (e == hipSuccess) e = hipMemsetAsync(s->d_ctl, 0, sizeof(unsigned int) * 2 * W, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);                  // the host vectors go out of scope
    if (e != hipSuccess) { const int rc = nfail(e, "gf_nested_create"); gf_nested_destroy(s); return rc; }
    a.commons = s->d_commons; a.tbs = s->d_tbs; a.ptabs = s->d_ptabs; a.run_ids = s->d_run_ids; a.bases = s->d_bases;
    GfSettleArgs& sa = s->sa;
    sa.state = s->d_state; sa.pq = a.pq; sa.pend_rows = a.pend_rows; sa.ctl = s->d_ctl; sa.flags = a.nonunit;
    sa.nchains = nruns; sa.nwalkers = 2 * batch; sa.ndim = ndim; sa.commons = s->d_commons; sa.tbs = s->d_tbs; sa.multi = 1;
    sa.ns_lstar = a.lstar; sa.ns_prop_u = a.prop_u; sa.ns_wu = a.wu; sa.ns_wl = a.wl; sa.ns_wacc = a.wacc; sa.ns_wev = a.wev;
    sa.ns_nonunit = a.nonunit; sa.ns_nscan = nscan;
    *out = s;
    return GF_OK;
}

int gf_nested_set_run_ids(gf_nested* s, const uint64_t* ids)
{
    if (!s || !ids) return GF_ERR_INVALID_ARG;
    if (s->initialised) return nmsg(GF_ERR_INVALID_ARG, "gf_nested_set_run_ids: before the first gf_nested_run");
    GFN_HIP(hipSetDevice(s->device));
    GFN_HIP(hipMemcpyAsync(s->d_run_ids, ids, sizeof(uint64_t) * (size_t)s->a.nruns, hipMemcpyHostToDevice, s->stream));
    GFN_HIP(hipStreamSynchronize(s->stream));
    return GF_OK;
}

int gf_nested_set_tolerance(gf_nested* s, double tol)
{
    if (!s || !(tol > 0.0)) return GF_ERR_INVALID_ARG;
    s->a.tol = tol;
    return GF_OK;
}

void gf_nested_destroy(gf_nested* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    NsArgs& a = s->a;
    void* ptrs[] = {s->d_commons, (void*)s->d_tbs, (void*)s->d_ptabs, s->d_run_ids, s->d_bases, a.runs, a.lstar, a.nonunit,
                    a.live_u, a.live_l, a.chol, a.freed, a.wu, a.wl, a.wacc, a.wev, a.prop_u, a.theta, a.status, s->d_state,
                    a.pq, a.pend_rows, s->d_ctl, a.dead_l, a.dead_w, a.dead_u};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete[] s->models;
    delete s;
}

// Iterations until every run is done.  The done flags are read back every `check` iterations; the enqueued iterations of a
// run that finished in between return at once.  max_iter (counted over this sampler's life) reached first: GF_ERR_UNSUPPORTED.
int gf_nested_run(gf_nested* s, int64_t max_iter)
{
    if (!s || max_iter < 1) return GF_ERR_INVALID_ARG;
    GFN_HIP(hipSetDevice(s->device));
    NsArgs& a = s->a;
    if (!s->initialised) { const int rc = ns_init(s); if (rc != GF_OK) return rc; }
    const int lpw = gf_propose_lanes_per_walker(s->mode, (int64_t)a.nruns * a.batch, a.nbins_max, s->cus, "GF_NESTED_LPW");
    constexpr int check = 4;
    std::vector<NsRun> hr(a.nruns);
    for (;;) {
        GFN_HIP(hipMemcpyAsync(hr.data(), a.runs, sizeof(NsRun) * a.nruns, hipMemcpyDeviceToHost, s->stream));
        GFN_HIP(hipStreamSynchronize(s->stream));
        bool all = true;
        int64_t most = 0;
        for (const NsRun& x : hr) { all = all && x.done; if (!x.done && x.iter > most) most = x.iter; }
        if (all) break;
        if (most >= max_iter) return nmsg(GF_ERR_UNSUPPORTED, "gf_nested_run: max_iter reached before every run met its tolerance");
        for (int i = 0; i < check; ++i) {
            const int rc = ns_grow_dead(s, s->launched + 1);
            if (rc != GF_OK) return rc;
            hipLaunchKernelGGL(k_ns_select, dim3(a.nruns), dim3(NS_SEL_BLOCK), 0, s->stream, a);
            GFN_HIP(hipGetLastError());
            for (int step = 0; step < a.walks; ++step) {
                a.step = step;
                GFN_HIP(launch_walk_any(s->mode, lpw, a, s->stream));
                if (s->mode == MODE_BSM_GAUSS) GFN_HIP(gf_launch_nested_settle(s->sa, s->cus, s->stream));
            }
            hipLaunchKernelGGL(k_ns_commit, dim3(a.nruns), dim3(GF_BLOCK), 0, s->stream, a);
            GFN_HIP(hipGetLastError());
            s->launched += 1;
        }
    }
    return GF_OK;
}

int gf_nested_result(gf_nested* s, double* lnz, double* lnz_err, double* info, double* max_lnl, int64_t* niter, int64_t* nevals,
                     uint32_t* nonunitary, int32_t* failed)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GFN_HIP(hipSetDevice(s->device));
    const int R = s->a.nruns;
    std::vector<NsRun> hr(R);
    std::vector<uint32_t> nu(R);
    GFN_HIP(hipMemcpyAsync(hr.data(), s->a.runs, sizeof(NsRun) * R, hipMemcpyDeviceToHost, s->stream));
    GFN_HIP(hipMemcpyAsync(nu.data(), s->a.nonunit, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, s->stream));
    GFN_HIP(hipStreamSynchronize(s->stream));
    for (int r = 0; r < R; ++r) {
        const NsRun& x = hr[r];
        if (lnz) lnz[r] = x.lnz;
        if (lnz_err) lnz_err[r] = std::sqrt((x.h > 0.0 ? x.h : 0.0) / (double)s->a.nlive + x.pvar);
        if (info) info[r] = x.h;
        if (max_lnl) max_lnl[r] = x.lmax;
        if (niter) niter[r] = x.iter;
        if (nevals) nevals[r] = x.nevals;
        if (nonunitary) nonunitary[r] = nu[r];
        if (failed) failed[r] = x.failed;
    }
    return GF_OK;
}

// Test access, not declared in the header: every run's walk step scale s and ln X, [nruns] each; NULL = skip.  With the live
// set and the dead rows (gf_nested_get_dead) they are the whole state the next iteration starts from.
int gf_internal_nested_state(gf_nested* s, double* scale, double* lnx)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GFN_HIP(hipSetDevice(s->device));
    const int R = s->a.nruns;
    std::vector<NsRun> hr(R);
    GFN_HIP(hipMemcpyAsync(hr.data(), s->a.runs, sizeof(NsRun) * R, hipMemcpyDeviceToHost, s->stream));
    GFN_HIP(hipStreamSynchronize(s->stream));
    for (int r = 0; r < R; ++r) {
        if (scale) scale[r] = hr[r].scale;
        if (lnx) lnx[r] = hr[r].lnx;
    }
    return GF_OK;
}

// Run `run`'s dead points in removal order, then its final live set: n = iterations * batch + nlive rows.  lnl [n], lnw [n]
// (log-weights; the live set's are ln X_final - ln nlive + lnL), cube [n][nscan]; NULL = skip.  With every pointer NULL only *n
// is set.  cap: rows the caller's arrays hold.
int gf_nested_get_dead(gf_nested* s, int run, int64_t cap, double* lnl, double* lnw, double* cube, int64_t* n)
{
    if (!s || !n || run < 0 || run >= s->a.nruns) return GF_ERR_INVALID_ARG;
    GFN_HIP(hipSetDevice(s->device));
    const NsArgs& a = s->a;
    NsRun x;
    GFN_HIP(hipMemcpyAsync(&x, a.runs + run, sizeof(NsRun), hipMemcpyDeviceToHost, s->stream));
    GFN_HIP(hipStreamSynchronize(s->stream));
    const int64_t nd = x.iter * a.batch, total = nd + a.nlive;
    *n = total;
    if (!lnl && !lnw && !cube) return GF_OK;
    if (cap < total) return nmsg(GF_ERR_INVALID_ARG, "gf_nested_get_dead: cap is smaller than the number of rows");
    const size_t B = a.batch, D = a.nscan, R = a.nruns;
    for (int64_t it = 0; it < x.iter; ++it) {
        const size_t off = ((size_t)it * R + run) * B;
        if (lnl) GFN_HIP(hipMemcpyAsync(lnl + it * B, a.dead_l + off, sizeof(double) * B, hipMemcpyDeviceToHost, s->stream));
        if (lnw) GFN_HIP(hipMemcpyAsync(lnw + it * B, a.dead_w + off, sizeof(double) * B, hipMemcpyDeviceToHost, s->stream));
        if (cube) GFN_HIP(hipMemcpyAsync(cube + it * B * D, a.dead_u + off * D, sizeof(double) * B * D, hipMemcpyDeviceToHost, s->stream));
    }
    double* ll = lnl ? lnl + nd : (double*)std::malloc(sizeof(double) * a.nlive);
    if (!ll) return GF_ERR_ALLOC;
    GFN_HIP(hipMemcpyAsync(ll, a.live_l + (size_t)run * a.nlive, sizeof(double) * a.nlive, hipMemcpyDeviceToHost, s->stream));
    if (cube) GFN_HIP(hipMemcpyAsync(cube + nd * D, a.live_u + (size_t)run * a.nlive * D, sizeof(double) * a.nlive * D,
                                     hipMemcpyDeviceToHost, s->stream));
    const hipError_t e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess && lnw)
        for (int k = 0; k < a.nlive; ++k) lnw[nd + k] = x.lnx - std::log((double)a.nlive) + ll[k];
    if (!lnl) std::free(ll);
    if (e != hipSuccess) return nfail(e, "gf_nested_get_dead");
    return GF_OK;
}

}  // extern "C"
