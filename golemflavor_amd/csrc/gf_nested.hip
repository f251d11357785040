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
#include <cstdlib>
#include <vector>

#include "gf_cube_runs.hpp"

namespace {

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

struct NsArgs : GfCubeRuns {       // pq: capacity R * B
    int32_t nlive, batch, walks, raise, step;     // first: next to GfCubeRuns::nscan in the kernel arguments
    double tol;
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
    double* dead_l;                 // [cap][R][B] (iteration-major: growing the buffer is one copy)
    double* dead_w;                 // [cap][R][B] log-weights
    double* dead_u;                 // [cap][R][B][D]
    double* theta;                  // [R][K][ndim] initial points (k_cube_draw)
    int32_t* status;                // [R][K]
};

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
        cube_uniform2(a, r, (uint32_t)it, (uint32_t)j, NS_START_STEP, v);
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
    constexpr bool BSM = MODE == MODE_BSM_GAUSS || MODE == MODE_BSM_BINNED || MODE == MODE_BSM_TABLE;
    __shared__ __attribute__((aligned(16))) double btab[MODE == MODE_BSM_BINNED ? GF_BINNED_DOUBLES : 1];   // the run's binned measurement
    load_eval_tables(ctab, ptab, tb, BSM);
    if constexpr (MODE == MODE_BSM_BINNED) load_binned_table(btab, a.btabs[r], tb->nbins);
    // the run's tabulated likelihood stays in global memory: the table instance alone reads the two arrays
    const double* ltab = btab;
    int tside = 0;
    if constexpr (MODE == MODE_BSM_TABLE) { ltab = a.ttabs[r]; tside = a.tsides[r]; }
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
        cube_uniform2(a, r, it, (uint32_t)k, ((uint32_t)p << 24) | (uint32_t)a.step, v);
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
    cube_to_theta(a, c, r, u, row);
    int st;
    unsigned long long pending;
    const double lnq = proposal_lnprob<0, MODE, LPW>(c, tb, ctab, ttab, row, a.ndim, st, sub, fgrp, pending, ltab, tside);
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    if (BSM && pending != 0ull) {
        // undecided unitarity: park; k_stretch_settle<Team9, true> settles and completes this step
        for (int d = 0; d < D; ++d) a.prop_u[w * D + d] = u[d];
        park_proposal(a.pq, a.pend_rows, w, row, a.ndim, lnq, pending);
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

hipError_t launch_walk_any(int mode, int lpw, const NsArgs& a, hipStream_t st)
{
    return launch_mode_lpw(mode, lpw, [&](auto m, auto l) {
        return launch_points(k_ns_walk<decltype(m)::value, decltype(l)::value>, a, l, a.batch, st);
    });
}

}  // namespace

struct gf_nested {
    GfCubeRunsHost rs;
    int64_t dead_cap = 0;               // iterations the dead buffers hold
    int64_t launched = 0;               // iterations enqueued so far (an upper bound of every run's iteration count)
    NsArgs a = {};
    GfSettleArgs sa = {};
};

namespace {

// grow the dead buffers (iteration-major) to hold `need` iterations
int ns_grow_dead(gf_nested* s, int64_t need)
{
    if (need <= s->dead_cap) return GF_OK;
    int64_t cap = s->dead_cap > 0 ? s->dead_cap : 64;
    while (cap < need) cap *= 2;
    const size_t per = (size_t)s->a.nruns * s->a.batch;
    double *l = nullptr, *w = nullptr, *u = nullptr;
    GF_HIP(hipMalloc((void**)&l, sizeof(double) * per * cap));
    GF_HIP(hipMalloc((void**)&w, sizeof(double) * per * cap));
    GF_HIP(hipMalloc((void**)&u, sizeof(double) * per * s->a.nscan * cap));
    if (s->dead_cap > 0) {
        GF_HIP(hipMemcpyAsync(l, s->a.dead_l, sizeof(double) * per * s->dead_cap, hipMemcpyDeviceToDevice, s->rs.set.stream));
        GF_HIP(hipMemcpyAsync(w, s->a.dead_w, sizeof(double) * per * s->dead_cap, hipMemcpyDeviceToDevice, s->rs.set.stream));
        GF_HIP(hipMemcpyAsync(u, s->a.dead_u, sizeof(double) * per * s->a.nscan * s->dead_cap, hipMemcpyDeviceToDevice, s->rs.set.stream));
        GF_HIP(hipStreamSynchronize(s->rs.set.stream));
        (void)hipFree(s->a.dead_l); (void)hipFree(s->a.dead_w); (void)hipFree(s->a.dead_u);
    }
    s->a.dead_l = l; s->a.dead_w = w; s->a.dead_u = u;
    s->dead_cap = cap;
    return GF_OK;
}

// K cube points per run (iteration word NS_INIT_ITER), evaluated by the bulk lnprob path
int ns_init(gf_nested* s)
{
    NsArgs& a = s->a;
    const int rc = cube_runs_draw(s->rs, a, NS_INIT_ITER, a.nlive, a.live_u, a.theta, a.live_l, a.status);
    if (rc != GF_OK) return rc;
    const dim3 grid((unsigned)((a.nlive + GF_BLOCK - 1) / GF_BLOCK), a.nruns);
    hipLaunchKernelGGL(k_ns_init_fix, grid, dim3(GF_BLOCK), 0, s->rs.set.stream, a);
    GF_HIP(hipGetLastError());
    s->rs.initialised = 1;
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
    gf_nested* s = new (std::nothrow) gf_nested();
    if (!s) return GF_ERR_ALLOC;
    NsArgs& a = s->a;
    const int rc = cube_runs_create(s->rs, a, models, nruns, nscan, cols, bases, seed, "gf_nested_create");
    if (rc != GF_OK) { delete s; return rc; }
    a.tol = 0.01;
    a.nlive = nlive; a.batch = batch; a.walks = walks; a.raise = on_nonunitary == 0;
    const size_t R = nruns, K = nlive, B = batch, D = nscan, W = R * B;
    hipError_t e = hipSuccess;
    hipStream_t st = s->rs.set.stream;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
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
    al((void**)&a.theta, sizeof(double) * R * K * a.ndim);
    al((void**)&a.status, sizeof(int32_t) * R * K);
    std::vector<NsRun> hr(R);
    for (size_t r = 0; r < R; ++r) {
        NsRun& x = hr[r];
        x.lnx = 0.0; x.lnz = -HUGE_VAL; x.h = 0.0; x.lmax = -HUGE_VAL; x.scale = 1.0; x.pvar = 0.0; x.nplat = 0;
        x.iter = 0; x.nevals = (int64_t)K; x.done = 0; x.failed = 0;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(a.runs, hr.data(), sizeof(NsRun) * R, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.nonunit, 0, sizeof(uint32_t) * R, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.lstar, 0, sizeof(double) * R, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                  // hr goes out of scope
    if (e == hipSuccess) e = cube_runs_alloc_queue(s->rs, a, W);
    if (e != hipSuccess) { const int rc2 = gf_hip_fail(e, "gf_nested_create"); gf_nested_destroy(s); return rc2; }
    GfSettleArgs& sa = s->sa;
    cube_runs_settle_args(s->rs, a, 2 * batch, sa);
    sa.flags = a.nonunit;
    sa.ns_lstar = a.lstar; sa.ns_prop_u = a.prop_u; sa.ns_wu = a.wu; sa.ns_wl = a.wl; sa.ns_wacc = a.wacc; sa.ns_wev = a.wev;
    sa.ns_nonunit = a.nonunit; sa.ns_nscan = nscan;
    *out = s;
    return GF_OK;
}

int gf_nested_set_run_ids(gf_nested* s, const uint64_t* ids)
{
    if (!s || !ids) return GF_ERR_INVALID_ARG;
    return cube_runs_set_ids(s->rs, s->a, ids, "gf_nested_set_run_ids: before the first gf_nested_run");
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
    NsArgs& a = s->a;
    cube_runs_free(s->rs, a);
    void* ptrs[] = {a.runs, a.lstar, a.nonunit, a.live_u, a.live_l, a.chol, a.freed, a.wu, a.wl, a.wacc, a.wev, a.prop_u, a.theta,
                    a.status, a.dead_l, a.dead_w, a.dead_u};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete s;
}

// Iterations until every run is done.  The done flags are read back every `check` iterations; the enqueued iterations of a
// run that finished in between return at once.  max_iter (counted over this sampler's life) reached first: GF_ERR_UNSUPPORTED.
int gf_nested_run(gf_nested* s, int64_t max_iter)
{
    if (!s || max_iter < 1) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    NsArgs& a = s->a;
    if (const int rc = cube_runs_begin(s->rs, "gf_nested_run")) return rc;
    if (!s->rs.initialised) { const int rc = ns_init(s); if (rc != GF_OK) return rc; }
    const int lpw = lanes_per_walker(gf_modelset_eval_mode(&s->rs.set), (int64_t)a.nruns * a.batch, a.nbins_max, s->rs.set.cus, {false, 32 * 1024, "GF_NESTED_LPW"});
    constexpr int check = 4;
    std::vector<NsRun> hr(a.nruns);
    for (;;) {
        GF_HIP(hipMemcpyAsync(hr.data(), a.runs, sizeof(NsRun) * a.nruns, hipMemcpyDeviceToHost, s->rs.set.stream));
        GF_HIP(hipStreamSynchronize(s->rs.set.stream));
        bool all = true;
        int64_t most = 0;
        for (const NsRun& x : hr) { all = all && x.done; if (!x.done && x.iter > most) most = x.iter; }
        if (all) break;
        if (most >= max_iter) return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_nested_run: max_iter reached before every run met its tolerance");
        for (int i = 0; i < check; ++i) {
            const int rc = ns_grow_dead(s, s->launched + 1);
            if (rc != GF_OK) return rc;
            hipLaunchKernelGGL(k_ns_select, dim3(a.nruns), dim3(NS_SEL_BLOCK), 0, s->rs.set.stream, a);
            GF_HIP(hipGetLastError());
            for (int step = 0; step < a.walks; ++step) {
                a.step = step;
                GF_HIP(launch_walk_any(gf_modelset_eval_mode(&s->rs.set), lpw, a, s->rs.set.stream));
                if (s->rs.set.mode == MODE_BSM_GAUSS) GF_HIP(gf_launch_nested_settle(s->sa, s->rs.set.cus, s->rs.set.stream));
            }
            hipLaunchKernelGGL(k_ns_commit, dim3(a.nruns), dim3(GF_BLOCK), 0, s->rs.set.stream, a);
            GF_HIP(hipGetLastError());
            s->launched += 1;
        }
    }
    return GF_OK;
}

int gf_nested_result(gf_nested* s, double* lnz, double* lnz_err, double* info, double* max_lnl, int64_t* niter, int64_t* nevals,
                     uint32_t* nonunitary, int32_t* failed)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    const int R = s->a.nruns;
    std::vector<NsRun> hr(R);
    std::vector<uint32_t> nu(R);
    GF_HIP(hipMemcpyAsync(hr.data(), s->a.runs, sizeof(NsRun) * R, hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipMemcpyAsync(nu.data(), s->a.nonunit, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
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
    GF_HIP(hipSetDevice(s->rs.set.device));
    const int R = s->a.nruns;
    std::vector<NsRun> hr(R);
    GF_HIP(hipMemcpyAsync(hr.data(), s->a.runs, sizeof(NsRun) * R, hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    for (int r = 0; r < R; ++r) {
        if (scale) scale[r] = hr[r].scale;
        if (lnx) lnx[r] = hr[r].lnx;
    }
    return GF_OK;
}

// What gf_nested_post.hip reads: the device buffers of the runs' points (gf_internal.h)
int gf_internal_nested_view(gf_nested* s, GfNestedView* v, GfNestedRunState* state)
{
    if (!s || !v) return GF_ERR_INVALID_ARG;
    const NsArgs& a = s->a;
    v->device = s->rs.set.device; v->stream = s->rs.set.stream; v->cus = s->rs.set.cus;
    v->nruns = a.nruns; v->nlive = a.nlive; v->batch = a.batch; v->nscan = a.nscan; v->ndim = a.ndim;
    v->seed = a.seed;
    for (int d = 0; d < GF_MAX_DIM; ++d) v->slot[d] = a.slot[d];
    v->d_commons = a.commons; v->d_bases = a.bases; v->d_run_ids = a.run_ids;
    v->d_dead_l = a.dead_l; v->d_dead_w = a.dead_w; v->d_dead_u = a.dead_u;
    v->d_live_l = a.live_l; v->d_live_u = a.live_u;
    v->models = s->rs.set.models.data();
    if (!state) return GF_OK;
    GF_HIP(hipSetDevice(s->rs.set.device));
    std::vector<NsRun> hr(a.nruns);
    GF_HIP(hipMemcpyAsync(hr.data(), a.runs, sizeof(NsRun) * a.nruns, hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    for (int r = 0; r < a.nruns; ++r) {
        const NsRun& x = hr[r];
        state[r].iter = x.iter; state[r].lnx = x.lnx; state[r].lnz = x.lnz;
        state[r].done = s->rs.initialised ? x.done : 0; state[r].failed = x.failed;
    }
    return GF_OK;
}

// Run `run`'s dead points in removal order, then its final live set: n = iterations * batch + nlive rows.  lnl [n], lnw [n]
// (log-weights; the live set's are ln X_final - ln nlive + lnL), cube [n][nscan]; NULL = skip.  With every pointer NULL only *n
// is set.  cap: rows the caller's arrays hold.
int gf_nested_get_dead(gf_nested* s, int run, int64_t cap, double* lnl, double* lnw, double* cube, int64_t* n)
{
    if (!s || !n || run < 0 || run >= s->a.nruns) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    const NsArgs& a = s->a;
    NsRun x;
    GF_HIP(hipMemcpyAsync(&x, a.runs + run, sizeof(NsRun), hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    const int64_t nd = x.iter * a.batch, total = nd + a.nlive;
    *n = total;
    if (!lnl && !lnw && !cube) return GF_OK;
    if (cap < total) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_nested_get_dead: cap is smaller than the number of rows");
    const size_t B = a.batch, D = a.nscan, R = a.nruns;
    for (int64_t it = 0; it < x.iter; ++it) {
        const size_t off = ((size_t)it * R + run) * B;
        if (lnl) GF_HIP(hipMemcpyAsync(lnl + it * B, a.dead_l + off, sizeof(double) * B, hipMemcpyDeviceToHost, s->rs.set.stream));
        if (lnw) GF_HIP(hipMemcpyAsync(lnw + it * B, a.dead_w + off, sizeof(double) * B, hipMemcpyDeviceToHost, s->rs.set.stream));
        if (cube) GF_HIP(hipMemcpyAsync(cube + it * B * D, a.dead_u + off * D, sizeof(double) * B * D, hipMemcpyDeviceToHost, s->rs.set.stream));
    }
    double* ll = lnl ? lnl + nd : (double*)std::malloc(sizeof(double) * a.nlive);
    if (!ll) return GF_ERR_ALLOC;
    GF_HIP(hipMemcpyAsync(ll, a.live_l + (size_t)run * a.nlive, sizeof(double) * a.nlive, hipMemcpyDeviceToHost, s->rs.set.stream));
    if (cube) GF_HIP(hipMemcpyAsync(cube + nd * D, a.live_u + (size_t)run * a.nlive * D, sizeof(double) * a.nlive * D,
                                     hipMemcpyDeviceToHost, s->rs.set.stream));
    const hipError_t e = hipStreamSynchronize(s->rs.set.stream);
    if (e == hipSuccess && lnw)
        for (int k = 0; k < a.nlive; ++k) lnw[nd + k] = x.lnx - std::log((double)a.nlive) + ll[k];
    if (!lnl) std::free(ll);
    if (e != hipSuccess) return gf_hip_fail(e, "gf_nested_get_dead");
    return GF_OK;
}

}  // extern "C"
