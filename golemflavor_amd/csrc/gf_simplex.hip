// gf_simplex.hip -- device multi-start Nelder-Mead maximiser of ln_prob: the profile likelihood of scripts/sens.py's frequentist
// statistic (golemflavor/plot.py:605-608 plots -2 (max lnL(scale) - max lnL(null))) at every new-physics scale at once.
//
// Every run r (one posterior, one gf_model) minimises f(u) = -ln_prob(theta(u)) over the unit cube of its scanned columns,
// theta_i = (hi_i - lo_i) u_i + lo_i (the nested sampler's map, product and sum each rounded), every other column at its base
// value; ln_prob = -inf or NaN is f = +inf.  Each start follows scipy.optimize._optimize._minimize_neldermead (scipy 1.15.3,
// bounds = [0, 1]^n) step for step: the same initial simplex (x0 clipped, vertex k+1 = x0 with coordinate k times 1.05 or set
// to 0.00025, reflected across the upper bound, clipped), the same centroid (rows summed one after another, then divided), the
// same candidate arithmetic (no FMA contraction: `#pragma clang fp contract(off)` in every function that forms a point), the
// same clipping, decisions, termination test and nfev count.  The vertices are sorted stably (ties in index order).
//
// One evaluation round per iteration: scipy evaluates xr and then at most one of xe, xc, xcc; here the step kernel forms all
// four for every live start and k_sx_eval evaluates them in one launch; k_sx_step then applies scipy's sequential decision
// table to the four values (the trajectory is scipy's; only the device evaluation count is higher, reported apart from nfev).
// A shrink needs n more evaluations: the step kernel forms the shrunk vertices and the next round evaluates them.  Candidates
// whose unitarity verdict the in-kernel tiers cannot settle are parked and settled by the emulated-x87 team
// (k_stretch_settle<Team9, false, true>, gf_unitarity.hip) before k_sx_step runs.  A non-unitary verdict counts only for a
// candidate scipy's sequential algorithm would have evaluated: a speculative xe that scipy never evaluates neither fails a run
// nor adds to its count.
//
// Starts: nseed uniform cube points per run (Philox4x32-10 keyed by the seed, counter (run id, SX_SEED_ITER, point, pair of
// coordinates): disjoint from the nested sampler's draws), evaluated by the bulk lnprob path with its own arbitration; the K
// best finite ones (lnL descending, then index ascending) are the starts, the caller's starts follow.  A converged start may be
// restarted from its best vertex with a fresh initial simplex (scipy.optimize.minimize again with x0 = res.x), until the gain
// is at most fatol or the restarts are used up.  The host loop reads the per-run counts of live starts back every few rounds;
// it is not captured into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "gf_cube_runs.hpp"

namespace {

constexpr int SX_PICK_BLOCK = 256;
constexpr int SX_STEP_BLOCK = 64;
constexpr int32_t SX_PARKED = -1;                  // status of a candidate waiting for the settle kernel

enum : int32_t { PH_INIT = 0, PH_ITER = 1, PH_SHRINK = 2 };

struct SxStart {
    double fprev;           // f of the previous minimize call's result (restarts)
    int64_t nfev;           // scipy's count, summed over the calls
    int64_t devals;         // device evaluations
    int32_t nit;            // scipy's nit, summed over the calls
    int32_t nit_cur;        // scipy's `iterations` of the current call
    int32_t phase, npend, calls, done, used;
    int32_t pad;
};

struct SxRun {
    int32_t active;         // starts not yet done
    int32_t nstarts;        // starts used
    int32_t failed;         // on_nonunitary == raise and a candidate scipy evaluates is non-unitary
    uint32_t nonunit;       // non-unitary points counted (seeding and evaluated candidates)
    uint32_t parked;        // candidates whose unitarity verdict the settle kernel took
    uint32_t pad;
};

struct SxArgs : GfCubeRuns {       // pq: capacity R * S * Q
    int32_t nstarts, nuser, nseed, maxiter, restarts, raise;     // first: next to GfCubeRuns::nscan (k_sx_pick loads them together)
    int32_t S, P;                   // starts per run (nstarts + nuser), vertices per simplex (nscan + 1)
    int32_t Q;                      // points per start and round: max(P, 4) -- the initial simplex, the four candidates, a shrink
    SxRun* runs;                    // [R]
    SxStart* starts;                // [R][S]
    double* sim;                    // [R][S][P][N]
    double* fsim;                   // [R][S][P]
    double* tmp;                    // [R][S][P][N] sort buffer
    double* pts;                    // [R][S][Q][N] points of the next evaluation round
    double* lnq;                    // [R][S][Q] their lnprob
    int32_t* pst;                   // [R][S][Q] their status
    const double* ustart;           // [R][nuser][N] caller's starts
    double* seed_u;                 // [R][M][N]
    double* seed_l;                 // [R][M]
    int32_t* seed_st;               // [R][M]
    double* theta;                  // [R][M][ndim]
    double coef[9];                 // 1 + rho, rho, 1 + rho chi, rho chi, 1 + psi rho, psi rho, 1 - psi, psi, sigma
    double xatol, fatol;
};

// np.clip(x, 0, 1): maximum(x, 0) then minimum(., 1), NaN kept; -0.0 becomes +0.0 as in numpy
__device__ __forceinline__ double sx_clip(double x)
{
    if (x != x) return x;
    const double m = x > 0.0 ? x : 0.0;
    return m < 1.0 ? m : 1.0;
}

// f of a round's point: -lnprob, +inf for -inf, NaN or a non-unitary verdict
__device__ __forceinline__ double sx_f(double lnq, int32_t st) { return (st != ST_NON_UNITARY && lnq > -gf_inf()) ? -lnq : gf_inf(); }

// a fresh initial simplex around x0 (_minimize_neldermead with bounds [0, 1]^n): every vertex goes to the next round
__device__ void sx_begin(const SxArgs& a, int64_t s, const double* x0)
{
#pragma clang fp contract(off)
    const int N = a.nscan, P = a.P;
    double* sim = a.sim + s * P * N;
    double* pts = a.pts + s * a.Q * N;
    const double nonzdelt = 1.0 + 0.05;                  // (1 + nonzdelt) * y[k]
    for (int d = 0; d < N; ++d) sim[d] = sx_clip(x0[d]);
    for (int k = 0; k < N; ++k)
        for (int d = 0; d < N; ++d) {
            double y = sim[d];
            if (d == k) y = y != 0.0 ? nonzdelt * y : 0.00025;
            sim[(k + 1) * N + d] = y;
        }
    for (int e = 0; e < P * N; ++e) {
        double y = sim[e];
        if (y > 1.0) y = 2.0 * 1.0 - y;                 // reflect into the interior, then clip
        sim[e] = sx_clip(y);
        pts[e] = sim[e];
    }
    SxStart& st = a.starts[s];
    st.phase = PH_INIT;
    st.npend = P;
    st.nit_cur = 0;
}

// one workgroup per run: a seed point the reference would have raised on is outside the support (-inf) and counted (and fails
// the run in raise mode); NaN is -inf too.
// The K best finite seeds (lnL descending, index ascending) then the caller's starts become starts; the rest stay unused.
__global__ __launch_bounds__(SX_PICK_BLOCK) void k_sx_pick(const SxArgs a)
{
    __shared__ double bl[SX_PICK_BLOCK];
    __shared__ int bi[SX_PICK_BLOCK];
    __shared__ int found;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int M = a.nseed, N = a.nscan;
    double* sl = a.seed_l + (int64_t)r * M;
    unsigned int nu = 0;
    for (int i = tid; i < M; i += SX_PICK_BLOCK) {
        const double l = sl[i];
        if (a.seed_st[(int64_t)r * M + i] == ST_NON_UNITARY) { sl[i] = -gf_inf(); ++nu; }
        else if (l != l) sl[i] = -gf_inf();
    }
    if (nu) atomicAdd(&a.runs[r].nonunit, nu);
    if (tid == 0) found = 0;
    __syncthreads();
    // a seed point the reference would have raised on fails the run in raise mode, as the nested sampler's initial draws do
    const bool fail = a.raise && atomicAdd(&a.runs[r].nonunit, 0u) != 0u;
    if (fail) {
        for (int j = tid; j < a.S; j += SX_PICK_BLOCK) {
            SxStart& st = a.starts[(int64_t)r * a.S + j];
            st.done = 1; st.npend = 0;
        }
        if (tid == 0) { a.runs[r].failed = 1; a.runs[r].nstarts = 0; a.runs[r].active = 0; }
        return;
    }
    // round k takes the best seed below the one round k - 1 took, in the order (lnL descending, index ascending)
    double pl = gf_inf();
    int pi = -1;
    for (int k = 0; k < a.nstarts; ++k) {
        double best = -gf_inf();
        int bidx = M;
        for (int i = tid; i < M; i += SX_PICK_BLOCK) {
            const double l = sl[i];
            const bool below = l < pl || (l == pl && i > pi);
            if (below && (l > best || (l == best && i < bidx))) { best = l; bidx = i; }
        }
        bl[tid] = best; bi[tid] = bidx;
        __syncthreads();
        for (int o = SX_PICK_BLOCK / 2; o > 0; o >>= 1) {
            if (tid < o && (bl[tid + o] > bl[tid] || (bl[tid + o] == bl[tid] && bi[tid + o] < bi[tid]))) {
                bl[tid] = bl[tid + o]; bi[tid] = bi[tid + o];
            }
            __syncthreads();
        }
        pl = bl[0]; pi = bi[0];
        __syncthreads();
        if (!(pl > -gf_inf())) break;                   // no finite seed left (the same on every thread)
        if (tid == 0) {
            const int64_t s = (int64_t)r * a.S + k;
            sx_begin(a, s, a.seed_u + ((int64_t)r * M + pi) * N);
            a.starts[s].used = 1;
            found = k + 1;
        }
    }
    __syncthreads();
    const int nf = found;
    for (int j = tid; j < a.nuser; j += SX_PICK_BLOCK) {
        const int64_t s = (int64_t)r * a.S + nf + j;
        sx_begin(a, s, a.ustart + ((int64_t)r * a.nuser + j) * N);
        a.starts[s].used = 1;
    }
    for (int j = nf + a.nuser + tid; j < a.S; j += SX_PICK_BLOCK) {
        SxStart& st = a.starts[(int64_t)r * a.S + j];
        st.done = 1; st.npend = 0;
    }
    if (tid == 0) { a.runs[r].nstarts = nf + a.nuser; a.runs[r].active = nf + a.nuser; }
}

// Realisation ensembles (gf_toys.hip): run r keeps the first counts[r] of its caller's starts, the rest become unused, as the starts
// behind a run's finite seeds are -- right behind k_sx_pick, before the first evaluation round.  One workgroup per run.
__global__ __launch_bounds__(SX_PICK_BLOCK) void k_sx_trim(const SxArgs a, const int32_t* __restrict__ counts)
{
    const int r = blockIdx.x;
    if (a.runs[r].failed) return;
    const int c = counts[r] < a.S ? counts[r] : a.S;                 // (a later gf_simplex_set_starts may have given fewer starts)
    for (int j = c + threadIdx.x; j < a.S; j += SX_PICK_BLOCK) {
        SxStart& st = a.starts[(int64_t)r * a.S + j];
        st.done = 1; st.npend = 0; st.used = 0;
    }
    if (threadIdx.x == 0) { a.runs[r].nstarts = c; a.runs[r].active = c; }
}

// every pending point of every live start (blockIdx.y = run); LPW lanes per point as in the nested sampler's walk
template <int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK) void k_sx_eval(const SxArgs a)
{
    const int r = blockIdx.y;
    if (a.runs[r].active == 0 || a.runs[r].failed) return;
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
    if (k >= a.S * a.Q) return;
    const int j = k / a.Q, p = k - j * a.Q;
    const int64_t s = (int64_t)r * a.S + j;
    const SxStart& st = a.starts[s];
    if (st.done || p >= st.npend) return;
    const int64_t w = s * a.Q + p;
    const int lane = threadIdx.x & (GF_WAVE - 1);
    double* row = tiles[threadIdx.x / GF_WAVE] + lane * GF_MAX_DIM;
    cube_to_theta(a, c, r, a.pts + w * a.nscan, row);
    int status;
    unsigned long long pending;
    const double lnq = proposal_lnprob<0, MODE, LPW>(c, tb, ctab, ttab, row, a.ndim, status, sub, fgrp, pending, ltab, tside);
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    if (BSM && pending != 0ull) {
        // undecided unitarity: park; k_stretch_settle<Team9, false, true> writes lnq and the verdict
        a.pst[w] = SX_PARKED;
        atomicAdd(&a.runs[r].parked, 1u);
        park_proposal(a.pq, a.pend_rows, w, row, a.ndim, lnq, pending);
        return;
    }
    a.lnq[w] = lnq;
    a.pst[w] = status;
}

// np.argsort(fsim) (stable: ties in index order), then sim and fsim taken in that order; `ind` and `fo` are this thread's
// rows of LDS (GF_MAX_DIM + 1 entries each)
__device__ void sx_sort(const SxArgs& a, int64_t s, int* ind, double* fo)
{
    const int N = a.nscan, P = a.P;
    double* sim = a.sim + s * P * N;
    double* fs = a.fsim + s * P;
    double* tmp = a.tmp + s * P * N;
    for (int k = 0; k < P; ++k) ind[k] = k;
    // insertion sort of the indices by f; only strictly smaller keys move ahead
    for (int k = 1; k < P; ++k) {
        const int v = ind[k];
        const double fv = fs[v];
        int m = k;
        while (m > 0 && fs[ind[m - 1]] > fv) { ind[m] = ind[m - 1]; --m; }
        ind[m] = v;
    }
    for (int k = 0; k < P; ++k)
        for (int d = 0; d < N; ++d) tmp[k * N + d] = sim[ind[k] * N + d];
    for (int k = 0; k < P; ++k) fo[k] = fs[ind[k]];
    for (int k = 0; k < P; ++k) fs[k] = fo[k];
    for (int e = 0; e < P * N; ++e) sim[e] = tmp[e];
}

// a point scipy evaluates: its non-unitary verdict fails the run (raise) or is counted (-inf); false if the run failed
__device__ __forceinline__ bool sx_use(const SxArgs& a, int r, int32_t status)
{
    if (status != ST_NON_UNITARY) return true;
    if (a.raise) { atomicExch(&a.runs[r].failed, 1); return false; }
    atomicAdd(&a.runs[r].nonunit, 1u);
    return true;
}

// scipy's loop head for a sorted simplex: maxiter, then the xatol / fatol test; otherwise the four candidates of the next round
__device__ bool sx_next(const SxArgs& a, int64_t s)
{
#pragma clang fp contract(off)
    const int N = a.nscan, P = a.P;
    const double* sim = a.sim + s * P * N;
    const double* fs = a.fsim + s * P;
    SxStart& st = a.starts[s];
    if (st.nit_cur >= a.maxiter) return false;
    bool conv = true;
    for (int e = N; e < P * N; ++e) { const double v = fabs(sim[e] - sim[e % N]); conv = conv && v <= a.xatol; }
    if (conv)
        for (int k = 1; k < P; ++k) { const double v = fabs(fs[0] - fs[k]); conv = conv && v <= a.fatol; }
    if (conv) return false;
    double* pts = a.pts + s * a.Q * N;
    const double* c = a.coef;
    const double* worst = sim + N * N;
    for (int d = 0; d < N; ++d) {
        double xb = sim[d];                                  // np.add.reduce(sim[:-1], 0): rows one after another
        for (int k = 1; k < N; ++k) xb = xb + sim[k * N + d];
        xb = xb / (double)N;
        const double w = worst[d];
        pts[0 * N + d] = sx_clip(c[0] * xb - c[1] * w);       // xr = (1 + rho) xbar - rho sim[-1]
        pts[1 * N + d] = sx_clip(c[2] * xb - c[3] * w);       // xe = (1 + rho chi) xbar - rho chi sim[-1]
        pts[2 * N + d] = sx_clip(c[4] * xb - c[5] * w);       // xc = (1 + psi rho) xbar - psi rho sim[-1]
        pts[3 * N + d] = sx_clip(c[6] * xb + c[7] * w);       // xcc = (1 - psi) xbar + psi sim[-1]
    }
    st.phase = PH_ITER;
    st.npend = 4;
    return true;
}

// the end of one minimize call: restart from its best vertex, or done
__device__ void sx_finish(const SxArgs& a, int r, int64_t s)
{
    SxStart& st = a.starts[s];
    const double f = a.fsim[s * a.P];
    st.nit += st.nit_cur;
    st.calls += 1;
    bool again = st.calls <= a.restarts;
    if (st.calls > 1) again = again && !(st.fprev - f <= a.fatol);
    st.fprev = f;
    if (again) {
        sx_begin(a, s, a.sim + s * a.P * a.nscan);             // x0 = res.x, the best vertex (sx_begin reads it in place)
    } else {
        st.done = 1;
        st.npend = 0;
        atomicSub(&a.runs[r].active, 1);
    }
}

// one thread per start: the values of the round just evaluated are committed as scipy's sequential algorithm would have
__global__ __launch_bounds__(SX_STEP_BLOCK) void k_sx_step(const SxArgs a)
{
#pragma clang fp contract(off)
    __shared__ int sind[SX_STEP_BLOCK][GF_MAX_DIM + 1];
    __shared__ double sfo[SX_STEP_BLOCK][GF_MAX_DIM + 1];
    const int r = blockIdx.y;
    const int j = blockIdx.x * SX_STEP_BLOCK + threadIdx.x;
    if (j >= a.S) return;
    const int64_t s = (int64_t)r * a.S + j;
    SxStart& st = a.starts[s];
    if (st.done) return;
    if (a.runs[r].failed) { st.done = 1; st.npend = 0; atomicSub(&a.runs[r].active, 1); return; }
    const int N = a.nscan, P = a.P;
    double* sim = a.sim + s * P * N;
    double* fs = a.fsim + s * P;
    const int Q = a.Q;
    const double* pts = a.pts + s * Q * N;
    const double* lq = a.lnq + s * Q;
    const int32_t* ps = a.pst + s * Q;
    st.devals += st.npend;
    bool ok = true;
    if (st.phase == PH_INIT) {
        for (int k = 0; k < P && ok; ++k) { ok = sx_use(a, r, ps[k]); fs[k] = sx_f(lq[k], ps[k]); }
        st.nfev += P;
        st.nit_cur = 1;
    } else if (st.phase == PH_SHRINK) {
        for (int k = 1; k < P && ok; ++k) { ok = sx_use(a, r, ps[k - 1]); fs[k] = sx_f(lq[k - 1], ps[k - 1]); }
        st.nfev += N;
        st.nit_cur += 1;
    } else {
        int take = -1;                                       // candidate that replaces sim[-1]; -1: shrink
        ok = sx_use(a, r, ps[0]);
        st.nfev += 1;
        const double fxr = sx_f(lq[0], ps[0]);
        if (ok) {
            if (fxr < fs[0]) {
                ok = sx_use(a, r, ps[1]);
                st.nfev += 1;
                const double fxe = sx_f(lq[1], ps[1]);
                take = fxe < fxr ? 1 : 0;
            } else if (fxr < fs[N - 1]) {
                take = 0;
            } else if (fxr < fs[N]) {
                ok = sx_use(a, r, ps[2]);
                st.nfev += 1;
                take = sx_f(lq[2], ps[2]) <= fxr ? 2 : -1;
            } else {
                ok = sx_use(a, r, ps[3]);
                st.nfev += 1;
                take = sx_f(lq[3], ps[3]) < fs[N] ? 3 : -1;
            }
        }
        if (ok && take >= 0) {
            for (int d = 0; d < N; ++d) sim[N * N + d] = pts[take * N + d];
            fs[N] = sx_f(lq[take], ps[take]);
            st.nit_cur += 1;
        } else if (ok) {
            // shrink towards sim[0], clipped vertex by vertex; the next round evaluates the n new vertices
            double* np_ = a.pts + s * Q * N;
            const double sigma = a.coef[8];
            for (int k = 1; k < P; ++k)
                for (int d = 0; d < N; ++d) {
                    const double v = sx_clip(sim[d] + sigma * (sim[k * N + d] - sim[d]));
                    sim[k * N + d] = v;
                    np_[(k - 1) * N + d] = v;
                }
            st.phase = PH_SHRINK;
            st.npend = N;
            return;
        }
    }
    if (!ok) { st.done = 1; st.npend = 0; atomicSub(&a.runs[r].active, 1); return; }
    sx_sort(a, s, sind[threadIdx.x], sfo[threadIdx.x]);
    if (!sx_next(a, s)) sx_finish(a, r, s);
}

hipError_t launch_eval_any(int mode, int lpw, const SxArgs& a, hipStream_t st)
{
    return launch_mode_lpw(mode, lpw, [&](auto m, auto l) {
        return launch_points(k_sx_eval<decltype(m)::value, decltype(l)::value>, a, l, (int64_t)a.S * a.Q, st);
    });
}

}  // namespace

struct gf_simplex {
    GfCubeRunsHost rs;
    int64_t rounds = 0;                 // evaluation rounds launched
    SxArgs a = {};
    GfSettleArgs sa = {};
    double* d_ustart = nullptr;
    int32_t* d_counts = nullptr;        // gf_toys_set_start_counts: [nruns], NULL: every run keeps all of the caller's starts
};

namespace {

// scipy's coefficients (_minimize_neldermead: dim = float(len(x0))) and the scalars of its candidate expressions
void sx_coefficients(int n, int adaptive, double coef[9])
{
    double rho, chi, psi, sigma;
    if (adaptive) {
        const double dim = (double)n;
        rho = 1.0; chi = 1.0 + 2.0 / dim; psi = 0.75 - 1.0 / (2.0 * dim); sigma = 1.0 - 1.0 / dim;
    } else {
        rho = 1.0; chi = 2.0; psi = 0.5; sigma = 0.5;
    }
    coef[0] = 1.0 + rho; coef[1] = rho;
    coef[2] = 1.0 + rho * chi; coef[3] = rho * chi;
    coef[4] = 1.0 + psi * rho; coef[5] = psi * rho;
    coef[6] = 1.0 - psi; coef[7] = psi;
    coef[8] = sigma;
}

int sx_init(gf_simplex* s)
{
    SxArgs& a = s->a;
    if (a.nseed > 0) {
        const int rc = cube_runs_draw(s->rs, a, SX_SEED_ITER, a.nseed, a.seed_u, a.theta, a.seed_l, a.seed_st);
        if (rc != GF_OK) return rc;
    }
    hipLaunchKernelGGL(k_sx_pick, dim3(a.nruns), dim3(SX_PICK_BLOCK), 0, s->rs.set.stream, a);
    GF_HIP(hipGetLastError());
    if (s->d_counts) {
        hipLaunchKernelGGL(k_sx_trim, dim3(a.nruns), dim3(SX_PICK_BLOCK), 0, s->rs.set.stream, a, s->d_counts);
        GF_HIP(hipGetLastError());
    }
    s->rs.initialised = 1;
    return GF_OK;
}
}  // namespace

extern "C" {

int gf_simplex_create(gf_model* const* models, int nruns, int nscan, const int32_t* cols, const double* bases, int nstarts,
                      int nseed, uint64_t seed, int on_nonunitary, gf_simplex** out)
{
    if (!models || !cols || !bases || !out || nruns < 1 || nruns > 65535 || nscan < 1 || nscan > GF_MAX_DIM || nstarts < 0 ||
        nseed < 0 || nstarts > nseed || nstarts > 4096 || nseed > (1 << 22) || (on_nonunitary != 0 && on_nonunitary != 1))
        return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_simplex* s = new (std::nothrow) gf_simplex();
    if (!s) return GF_ERR_ALLOC;
    SxArgs& a = s->a;
    const int rc = cube_runs_create(s->rs, a, models, nruns, nscan, cols, bases, seed, "gf_simplex_create");
    if (rc != GF_OK) { delete s; return rc; }
    a.nstarts = nstarts; a.nuser = 0; a.nseed = nseed; a.raise = on_nonunitary == 0;
    a.xatol = 1e-4; a.fatol = 1e-4; a.maxiter = 200 * nscan; a.restarts = 0;
    sx_coefficients(nscan, 0, a.coef);
    a.S = nstarts; a.P = nscan + 1; a.Q = nscan + 1 > 4 ? nscan + 1 : 4;
    const size_t R = nruns, M = nseed;
    hipError_t e = hipSuccess;
    auto al = [&](void** p, size_t bytes) { if (e == hipSuccess && bytes > 0) e = hipMalloc(p, bytes); };
    al((void**)&a.runs, sizeof(SxRun) * R);
    al((void**)&a.seed_u, sizeof(double) * R * M * nscan);
    al((void**)&a.seed_l, sizeof(double) * R * M);
    al((void**)&a.seed_st, sizeof(int32_t) * R * M);
    al((void**)&a.theta, sizeof(double) * R * M * a.ndim);
    if (e == hipSuccess) e = hipMemsetAsync(a.runs, 0, sizeof(SxRun) * R, s->rs.set.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->rs.set.stream);
    if (e != hipSuccess) { const int rc2 = gf_hip_fail(e, "gf_simplex_create"); gf_simplex_destroy(s); return rc2; }
    *out = s;
    return GF_OK;
}

int gf_simplex_set_run_ids(gf_simplex* s, const uint64_t* ids)
{
    if (!s || !ids) return GF_ERR_INVALID_ARG;
    return cube_runs_set_ids(s->rs, s->a, ids, "gf_simplex_set_run_ids: before the first gf_simplex_run");
}

int gf_simplex_set_starts(gf_simplex* s, int nuser, const double* cube)
{
    if (!s || nuser < 0 || nuser > 4096 || (nuser > 0 && !cube)) return GF_ERR_INVALID_ARG;
    if (s->rs.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_simplex_set_starts: before the first gf_simplex_run");
    const size_t n = (size_t)s->a.nruns * nuser * s->a.nscan;
    for (size_t i = 0; i < n; ++i)
        if (!(cube[i] == cube[i])) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_simplex_set_starts: NaN in a start");
    GF_HIP(hipSetDevice(s->rs.set.device));
    if (s->d_ustart) { (void)hipFree(s->d_ustart); s->d_ustart = nullptr; }
    if (n > 0) {
        GF_HIP(hipMalloc((void**)&s->d_ustart, sizeof(double) * n));
        GF_HIP(hipMemcpyAsync(s->d_ustart, cube, sizeof(double) * n, hipMemcpyHostToDevice, s->rs.set.stream));
        GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    }
    s->a.ustart = s->d_ustart;
    s->a.nuser = nuser;
    return GF_OK;
}

int gf_toys_set_measurements(gf_simplex* s, const double* bf, const double* smearing)
{
    if (!s || !bf || !smearing) return GF_ERR_INVALID_ARG;
    // the set's own seeding goes through the models' bulk path (cube_runs_draw): it would score under the models' measurement
    if (s->rs.set.kind == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_set_measurements: the runs' models carry a tabulated likelihood, which has no Gaussian measurement to replace");
    if (s->a.nseed > 0)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_set_measurements: the set draws %d seed points per run, which its models would score; "
                           "give the starts (nseed = 0, gf_simplex_set_starts)", s->a.nseed);
    return cube_runs_set_measurements(s->rs, s->a, bf, smearing, "gf_toys_set_measurements");
}

int gf_toys_set_binned_measurements(gf_simplex* s, int nbins, const double* fr_bins, const double* sigma)
{
    if (!s || !fr_bins || !sigma) return GF_ERR_INVALID_ARG;
    if (s->rs.set.kind == GF_LLH_TABLE)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_toys_set_binned_measurements: the runs' models carry a tabulated likelihood, which has no binned measurement to replace");
    // as gf_toys_set_measurements: the set's own seeding would score under the models' measurement
    if (s->a.nseed > 0)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_set_binned_measurements: the set draws %d seed points per run, which its models would score; "
                           "give the starts (nseed = 0, gf_simplex_set_starts)", s->a.nseed);
    return cube_runs_set_binned_measurements(s->rs, s->a, nbins, fr_bins, sigma, "gf_toys_set_binned_measurements");
}

int gf_toys_set_start_counts(gf_simplex* s, const int32_t* counts)
{
    if (!s || !counts) return GF_ERR_INVALID_ARG;
    if (s->rs.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_set_start_counts: before the first run");
    if (s->a.nstarts != 0)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_set_start_counts: the set picks %d starts of its own per run; the counts are of the caller's starts alone", s->a.nstarts);
    for (int r = 0; r < s->a.nruns; ++r)
        if (counts[r] < 0 || counts[r] > s->a.nuser)
            return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_toys_set_start_counts: run %d keeps %d of %d starts", r, counts[r], s->a.nuser);
    GF_HIP(hipSetDevice(s->rs.set.device));
    if (!s->d_counts) GF_HIP(hipMalloc((void**)&s->d_counts, sizeof(int32_t) * (size_t)s->a.nruns));
    GF_HIP(hipMemcpyAsync(s->d_counts, counts, sizeof(int32_t) * (size_t)s->a.nruns, hipMemcpyHostToDevice, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    return GF_OK;
}

int gf_simplex_set_options(gf_simplex* s, double xatol, double fatol, int maxiter, int adaptive, int restarts)
{
    if (!s || !(xatol >= 0.0) || !(fatol >= 0.0) || maxiter < 1 || (adaptive != 0 && adaptive != 1) || restarts < 0)
        return GF_ERR_INVALID_ARG;
    if (s->rs.initialised) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_simplex_set_options: before the first gf_simplex_run");
    SxArgs& a = s->a;
    a.xatol = xatol; a.fatol = fatol; a.maxiter = maxiter; a.restarts = restarts;
    sx_coefficients(a.nscan, adaptive, a.coef);
    return GF_OK;
}

void gf_simplex_destroy(gf_simplex* s)
{
    if (!s) return;
    SxArgs& a = s->a;
    cube_runs_free(s->rs, a);
    void* ptrs[] = {s->d_ustart, s->d_counts, a.runs, a.starts, a.sim, a.fsim, a.tmp, a.pts, a.lnq, a.pst, a.seed_u, a.seed_l, a.seed_st, a.theta};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete s;
}

// Rounds until every start of every run is done; the per-run counts of live starts are read back every `check` rounds.
int gf_simplex_run(gf_simplex* s, int64_t max_rounds)
{
    if (!s || max_rounds < 1) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    SxArgs& a = s->a;
    if (const int rc = cube_runs_begin(s->rs, "gf_simplex_run")) return rc;
    if (!s->rs.initialised) {
        // the per-start buffers are sized once the caller's starts are known
        a.S = a.nstarts + a.nuser;
        // simplex rows: P per start; rows of a round (points, values, statuses, parked candidates): Q = max(P, 4) per start
        const size_t R = a.nruns, S = a.S > 0 ? a.S : 1, N = a.nscan, WP = R * S * a.P, W = R * S * a.Q;
        hipError_t e = hipSuccess;
        auto al = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
        al((void**)&a.starts, sizeof(SxStart) * R * S);
        al((void**)&a.sim, sizeof(double) * WP * N);
        al((void**)&a.fsim, sizeof(double) * WP);
        al((void**)&a.tmp, sizeof(double) * WP * N);
        al((void**)&a.pts, sizeof(double) * W * N);
        al((void**)&a.lnq, sizeof(double) * W);
        al((void**)&a.pst, sizeof(int32_t) * W);
        if (e == hipSuccess) e = hipMemsetAsync(a.starts, 0, sizeof(SxStart) * R * S, s->rs.set.stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.pst, 0, sizeof(int32_t) * W, s->rs.set.stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.lnq, 0, sizeof(double) * W, s->rs.set.stream);
        if (e == hipSuccess) e = cube_runs_alloc_queue(s->rs, a, W);
        if (e != hipSuccess) return gf_hip_fail(e, "gf_simplex_run: buffers");
        GfSettleArgs& sa = s->sa;
        cube_runs_settle_args(s->rs, a, (int32_t)(2 * S * a.Q), sa);
        sa.flags = nullptr; sa.sx_lnq = a.lnq; sa.sx_status = a.pst;
        const int rc = sx_init(s);
        if (rc != GF_OK) return rc;
    }
    if (a.S == 0) return GF_OK;
    const int lpw = lanes_per_walker(gf_modelset_eval_mode(&s->rs.set), (int64_t)a.nruns * a.S * a.Q, a.nbins_max, s->rs.set.cus, {false, 32 * 1024, "GF_SIMPLEX_LPW"});
    constexpr int check = 4;
    std::vector<SxRun> hr(a.nruns);
    const dim3 sgrid((unsigned)((a.S + SX_STEP_BLOCK - 1) / SX_STEP_BLOCK), a.nruns);
    int64_t done_here = 0;
    for (;;) {
        GF_HIP(hipMemcpyAsync(hr.data(), a.runs, sizeof(SxRun) * a.nruns, hipMemcpyDeviceToHost, s->rs.set.stream));
        GF_HIP(hipStreamSynchronize(s->rs.set.stream));
        bool all = true;
        for (const SxRun& x : hr) all = all && (x.active == 0 || x.failed);
        if (all) break;
        if (done_here >= max_rounds) return GF_OK;                      // stepping: the caller asked for this many rounds
        for (int i = 0; i < check && done_here < max_rounds; ++i, ++done_here) {
            GF_HIP(launch_eval_any(gf_modelset_eval_mode(&s->rs.set), lpw, a, s->rs.set.stream));
            if (s->rs.set.mode == MODE_BSM_GAUSS) GF_HIP(gf_launch_simplex_settle(s->sa, s->rs.set.cus, s->rs.set.stream));
            hipLaunchKernelGGL(k_sx_step, sgrid, dim3(SX_STEP_BLOCK), 0, s->rs.set.stream, a);
            GF_HIP(hipGetLastError());
            s->rounds += 1;
        }
    }
    return GF_OK;
}

int gf_simplex_result(gf_simplex* s, double* max_lnl, double* argmax_cube, int32_t* nstarts, int64_t* niter, int64_t* nfev,
                      int64_t* nevals, uint32_t* nonunitary, uint32_t* parked, int32_t* failed)
{
    if (!s) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    const SxArgs& a = s->a;
    const int R = a.nruns, S = a.S, P = a.P, N = a.nscan;
    std::vector<SxRun> hr(R);
    GF_HIP(hipMemcpyAsync(hr.data(), a.runs, sizeof(SxRun) * R, hipMemcpyDeviceToHost, s->rs.set.stream));
    std::vector<SxStart> hs((size_t)R * S);
    std::vector<double> f((size_t)R * S * P), x((size_t)R * S * P * N);
    if (s->rs.initialised && S > 0) {
        GF_HIP(hipMemcpyAsync(hs.data(), a.starts, sizeof(SxStart) * hs.size(), hipMemcpyDeviceToHost, s->rs.set.stream));
        GF_HIP(hipMemcpyAsync(f.data(), a.fsim, sizeof(double) * f.size(), hipMemcpyDeviceToHost, s->rs.set.stream));
        GF_HIP(hipMemcpyAsync(x.data(), a.sim, sizeof(double) * x.size(), hipMemcpyDeviceToHost, s->rs.set.stream));
    }
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    for (int r = 0; r < R; ++r) {
        const int used = s->rs.initialised ? hr[r].nstarts : 0;
        double best = HUGE_VAL;
        int bj = -1;
        int64_t it = 0, fe = 0, ev = 0;
        for (int j = 0; j < used; ++j) {
            const size_t k = (size_t)r * S + j;
            it += hs[k].nit; fe += hs[k].nfev; ev += hs[k].devals;
            const double fj = f[k * P];
            if (hs[k].calls > 0 && (bj < 0 || fj < best)) { best = fj; bj = j; }
        }
        if (max_lnl) max_lnl[r] = bj >= 0 ? -best : -HUGE_VAL;
        if (argmax_cube)
            for (int d = 0; d < N; ++d) argmax_cube[(size_t)r * N + d] = bj >= 0 ? x[((size_t)r * S + bj) * P * N + d] : NAN;
        if (nstarts) nstarts[r] = used;
        if (niter) niter[r] = it;
        if (nfev) nfev[r] = fe;
        if (nevals) nevals[r] = ev + (int64_t)a.nseed;
        if (nonunitary) nonunitary[r] = hr[r].nonunit;
        if (parked) parked[r] = hr[r].parked;
        if (failed) failed[r] = hr[r].failed;
    }
    return GF_OK;
}

int gf_simplex_get_starts(gf_simplex* s, int run, double* fun, double* cube, int32_t* nit, int64_t* nfev)
{
    if (!s || run < 0 || run >= s->a.nruns) return GF_ERR_INVALID_ARG;
    GF_HIP(hipSetDevice(s->rs.set.device));
    const SxArgs& a = s->a;
    const int S = a.S, P = a.P, N = a.nscan;
    if (!s->rs.initialised || S == 0) return GF_OK;
    std::vector<SxStart> hs(S);
    std::vector<double> f((size_t)S * P), x((size_t)S * P * N);
    GF_HIP(hipMemcpyAsync(hs.data(), a.starts + (size_t)run * S, sizeof(SxStart) * S, hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipMemcpyAsync(f.data(), a.fsim + (size_t)run * S * P, sizeof(double) * f.size(), hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipMemcpyAsync(x.data(), a.sim + (size_t)run * S * P * N, sizeof(double) * x.size(), hipMemcpyDeviceToHost, s->rs.set.stream));
    GF_HIP(hipStreamSynchronize(s->rs.set.stream));
    for (int j = 0; j < S; ++j) {
        if (fun) fun[j] = hs[j].calls > 0 ? f[(size_t)j * P] : HUGE_VAL;
        if (cube) for (int d = 0; d < N; ++d) cube[(size_t)j * N + d] = x[(size_t)j * P * N + d];
        if (nit) nit[j] = hs[j].nit + (hs[j].done ? 0 : hs[j].nit_cur);
        if (nfev) nfev[j] = hs[j].nfev;
    }
    return GF_OK;
}

}  // extern "C"
