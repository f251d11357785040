// gf_ns_toys.hip -- the evidence of every run of a nested sampler (gf_nested.hip) under the realisations of an ensemble of Gaussian
// measurements, from the points the runs keep: Z_t = sum_i dX_i L_t(theta_i) = sum_i exp(lnw_i + l_t(fr_i) -
// l_0(fr_i)).  The priors cancel and the composition fr_i of a point does not depend on the measurement, so the runs' points are
// gathered (k_np_gather through gf_internal_nested_gather) and propagated under their runs' models once; what is left per (point,
// realisation) is a Gaussian and an exp.  The arithmetic and the order of every sum are gf_ns_toys.hpp's.
//   k_nt_leaf<NT_MAX>   a workgroup per (leaf of 4096 points, run, tile of NT_TILE realisations): lane l keeps its 16 points l, l + 256,
//                       ... in registers (composition, base log-weight, the Gaussian of the run's own measurement) and loops over the
//                       tile's realisations, whose constants are uniform (scalar loads): the leaf's max of x
//   k_nt_run_max        a lane per (run, realisation): the max over the run's leaves (exact in any order)
//   k_nt_leaf<NT_SUM>   the same walk at that max: the leaf's S, S2 and kept -- the lane's points in order, the wave's fold by
//                       shuffles, lane 0 of every wave puts its group sum into LDS, and after the tile's loop lane q adds realisation
//                       q's four group sums in order: no barrier inside the loop
//   k_nt_run            a workgroup per (run, realisation): the leaves summed as gf_nested_post.hpp's tree sums them, and the ESS
// No atomics.  Nothing depends on the tile, on the grid or on the runs that share the launch.  The realisations are cut into batches
// so that the partials [run][leaf][realisation] stay under GF_NS_TOYS_SCRATCH_DEFAULT (GF_NS_TOYS_SCRATCH_BYTES overrides: the
// batching changes, no result does).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "gf_devcache.h"
#include "gf_host.h"
#include "gf_device.hpp"
#include "gf_ns_toys.hpp"
#include "gf_weights.h"

#define GF_NS_TOYS_SCRATCH_DEFAULT ((size_t)256 << 20)

namespace {
using namespace gfnt;
using gfnp::LANES;
using gfnp::LEAF;

constexpr int NT_BLOCK = LANES;
constexpr int NT_PER_LANE = LEAF / LANES;       // 16 points of a leaf per lane
constexpr int NT_TILE = 64;                     // realisations per workgroup of k_nt_leaf
constexpr int NT_MAX_TOYS = 1 << 24;
enum { NT_MAX = 0, NT_SUM = 1 };
enum { NT_M = 0, NT_S = 1, NT_S2 = 2, NT_ESS = 3, NT_OUT = 4 };
static_assert(gfrw::STATUS_NON_UNITARY == GF_ST_NON_UNITARY && LEAF == GF_WEIGHT_LEAF, "the headers state the public status and the leaf");

struct DevLogOfExp {
    __device__ __forceinline__ double operator()(double x) const { return gfdev::log_of_exp(x); }
};

struct NtArgs {
    const GfWeightRun* runs;            // [R]
    const GfCommon* commons;            // [R]: the runs' own measurements and offsets
    const double* lnw;                  // compact, a run's at its off
    const double* fr;                   // [total][3], as lnw
    const int32_t* st;                  // [total]
    const Consts* meas;                 // realisation t of run r at r * meas_stride + t; meas_stride = 0: shared by the runs
    int64_t meas_stride;
    int32_t t0, T;                      // this launch: the realisations t0 .. t0 + T - 1 of ntoys
    int32_t ntoys;
    int64_t maxleaves;
    double* part_m;                     // [R][maxleaves][T]
    double* part_s;                     // [R][maxleaves][T][2]: S, S2
    int32_t* part_k;                    // [R][maxleaves][T]
    double* run_m;                      // [R][T]
    double* out;                        // [R][ntoys][NT_OUT]
    int64_t* out_k;                     // [R][ntoys]
};

// the fold of a wave's 64 lane values (gf_nested_post.hpp fold_lanes, one group); the result is lane 0's
__device__ __forceinline__ double nt_wave_sum(double s)
{
    for (int o = 32; o > 0; o >>= 1) s = gfnp::add(s, __shfl_down(s, o));
    return s;
}
__device__ __forceinline__ double nt_wave_max(double s)
{
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_down(s, o); s = t > s ? t : s; }
    return s;
}
__device__ __forceinline__ int nt_wave_count(int s)
{
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    return s;
}

// grid (maxleaves, R, tiles of the launch's realisations)
template <int PASS>
__global__ __launch_bounds__(NT_BLOCK) void k_nt_leaf(const NtArgs a)
{
    __shared__ double sm[2][NT_TILE][4];                              // a realisation's four group sums: S, S2 (NT_MAX: the maxima)
    __shared__ int32_t smk[NT_TILE][4];
    const int r = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int64_t leaf = blockIdx.x;
    const GfWeightRun R = a.runs[r];
    if (leaf * LEAF >= R.n) return;                                   // uniform
    const int q0 = blockIdx.z * NT_TILE;
    const int nq = a.T - q0 < NT_TILE ? a.T - q0 : NT_TILE;
    const GfCommon& c = a.commons[r];
    const Consts own = {{c.bf[0], c.bf[1], c.bf[2]}, c.gauss_mh, c.gauss_k};
    const double offset = c.offset;
    // the lane's points: j < cnt are the run's
    double f0[NT_PER_LANE], f1[NT_PER_LANE], f2[NT_PER_LANE], bl[NT_PER_LANE], l0[NT_PER_LANE];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < NT_PER_LANE; ++j) {
        const int64_t i = leaf * LEAF + j * NT_BLOCK + tid;
        f0[j] = f1[j] = f2[j] = l0[j] = 0.0;
        bl[j] = gfrw::neg_inf();
        if (i < R.n) {
            const int64_t g = R.off + i;
            f0[j] = a.fr[3 * g]; f1[j] = a.fr[3 * g + 1]; f2[j] = a.fr[3 * g + 2];
            l0[j] = gauss(own, offset, f0[j], f1[j], f2[j], DevLogOfExp());
            bl[j] = base_lnw(a.lnw[g], l0[j], a.st[g]);
            cnt = j + 1;
        }
    }
    const Consts* meas = a.meas + (int64_t)r * a.meas_stride + a.t0 + q0;
    for (int q = 0; q < nq; ++q) {                                    // uniform: the constants come by scalar loads
        const Consts g = meas[q];
        if constexpr (PASS == NT_MAX) {
            double mx = gfrw::neg_inf();
#pragma unroll
            for (int j = 0; j < NT_PER_LANE; ++j) {
                const double x = x_term(bl[j], l0[j], gauss(g, offset, f0[j], f1[j], f2[j], DevLogOfExp()));
                if (j < cnt) mx = x > mx ? x : mx;
            }
            mx = nt_wave_max(mx);
            if ((tid & 63) == 0) sm[0][q][wave] = mx;
        } else {
            const double M = a.run_m[(int64_t)r * a.T + q0 + q];
            double s = 0.0, s2 = 0.0;
            int k = 0;
#pragma unroll
            for (int j = 0; j < NT_PER_LANE; ++j) {
                const double x = x_term(bl[j], l0[j], gauss(g, offset, f0[j], f1[j], f2[j], DevLogOfExp()));
                const double e = gfnp::weight(x, M);
                if (j < cnt) {
                    s = gfnp::add(s, e);
                    s2 = gfnp::add(s2, gfnp::square(e));
                    k += kept(x);
                }
            }
            s = nt_wave_sum(s);
            s2 = nt_wave_sum(s2);
            k = nt_wave_count(k);
            if ((tid & 63) == 0) { sm[0][q][wave] = s; sm[1][q][wave] = s2; smk[q][wave] = k; }
        }
    }
    __syncthreads();
    if (tid >= nq) return;
    const int64_t at = ((int64_t)r * a.maxleaves + leaf) * a.T + q0 + tid;
    if constexpr (PASS == NT_MAX) {
        const double p = sm[0][tid][0] > sm[0][tid][1] ? sm[0][tid][0] : sm[0][tid][1];
        const double q = sm[0][tid][2] > sm[0][tid][3] ? sm[0][tid][2] : sm[0][tid][3];
        a.part_m[at] = p > q ? p : q;
    } else {
        a.part_s[2 * at] = gfnp::add(gfnp::add(gfnp::add(sm[0][tid][0], sm[0][tid][1]), sm[0][tid][2]), sm[0][tid][3]);
        a.part_s[2 * at + 1] = gfnp::add(gfnp::add(gfnp::add(sm[1][tid][0], sm[1][tid][1]), sm[1][tid][2]), sm[1][tid][3]);
        a.part_k[at] = smk[tid][0] + smk[tid][1] + smk[tid][2] + smk[tid][3];
    }
}

// grid (ceil(T / 256), R): run_m [R][T]
__global__ __launch_bounds__(NT_BLOCK) void k_nt_run_max(const NtArgs a)
{
    const int r = blockIdx.y;
    const int t = blockIdx.x * NT_BLOCK + threadIdx.x;
    if (t >= a.T) return;
    const int64_t leaves = (a.runs[r].n + LEAF - 1) / LEAF;
    double m = gfrw::neg_inf();
    for (int64_t l = 0; l < leaves; ++l) {
        const double v = a.part_m[((int64_t)r * a.maxleaves + l) * a.T + t];
        m = v > m ? v : m;
    }
    a.run_m[(int64_t)r * a.T + t] = m;
}

// grid (T, R): the run's leaves summed (lane l takes the leaves l, l + 256, ... in order, then the fold), and what follows the sums
__global__ __launch_bounds__(NT_BLOCK) void k_nt_run(const NtArgs a)
{
    __shared__ double sm[2][4];
    __shared__ long long smk[4];
    const int r = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const GfWeightRun R = a.runs[r];
    double* out = a.out + ((int64_t)r * a.ntoys + a.t0 + t) * NT_OUT;
    int64_t* out_k = a.out_k + (int64_t)r * a.ntoys + a.t0 + t;
    if (R.n == 0) {                                                    // a run without points
        if (tid == 0) { out[NT_M] = out[NT_S] = out[NT_S2] = gfnp::nan(); out[NT_ESS] = 0.0; *out_k = 0; }
        return;
    }
    const int64_t leaves = (R.n + LEAF - 1) / LEAF;
    double s = 0.0, s2 = 0.0;
    long long k = 0;
    for (int64_t l = tid; l < leaves; l += NT_BLOCK) {
        const int64_t at = ((int64_t)r * a.maxleaves + l) * a.T + t;
        s = gfnp::add(s, a.part_s[2 * at]);
        s2 = gfnp::add(s2, a.part_s[2 * at + 1]);
        k += a.part_k[at];
    }
    s = nt_wave_sum(s);
    s2 = nt_wave_sum(s2);
    for (int o = 32; o > 0; o >>= 1) k += __shfl_down(k, o);
    if ((tid & 63) == 0) { sm[0][tid >> 6] = s; sm[1][tid >> 6] = s2; smk[tid >> 6] = k; }
    __syncthreads();
    if (tid != 0) return;
    const double S = gfnp::add(gfnp::add(gfnp::add(sm[0][0], sm[0][1]), sm[0][2]), sm[0][3]);
    const double S2 = gfnp::add(gfnp::add(gfnp::add(sm[1][0], sm[1][1]), sm[1][2]), sm[1][3]);
    const int64_t K = smk[0] + smk[1] + smk[2] + smk[3];
    out[NT_M] = a.run_m[(int64_t)r * a.T + t];
    out[NT_S] = S;
    out[NT_S2] = S2;
    out[NT_ESS] = ess(S, S2, K);
    *out_k = K;
}

size_t nt_scratch_cap()
{
    const char* v = gf_internal_env("GF_NS_TOYS_SCRATCH_BYTES", 0);
    if (v) {
        const long long b = std::atoll(v);
        if (b > 0) return (size_t)b;
    }
    return (size_t)GF_NS_TOYS_SCRATCH_DEFAULT;
}

// the realisations' constants on the host: [n] from bf [n][3] and smearing[k % ntoys]
int nt_measurements(const double* bf, const double* smearing, size_t n, size_t ntoys, std::vector<Consts>& out, const char* who)
{
    out.resize(n);
    int rc = GF_OK;
    for (size_t k = 0; k < n && rc == GF_OK; ++k) rc = gf_gauss_realisation(bf + 3 * k, smearing[k % ntoys], k % ntoys, who, out[k].m, &out[k].mh, &out[k].k);
    return rc;
}

}  // namespace

extern "C" {

int gf_nested_toys_evidence(gf_nested* s, const double* bf, const double* smearing, int ntoys, int per_run, double* m, double* sum, double* sum2,
                            double* ess_out, int64_t* kept_out)
{
    const char* who = "gf_nested_toys_evidence";
    if (!s || !bf || !smearing || ntoys < 1 || ntoys > NT_MAX_TOYS || (per_run != 0 && per_run != 1)) return GF_ERR_INVALID_ARG;
    GfNestedView v;
    int rc = gf_internal_nested_view(s, &v, nullptr);
    if (rc != GF_OK) return rc;
    const int R = v.nruns, T = ntoys;
    int binned = 0;
    for (int r = 0; r < R; ++r) {
        const GfCommon* c; const GfBsm* tb; const double* pt; const double* bt; int device, cus, nb;
        if (gf_model_constants(v.models[r], &c, &tb, &pt, &device, &cus, &nb) != GF_OK) return GF_ERR_INVALID_ARG;
        binned += gf_model_binned(v.models[r], &bt);
        if (gf_model_table(v.models[r], nullptr) > 0)
            return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry a tabulated likelihood; a realisation of a table is not defined", who);
        if (c->mode != GF_MODE_SM_GAUSS && c->mode != GF_MODE_BSM_GAUSS)
            return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the models have no Gaussian measurement (mode %d)", who, c->mode);
    }
    if (binned)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: the runs' models carry a binned measurement; a realisation replaces the flux-averaged one only", who);
    std::vector<Consts> hm;
    rc = nt_measurements(bf, smearing, (size_t)(per_run ? R : 1) * T, (size_t)T, hm, who);
    if (rc != GF_OK) return rc;

    GF_HIP(hipSetDevice(v.device));
    std::vector<GfWeightRun> runs(R);
    int64_t total = 0, maxn = 0;
    rc = gf_internal_nested_runs(s, &v, runs.data(), &total, &maxn);
    if (rc != GF_OK) return rc;
    hipStream_t st = v.stream;
    NtArgs a = {};
    a.maxleaves = std::max<int64_t>(1, (maxn + LEAF - 1) / LEAF);
    if (a.maxleaves > 0x7fffffffll) return gf_fail_msg(GF_ERR_UNSUPPORTED, "%s: too many points per run", who);
    const size_t per_toy = (size_t)R * (size_t)a.maxleaves * (3 * sizeof(double) + sizeof(int32_t)) + (size_t)R * sizeof(double);
    // at most 65535 tiles of a launch (gridDim.z)
    const int Tb = (int)std::min<size_t>(std::min<size_t>((size_t)T, (size_t)65535 * NT_TILE), std::max<size_t>(1, nt_scratch_cap() / per_toy));
    const size_t N = (size_t)total, RL = (size_t)R * (size_t)a.maxleaves;

    GfScratch buf(GF_MEM_CACHED);
    GfWeightRun* d_runs = nullptr;
    double *d_lnw = nullptr, *d_theta = nullptr, *d_fr = nullptr;
    int32_t* d_st = nullptr;
    Consts* d_meas = nullptr;
    buf.take(&d_runs, sizeof(GfWeightRun) * R, who); buf.take(&d_lnw, sizeof(double) * N, who);       // sticky: checked once, below
    buf.take(&d_theta, sizeof(double) * N * v.ndim, who); buf.take(&d_fr, sizeof(double) * N * 3, who);
    buf.take(&d_st, sizeof(int32_t) * N, who); buf.take(&d_meas, sizeof(Consts) * hm.size(), who);
    buf.take(&a.part_m, sizeof(double) * RL * Tb, who); buf.take(&a.part_s, sizeof(double) * RL * Tb * 2, who);
    buf.take(&a.part_k, sizeof(int32_t) * RL * Tb, who); buf.take(&a.run_m, sizeof(double) * R * Tb, who);
    buf.take(&a.out, sizeof(double) * (size_t)R * T * NT_OUT, who); buf.take(&a.out_k, sizeof(int64_t) * (size_t)R * T, who);
    if (buf.failed != GF_OK) return buf.failed;
    a.runs = d_runs; a.commons = v.d_commons; a.lnw = d_lnw; a.fr = d_fr; a.st = d_st; a.meas = d_meas;
    a.meas_stride = per_run ? T : 0;
    a.ntoys = T;

    // from here on the stream is synchronised before the scratch and the host vectors go
    std::vector<double> h_out((size_t)R * T * NT_OUT);
    std::vector<int64_t> h_k((size_t)R * T);
    hipError_t e = hipMemcpyAsync(d_meas, hm.data(), sizeof(Consts) * hm.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        rc = gf_internal_nested_gather(&v, runs.data(), maxn, d_runs, d_lnw, d_theta);
        gf_internal_full_arbitration_grids(v.device, st, 1);             // the runs of a scan differ (gf_rowsets.h gf_propagate_sets)
        for (int r = 0; r < R && rc == GF_OK; ++r) {
            const GfWeightRun& q = runs[r];
            if (q.n > 0)
                rc = gf_model_propagate_on(v.models[r], st, d_theta + (size_t)q.toff * v.ndim, GF_LAYOUT_AOS, q.n, d_fr + (size_t)q.off * 3, d_st + q.off);
        }
        gf_internal_full_arbitration_grids(v.device, st, 0);
    }
    for (int t0 = 0; t0 < T && rc == GF_OK && e == hipSuccess; t0 += Tb) {
        a.t0 = t0;
        a.T = std::min(Tb, T - t0);
        const dim3 leaves((unsigned)a.maxleaves, (unsigned)R, (unsigned)((a.T + NT_TILE - 1) / NT_TILE));
        hipLaunchKernelGGL(k_nt_leaf<NT_MAX>, leaves, dim3(NT_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_nt_run_max, dim3((unsigned)((a.T + NT_BLOCK - 1) / NT_BLOCK), (unsigned)R), dim3(NT_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_nt_leaf<NT_SUM>, leaves, dim3(NT_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_nt_run, dim3((unsigned)a.T, (unsigned)R), dim3(NT_BLOCK), 0, st, a);
        e = hipGetLastError();
    }
    if (rc == GF_OK && e == hipSuccess) e = hipMemcpyAsync(h_out.data(), a.out, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, st);
    if (rc == GF_OK && e == hipSuccess) e = hipMemcpyAsync(h_k.data(), a.out_k, sizeof(int64_t) * h_k.size(), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (rc != GF_OK) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return gf_hip_fail(e != hipSuccess ? e : e2, who);
    rc = gf_internal_check_overflow(v.device, st);
    if (rc != GF_OK) return rc;
    for (size_t k = 0; k < (size_t)R * T; ++k) {
        const double* q = h_out.data() + k * NT_OUT;
        if (m) m[k] = q[NT_M];
        if (sum) sum[k] = q[NT_S];
        if (sum2) sum2[k] = q[NT_S2];
        if (ess_out) ess_out[k] = q[NT_ESS];
        if (kept_out) kept_out[k] = h_k[k];
    }
    return GF_OK;
}

}  // extern "C"
