// gf_sampler.hip -- device-resident affine-invariant ensemble sampler (the emcee step either side of
// the lnprob path).
//
// The reference drives the path through emcee's stretch move (un-vendored, requirements.txt:5; call
// sites golemflavor/mcmc.py:29-49).  Host-driven, every half-ensemble update costs a PCIe round trip and
// a launch for a few thousand evaluations.  Here the whole chain stays in HBM: one launch per
// half-ensemble update does proposal + lnprob + accept in place, for `nchains` independent ensembles
// stacked in one grid; the host only sees chains at the end.
//
// Stretch move (Goodman & Weare 2010, the published algorithm emcee runs by default), for walker k of
// the active half S with the complementary half C frozen during the launch:
//     z = ((a-1) u1 + 1)^2 / a,   j ~ U{0..|C|-1},   q = c_j - z (c_j - s_k),
//     accept iff (ndim-1) ln z + lnp(q) - lnp(s_k) > ln u3.
// Random numbers: one Philox4x32-10 block per (walker, half-step): counter = (global walker slot,
// 2*iteration + half), key = seed.  u1 has 53 bits, j and u3 32 bits each.  The accept test is evaluated
// as ln(z^(ndim-1) / u3) > lnp(s_k) - lnp(q): one logarithm.
//
// This file is the DEVICE side: the kernels, their device helpers and, at the end, the launchers that pick an instance
// (gf_sampler_launch.h).  gf_sampler, its runs and the C ABI are gf_sampler_host.hip's; nothing of the host's state is seen here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_internal.h"                // gf_internal_env, gf_launch_walker_mean
#include "gf_sampler_launch.h"          // StretchArgs, PersistArgs, ChainArgs and the launchers this file defines for gf_sampler_host.hip
#include "gf_device.hpp"
#include "gf_bsm_device.hpp"
#include "gf_launch.h"
#include "gf_unitarity_teams.hpp"      // Team9: the reference's unitarity chain on nine lanes (k_stretch_chain settles its own parked proposals)
#include "gf_propose.hpp"               // proposal_lnprob, park_proposal, lanes_per_walker: shared with the nested sampler (gf_nested.hip) and the maximiser
#include "gf_stretch.hpp"               // the move itself: draw, accept test's left side, row -- one definition for the launch shapes below

namespace {
using namespace gfdev;

// start positions the reference would have died on (fr.py:493-498, raised while emcee evaluates p0): -inf and counted, so
// that an `-inf` run treats them as a host-driven one does (any finite proposal replaces them) and a `raise` run dies at once
__global__ void k_fix_start(const int32_t* __restrict__ status, int64_t n, double* __restrict__ lnp, uint32_t* __restrict__ flags)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (status[i] == ST_NON_UNITARY) { lnp[i] = -gf_inf(); atomicAdd(flags, 1u); }
}

__global__ void k_tick(GfStepState* st, int nsteps)
{
    st->iteration_base += (uint64_t)nsteps;
    st->run_step_base += nsteps;
}

// One half-ensemble update for the walkers of one block.  `chain` / `k` = this thread's ensemble and its
// index in the active half (`valid` false for the padding threads of the last block of a chain).
// LPW > 1 (BSM posteriors on small ensembles): LPW adjacent lanes hold the same walker and split its energy
// bins (flux_average); everything else they compute redundantly and identically, lane `sub == 0` writes.
// MODE_BSM_BINNED (one lane per walker): the block stages its chain's binned measurement `btab_g` in LDS beside ctab; everything
// around the likelihood -- verdict tiers, parking, k_stretch_settle behind the half-step -- is the flux-averaged BSM instance's.
// MODE_BSM_TABLE (LPW lanes per walker, as the flux-averaged instance): `btab_g` is the chain's table of side `tside` and stays in
// global memory (up to 16.8 MB); both are block-uniform, so the lookup's addresses start from scalar registers.
template <int NDIM, int MODE, int LPW>
__device__ __forceinline__ void stretch_body(const GfCommon& c, const GfBsm* __restrict__ tb, const double* __restrict__ ptab,
                                             const StretchArgs& s, const int chain, const int k, const bool valid, const int sub,
                                             const double* __restrict__ btab_g = nullptr, const int tside = 0)
{
    constexpr bool BSM = MODE == MODE_BSM_GAUSS || MODE == MODE_BSM_BINNED || MODE == MODE_BSM_TABLE;
    extern __shared__ __attribute__((aligned(16))) double fdyn[];    // LPW > 1: per lane group [nbins_max][3] + [LPW]
    double* fgrp = LPW > 1 ? fdyn + (threadIdx.x / LPW) * GF_FGRP_DOUBLES(s.nbins_max, LPW) : nullptr;
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
    __shared__ __attribute__((aligned(16))) double tiles[GF_WAVES_PER_BLOCK][GF_WAVE * ND];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    __shared__ __attribute__((aligned(16))) double btab[MODE == MODE_BSM_BINNED ? GF_BINNED_DOUBLES : 1];   // the chain's binned measurement
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, ptab, tb, BSM);
    if constexpr (MODE == MODE_BSM_BINNED) load_binned_table(btab, btab_g, tb->nbins);
    __syncthreads();

    const int ndim = NDIM ? NDIM : c.ndim;
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int wave = threadIdx.x / GF_WAVE;
    double* row = tiles[wave] + lane * ndim;
    const uint64_t iteration = s.state->iteration_base + (uint64_t)s.step_offset;
    const int64_t run_step = s.state->run_step_base + s.step_offset;
    const int thin = s.state->thin;
    const bool store_now = s.state->store != 0 && s.chain != nullptr && (run_step % thin) == 0;
    const int64_t store_index = s.state->store_base + (run_step + thin - 1) / thin;   // stored steps before this one
    const int nhalf = s.nwalkers / 2;
    const uint64_t sid = s.stream_ids ? s.stream_ids[chain] : (uint64_t)chain;
    const uint64_t g = sid * (uint64_t)nhalf + (uint64_t)k;  // walker slot of the chain's random stream: the Philox counter
    if (valid) {
    const int w = s.half * nhalf + k;                        // this walker, in the active half
    const int cbase = (1 - s.half) * nhalf;                  // complementary half

    double z, u3;
    int j;
    stretch_draw(s.seed, g, 2 * iteration + s.half, nhalf, s.a, z, j, u3);
    const double* sk = s.pos + ((int64_t)chain * s.nwalkers + w) * ndim;
    const double* cj = s.pos + ((int64_t)chain * s.nwalkers + cbase + j) * ndim;
    stretch_row<NDIM>(row, cj, sk, z, ndim);
    int st;
    unsigned long long pending;
    double lnq;
    if constexpr (MODE == MODE_BSM_TABLE) lnq = proposal_lnprob<NDIM, MODE, LPW>(c, tb, ctab, ttab, row, ndim, st, sub, fgrp, pending, btab_g, tside);
    else lnq = proposal_lnprob<NDIM, MODE, LPW>(c, tb, ctab, ttab, row, ndim, st, sub, fgrp, pending, btab);
    const int64_t wi = (int64_t)chain * s.nwalkers + w;
    const double lnk = s.lnp[wi];
    const double lhs = stretch_lhs(z, u3, ndim);
    if (BSM && pending != 0ull) {
        // undecided unitarity: park the proposal; k_stretch_settle completes this walker's half-step
        if (sub == 0) park_proposal<true>(s.pq, s.pend_rows, (int64_t)chain * nhalf + k, row, ndim, lnq, pending, lhs);
        if constexpr (MODE == MODE_BSM_BINNED) atomicAdd(s.flags + 2, 1u);      // census: proposals k_stretch_settle completed (gf_internal_sampler_parked)
        if constexpr (MODE == MODE_BSM_TABLE) { if (sub == 0) atomicAdd(s.flags + 2, 1u); }      // (one count per lane group)
        return;
    }
    bool accept = lhs > lnk - lnq;                           // false for NaN and for lnq = -inf
    if (st == ST_NON_UNITARY) {                              // the reference raises inside ln_prob here
        accept = false;
        if (sub == 0) atomicAdd(s.flags, 1u);
    }
    if (LPW > 1 && sub != 0) return;                         // the group's results are identical: one writer
    // (written out, as in chain_propose, k_stretch_chain and k_stretch_settle: one shared function moves these kernels' register figures)
    if (accept) {
        double* dst = s.pos + wi * ndim;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            if (!NDIM && d >= ndim) break;
            dst[d] = row[d];
        }
        s.lnp[wi] = lnq;
        s.naccept[wi] += 1u;
    }
    if (store_now) {
        double* dst = s.chain + (((int64_t)chain * s.nstore_cap + store_index) * s.nwalkers + w) * ndim;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            if (!NDIM && d >= ndim) break;
            dst[d] = accept ? row[d] : sk[d];
        }
        if (s.lnp_chain)
            s.lnp_chain[((int64_t)chain * s.nstore_cap + store_index) * s.nwalkers + w] = accept ? lnq : lnk;
    }
    }   // valid
}

// every ensemble samples the same posterior: constants by value (scalar registers), walkers packed densely
#ifndef GF_STRETCH_WAVES
#define GF_STRETCH_WAVES 2      // blocks of 256 threads per CU the half-step kernels are compiled for (A/B: tools/build_variants.sh)
#endif
template <int NDIM, int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK, GF_STRETCH_WAVES) void k_stretch(const GfCommon c, const GfBsm* __restrict__ tb,
                                                          const double* __restrict__ ptab, const StretchArgs s)
{
    const int nhalf = s.nwalkers / 2;
    const int64_t t = (int64_t)blockIdx.x * GF_BLOCK + threadIdx.x;
    const int64_t g = t / LPW;
    const bool valid = g < (int64_t)s.nchains * nhalf;
    const int chain = valid ? (int)(g / nhalf) : 0;
    const int k = valid ? (int)(g - (int64_t)chain * nhalf) : 0;
    if constexpr (MODE == MODE_BSM_BINNED) stretch_body<NDIM, MODE, LPW>(c, tb, ptab, s, chain, k, valid, 0, s.btabs[0]);
    else if constexpr (MODE == MODE_BSM_TABLE) stretch_body<NDIM, MODE, LPW>(c, tb, ptab, s, chain, k, valid, (int)(t % LPW), s.ttabs[0], s.tsides[0]);
    else stretch_body<NDIM, MODE, LPW>(c, tb, ptab, s, chain, k, valid, (int)(t % LPW));
}

// one posterior per ensemble (grid scans, SURVEY.md 8(e) "all chains of a GPU stacked into one launch"):
// blockIdx.y = chain, so that a block's constants are block-uniform and come from scalar loads
template <int NDIM, int MODE, int LPW>
__global__ __launch_bounds__(GF_BLOCK, GF_STRETCH_WAVES) void k_stretch_multi(const StretchArgs s)
{
    const int chain = blockIdx.y;
    const int t = blockIdx.x * GF_BLOCK + threadIdx.x;
    const int k = t / LPW;
    if constexpr (MODE == MODE_BSM_BINNED)
        stretch_body<NDIM, MODE, LPW>(s.commons[chain], s.tbs[chain], s.ptabs[chain], s, chain, k, k < s.nwalkers / 2, 0, s.btabs[chain]);
    else if constexpr (MODE == MODE_BSM_TABLE)
        stretch_body<NDIM, MODE, LPW>(s.commons[chain], s.tbs[chain], s.ptabs[chain], s, chain, k, k < s.nwalkers / 2, t % LPW, s.ttabs[chain],
                                      s.tsides[chain]);
    else stretch_body<NDIM, MODE, LPW>(s.commons[chain], s.tbs[chain], s.ptabs[chain], s, chain, k, k < s.nwalkers / 2, t % LPW);
}

template <int NDIM, int MODE, int LPW>
hipError_t launch_stretch_nml(const GfCommon& c, const GfBsm* tb, const double* ptab, const StretchArgs& a, hipStream_t st)
{
    const size_t lds = LPW > 1 ? (size_t)(GF_BLOCK / LPW) * GF_FGRP_DOUBLES(a.nbins_max, LPW) * sizeof(double) : 0;
    if (a.commons) {
        const dim3 grid((unsigned)(((int64_t)(a.nwalkers / 2) * LPW + GF_BLOCK - 1) / GF_BLOCK), a.nchains);
        hipLaunchKernelGGL((k_stretch_multi<NDIM, MODE, LPW>), grid, dim3(GF_BLOCK), lds, st, a);
    } else {
        const int64_t total = (int64_t)a.nchains * (a.nwalkers / 2) * LPW;
        hipLaunchKernelGGL((k_stretch<NDIM, MODE, LPW>), dim3((unsigned)((total + GF_BLOCK - 1) / GF_BLOCK)), dim3(GF_BLOCK), lds, st,
                           c, tb, ptab, a);
    }
    return hipGetLastError();
}

// ---- one workgroup per ensemble, a whole run in ONE launch --------------------------------------------
// An ensemble of up to a few thousand walkers is a few waves of work per half-step: launched as a grid, every
// half-step is a ~3 us launch that the GPU spends mostly idle (the emcee regime: 100-walker chains, C1).  Here
// block b owns ensemble b for the whole run: walkers, their lnprob and acceptance counters live in LDS, the two
// half-steps of a step are separated by a workgroup barrier instead of a kernel boundary, and the only HBM
// traffic is the stored chain.  Random stream, proposal, evaluation and accept rule are those of k_stretch, so
// the chain is bitwise the same (tests compare the two).  PRIOR_ONLY and SM_GAUSS posteriors.
// MAXT: the largest workgroup the instance is compiled for.  1024 threads would cap the kernel at 128 VGPRs, which the
// likelihood instances overflow (32-256 B of scratch per lane inside the step loop, round 2); workgroups are at most 512 threads
// (two waves per SIMD, up to 256 VGPRs; the instances use 57-195) and a larger half-ensemble takes two or more passes of the loop
// over k.  The reference's 100-walker chain runs on ONE wave.
template <int NDIM, int MODE, int MAXT>
__global__ __launch_bounds__(MAXT) void k_stretch_persist(const PersistArgs s)
{
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
    extern __shared__ __attribute__((aligned(16))) double dyn[];
    const int chain = blockIdx.x;
    const GfCommon& c = s.commons[s.nmodels > 1 ? chain : 0];
    const double* __restrict__ ptab = s.ptabs[s.nmodels > 1 ? chain : 0];
    const int ndim = NDIM ? NDIM : c.ndim;
    const int nw = s.nwalkers, nhalf = nw / 2, nt = blockDim.x;
    // Workers and producers.  A half-step's random quantities -- the stretch factor z, the partner j and the left side of the
    // accept test, ln(z^(ndim-1) / u) -- depend on nothing but the counters, a third of a half-step's instructions (Philox4x32-10,
    // the conversions, a logarithm) on the one wave the reference's 100-walker chain runs on.  With `workers` < blockDim the
    // block's other threads compute them ONE HALF-STEP AHEAD into a double-buffered LDS table while the workers move the
    // walkers; the barrier that separates the half-steps anyway hands the table over.  Same expressions, same values: the chain
    // is bitwise the one-wave chain (tests).
    const int ntw = s.workers > 0 && s.workers < nt ? s.workers : nt;        // worker threads
    const int ntp = nt - ntw;                                                // producer threads (0: the workers draw for themselves)
    const bool producer = (int)threadIdx.x >= ntw;
    // LDS: ctab[64] | pos[nw][ndim] | lnp[nw] | rows[ntw][ndim] | naccept[nw] (u32) | [producers: z[2][nhalf] | lhs[2][nhalf] | j[2][nhalf]]
    double* ctab = dyn;
    double* pos = ctab + GF_MAX_DIM * 4;
    double* lnp = pos + (size_t)nw * ndim;
    double* rows = lnp + nw;
    uint32_t* nacc = reinterpret_cast<uint32_t*>(rows + (size_t)ntw * ndim);
    double* dz = reinterpret_cast<double*>(nacc + ((nw + 1) & ~1));
    double* dlhs = dz + 2 * (size_t)nhalf;
    int* dj = reinterpret_cast<int*>(dlhs + 2 * (size_t)nhalf);
    if (threadIdx.x < GF_MAX_DIM * 4) ctab[threadIdx.x] = ptab[threadIdx.x];
    const int64_t cw = (int64_t)chain * nw;
    for (int i = threadIdx.x; i < nw * ndim; i += nt) pos[i] = s.pos[cw * ndim + i];
    for (int i = threadIdx.x; i < nw; i += nt) { lnp[i] = s.lnp[cw + i]; nacc[i] = s.naccept[cw + i]; }
    double* row = rows + (size_t)(producer ? 0 : threadIdx.x) * ndim;
    const uint64_t gbase = (s.stream_ids ? s.stream_ids[chain] : (uint64_t)chain) * (uint64_t)nhalf;
    // the draws of walker slot k at half-step counter ctr
    auto draw = [&](int k, uint64_t ctr, double& z, int& j, double& lhs) {
        double u3;
        stretch_draw(s.seed, gbase + (uint64_t)k, ctr, nhalf, s.a, z, j, u3);
        lhs = stretch_lhs(z, u3, ndim);
    };
    const uint64_t ctr_first = 2 * s.iteration_base, ctr_end = ctr_first + 2 * (uint64_t)s.nsteps;
    if (producer && s.nsteps > 0)
        for (int k = (int)threadIdx.x - ntw; k < nhalf; k += ntp) {
            double z, lhs; int j;
            draw(k, ctr_first, z, j, lhs);
            dz[k] = z; dlhs[k] = lhs; dj[k] = j;                     // buffer 0 = (ctr_first & 1) * nhalf: see below
        }
    __syncthreads();

    for (int64_t step = 0; step < s.nsteps; ++step) {
        const uint64_t iteration = s.iteration_base + (uint64_t)step;
        const bool store_now = s.store != 0 && s.chain != nullptr && (step % s.thin) == 0;
        const int64_t store_index = s.store_base + (step + s.thin - 1) / s.thin;
        for (int half = 0; half < 2; ++half) {
            const int cbase = (1 - half) * nhalf;
            const uint64_t ctr = 2 * iteration + half;
            const size_t buf = (size_t)(half) * nhalf;                // ctr_first is even: the buffer of counter ctr is its parity
            if (producer) {
                if (ctr + 1 < ctr_end)
                    for (int k = (int)threadIdx.x - ntw; k < nhalf; k += ntp) {
                        double z, lhs; int j;
                        draw(k, ctr + 1, z, j, lhs);
                        const size_t nb = (size_t)(1 - half) * nhalf;
                        dz[nb + k] = z; dlhs[nb + k] = lhs; dj[nb + k] = j;
                    }
            } else
            for (int k = threadIdx.x; k < nhalf; k += ntw) {
                const int w = half * nhalf + k;
                double z, lhs; int j;
                if (ntp > 0) { z = dz[buf + k]; lhs = dlhs[buf + k]; j = dj[buf + k]; }
                else draw(k, ctr, z, j, lhs);
                double* sk = pos + (size_t)w * ndim;
                const double* cj = pos + (size_t)(cbase + j) * ndim;
                stretch_row<NDIM>(row, cj, sk, z, ndim);
                int st;
                unsigned long long pending;
                const double lnq = proposal_lnprob<NDIM, MODE, 1>(c, nullptr, ctab, nullptr, row, ndim, st, 0, nullptr, pending);
                const double lnk = lnp[w];
                const bool accept = lhs > lnk - lnq;
                if (accept) {
#pragma unroll
                    for (int d = 0; d < ND; ++d) {
                        if (!NDIM && d >= ndim) break;
                        sk[d] = row[d];
                    }
                    lnp[w] = lnq;
                    nacc[w] += 1u;
                }
                if (store_now) {
                    double* dst = s.chain + (((int64_t)chain * s.nstore_cap + store_index) * nw + w) * ndim;
#pragma unroll
                    for (int d = 0; d < ND; ++d) {
                        if (!NDIM && d >= ndim) break;
                        dst[d] = sk[d];                           // the walker's position after this half-step
                    }
                    if (s.lnp_chain) s.lnp_chain[((int64_t)chain * s.nstore_cap + store_index) * nw + w] = lnp[w];
                }
            }
            __syncthreads();                                      // the other half moves next: it reads these walkers (and the next draws are in place)
        }
    }
    for (int i = threadIdx.x; i < nw * ndim; i += nt) s.pos[cw * ndim + i] = pos[i];
    for (int i = threadIdx.x; i < nw; i += nt) { s.lnp[cw + i] = lnp[i]; s.naccept[cw + i] = nacc[i]; }
}


template <int NDIM>
hipError_t launch_persist_n(int mode, int nchains, int threads, size_t lds, const PersistArgs& a, hipStream_t st)
{
    if (mode == MODE_PRIOR_ONLY) {
        if (threads <= 256) hipLaunchKernelGGL((k_stretch_persist<NDIM, MODE_PRIOR_ONLY, 256>), dim3(nchains), dim3(threads), lds, st, a);
        else hipLaunchKernelGGL((k_stretch_persist<NDIM, MODE_PRIOR_ONLY, 512>), dim3(nchains), dim3(threads), lds, st, a);
    } else {
        if (threads <= 256) hipLaunchKernelGGL((k_stretch_persist<NDIM, MODE_SM_GAUSS, 256>), dim3(nchains), dim3(threads), lds, st, a);
        else hipLaunchKernelGGL((k_stretch_persist<NDIM, MODE_SM_GAUSS, 512>), dim3(nchains), dim3(threads), lds, st, a);
    }
    return hipGetLastError();
}


// ---- one workgroup per CHAIN, BSM posteriors ------------------------------------------------------------------------------------
// The grid kernels above advance ALL chains of a sampler half-step by half-step, and since round 3 a half-step is followed by
// k_stretch_settle, which takes the exact (emulated x87) unitarity verdict of the proposals the in-kernel tiers could not settle:
// ~66 us of ONE walker's dependent arithmetic.  Measured on the C5 scan (256 chains x 512 walkers, profiles/r03/
// arbitration_latency.txt): ~120 of 65 536 proposals park per half-step, in 30 of the 256 chains -- and all 256 chains, which share
// nothing, waited 66 us for them at the kernel boundary: 37 us of proposals + 67 us of settling per half-step.
//
// Chains are independent (emcee runs them as separate jobs: submitter/sens_dag.py:75-95), so here a workgroup OWNS a chain for a
// whole block of steps: its half-steps follow each other behind a workgroup barrier, the walkers stay where the grid kernels
// keep them (HBM; a chain's 49 KB live in this CU's caches), and when a half-step parks proposals the SAME workgroup settles
// them on the spot -- its four waves become 56 nine-lane teams (gf_unitarity_teams.hpp), a walker's undecided bins fan out over
// them, the last part to finish completes the walker's accept step -- and goes on.  Nobody else waits.  Same Philox counters,
// same proposal_lnprob instance, same chain arithmetic, same accept rule as k_stretch + k_stretch_settle: the chain is bitwise
// the grid sampler's (tests/test_gpu_sampler.py).
constexpr int CH_WAVES = CH_BLOCK / GF_WAVE;

// LDS pointers that stay LDS pointers across a call (ds_ instructions, not flat_)
typedef __attribute__((address_space(3))) double* LdsD;
typedef __attribute__((address_space(3))) unsigned int* LdsU;
typedef __attribute__((address_space(3))) int* LdsI;
typedef __attribute__((address_space(3))) unsigned long long* LdsL;

// One walker's proposal of k_stretch_chain (the pieces of gf_stretch.hpp, as in stretch_body) as a function of its own: the kernel around it holds
// the nine-lane teams' code (~210 VGPRs of its own), and compiled as one body for eight waves per CU (256 VGPRs) the allocator spilled
// inside the evaluation's bin loop (36 us per pass instead of 24).  Out of line, each side has the whole budget.
template <int NDIM>
__device__ __attribute__((noinline)) void chain_propose(const ChainArgs& s, const GfCommon& c, const GfBsm* __restrict__ tb, LdsD ctab_l, LdsD ttab_l,
                                                        LdsD row_l, const int chain, const int k, const int half, const uint64_t iteration,
                                                        const bool store_now, const int64_t store_index, const uint64_t sid, double* my_pend,
                                                        double* lz_rows, unsigned long long* lz_mask, LdsU pk_n, LdsI pk_k, LdsL pk_mask, LdsU lz_n)
{
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
    const double* ctab = (const double*)ctab_l;
    const double* ttab = (const double*)ttab_l;
    double* row = (double*)row_l;
    const int ndim = NDIM ? NDIM : c.ndim;
    const int nw = s.nwalkers, nhalf = nw / 2;
    const int cbase = (1 - half) * nhalf;
    const uint64_t g = sid * (uint64_t)nhalf + (uint64_t)k;
    const int w = half * nhalf + k;
    double z, u3;
    int j;
    stretch_draw(s.seed, g, 2 * iteration + half, nhalf, s.a, z, j, u3);
    const int64_t wi = (int64_t)chain * nw + w;
    const double* sk = s.pos + wi * ndim;
    const double* cj = s.pos + ((int64_t)chain * nw + cbase + j) * ndim;
#pragma unroll
    for (int d = 0; d < ND; ++d) {                        // (not stretch_row: with it k_stretch_chain's spill counts move)
        if (!NDIM && d >= ndim) break;
        const double cv = cj[d];
        row[d] = fma(-z, cv - sk[d], cv);
    }
    int st;
    unsigned long long pending;
    const double lnq = proposal_lnprob<NDIM, MODE_BSM_GAUSS, 1>(c, tb, ctab, ttab, row, ndim, st, 0, nullptr, pending);
    const double lnk = s.lnp[wi];
    const double lhs = stretch_lhs(z, u3, ndim);
    bool accept = lhs > lnk - lnq;                        // false for NaN and for lnq = -inf
    if (pending != 0ull && accept) {
        // undecided unitarity and the verdict DECIDES: park it; this workgroup settles it below, before anybody
        // reads this walker again
        double* dst = my_pend + (size_t)k * GF_PEND_STRIDE;
        park_row(dst, row, ndim);
        dst[GF_MAX_DIM] = lnq;
        dst[GF_MAX_DIM + 1] = lhs;
        const unsigned int at = atomicAdd((unsigned int*)pk_n, 1u);
        pk_k[at] = k;
        pk_mask[at] = pending;
    } else {
        if (pending != 0ull) {
            // undecided, but rejected either way: only the count wants the verdict -- later
            const unsigned int at = atomicAdd((unsigned int*)lz_n, 1u);
            park_row(lz_rows + (size_t)at * GF_PEND_STRIDE, row, ndim);
            lz_mask[at] = pending;
        }
        if (st == ST_NON_UNITARY) { accept = false; atomicAdd(s.flags, 1u); }      // the reference raises inside ln_prob here
        if (accept) {
            double* dst = s.pos + wi * ndim;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (!NDIM && d >= ndim) break;
                dst[d] = row[d];
            }
            s.lnp[wi] = lnq;
            s.naccept[wi] += 1u;
        }
        if (store_now) {
            double* dst = s.chain + (((int64_t)chain * s.nstore_cap + store_index) * nw + w) * ndim;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (!NDIM && d >= ndim) break;
                dst[d] = accept ? row[d] : sk[d];
            }
            if (s.lnp_chain) s.lnp_chain[((int64_t)chain * s.nstore_cap + store_index) * nw + w] = accept ? lnq : lnk;
        }
    }
}

// The workgroup's eight waves as 56 nine-lane teams on a list of `count` proposals whose unitarity is undecided.  Two stages per chunk
// of up to WT_CAP walkers, so that nothing is computed twice and no team idles behind a walker with many bins:
//   A  a team per WALKER builds the walker's two Hamiltonian terms (fr.py:380-394 in emulated x87: ~16 us) and leaves them in LDS;
//   B  a team per (walker, bin) PAIR takes the terms from LDS and evaluates that one energy bin (~23 us).  Pairs are handed out
//      rank-major -- every walker's highest undecided energy first (the likeliest to fail), then the second-highest ... -- and a pair
//      whose walker has failed meanwhile (fr.py:493-494: the reference raises at the first) is dropped unevaluated.  The last pair of
//      a walker to report calls done(item, failed).
// (k_stretch_settle, gf_unitarity.hip, gives every part of a walker its own copy of the terms: right for a kernel the whole GPU runs,
// 3 584 teams for a few hundred pairs; here 56 teams face up to ~100 pairs per half-step of a chain in the failing region, and the
// terms were 40 % of the work.)
//   row_of(item) -> the proposal's row (theta at [0, ndim))       mask_of(item) -> its undecided bins (non-zero)
//   head, aux -> LDS words;   ctl -> LDS [2 * CH_BLOCK], zero on entry and on exit;   wt -> LDS [WT_CAP][9][8] doubles
// A workgroup-uniform call: it contains workgroup barriers.
constexpr int WT_CAP = 64;                             // walkers whose terms are held at once (64 x 576 B = 36 KB)
constexpr int WT_DOUBLES = WT_CAP * Team9::LANES * 8;
__device__ __forceinline__ int nth_bit_from_top(unsigned long long m, unsigned int n)
{
    for (unsigned int i = 0; i < n; ++i) m &= ~(1ull << (63 - __clzll((long long)m)));
    return 63 - __clzll((long long)m);
}
template <class RowOf, class MaskOf, class Done>
__device__ __forceinline__ void chain_settle(double* uni, double* wt, unsigned int count, unsigned int* head, unsigned int* aux, unsigned int* ctl,
                                             const GfCommon& c, const GfBsm* __restrict__ tb, RowOf row_of, MaskOf mask_of, Done done)
{
    const int lane = threadIdx.x & (GF_WAVE - 1), wave = threadIdx.x / GF_WAVE;
    const int grp = lane / Team9::LANES;
    const bool team_active = grp < Team9::PER_WAVE;                                    // lane 63 has no team
    const int tl = lane - grp * Team9::LANES;                                          // lane within the team
    Team9 tm;
    tm.init(uni + ((size_t)wave * Team9::PER_WAVE + (team_active ? grp : 0)) * Team9::DOUBLES, tl);
    const bool lead = tm.leader();
    for (unsigned int first = 0; first < count; first += (unsigned int)WT_CAP) {
        const unsigned int nw_chunk = count - first < (unsigned int)WT_CAP ? count - first : (unsigned int)WT_CAP;
        if (threadIdx.x == 0) { *head = 0u; *aux = 0u; }
        __syncthreads();
        // ---- A: the walkers' terms
        for (;;) {
            const unsigned long long nb = __ballot(team_active && lead);
            unsigned int base = 0;
            const int leader = __ffsll((long long)nb) - 1;
            if (lane == leader) base = atomicAdd(head, (unsigned int)__popcll(nb));
            base = (unsigned int)__shfl((int)base, leader);
            const unsigned int idx = base + (unsigned int)grp;                       // teams 0..6 of the wave take consecutive walkers
            const bool have = team_active && idx < nw_chunk;
            if (__ballot(have) == 0ull) break;                                        // wave-uniform: the chunk's walkers are handed out
            if (have) {
                const unsigned int item = first + idx;
                tm.terms(c, *tb, row_of(item), 0, 1, 0, GF_PEND_STRIDE);
                double* w = wt + ((size_t)idx * Team9::LANES + tl) * 8;
                w[0] = tm.hs.re.hi; w[1] = tm.hs.re.lo; w[2] = tm.hs.im.hi; w[3] = tm.hs.im.lo;
                w[4] = tm.hn.re.hi; w[5] = tm.hn.re.lo; w[6] = tm.hn.im.hi; w[7] = tm.hn.im.lo;
                if (lead) atomicMax(aux, (unsigned int)__popcll(mask_of(item)));      // the most bins any walker of the chunk brings
            }
        }
        __syncthreads();
        const unsigned int maxb = *aux;
        const unsigned int npairs = nw_chunk * maxb;                                  // rank-major grid of pairs; holes where a walker has fewer bins
        __syncthreads();
        if (threadIdx.x == 0) *head = 0u;
        __syncthreads();
        // ---- B: one energy bin per team and round
        for (;;) {
            const unsigned long long nb = __ballot(team_active && lead);
            unsigned int base = 0;
            const int leader = __ffsll((long long)nb) - 1;
            if (lane == leader) base = atomicAdd(head, (unsigned int)__popcll(nb));
            base = (unsigned int)__shfl((int)base, leader);
            const unsigned int v = base + (unsigned int)grp;
            const bool inrange = team_active && v < npairs;
            if (__ballot(inrange) == 0ull) break;
            if (inrange) {
                const unsigned int idx = v % nw_chunk, rank = v / nw_chunk;
                const unsigned int item = first + idx;
                const unsigned long long im = mask_of(item);
                const unsigned int nbits = (unsigned int)__popcll(im);
                if (rank < nbits) {
                    bool failed = false;
                    if (__atomic_load_n(&ctl[2 * idx + 1], __ATOMIC_RELAXED) == 0u) {   // else: another bin of this walker has failed already
                        const double* w = wt + ((size_t)idx * Team9::LANES + tl) * 8;
                        tm.hs.re.hi = w[0]; tm.hs.re.lo = w[1]; tm.hs.im.hi = w[2]; tm.hs.im.lo = w[3];
                        tm.hn.re.hi = w[4]; tm.hn.re.lo = w[5]; tm.hn.im.hi = w[6]; tm.hn.im.lo = w[7];
                        const int kk = nth_bit_from_top(im, rank);
                        const double res = tm.bin(tb->inv2e[kk], tb->epow[kk]);
                        failed = !(res < 1e-7);                                       // fr.py:493-494 (NaN raises too)
                    }
                    if (lead) {
                        if (failed) atomicOr(&ctl[2 * idx + 1], 1u);
                        __threadfence_block();
                        const unsigned int before = atomicAdd(&ctl[2 * idx], 1u);
                        if (before == nbits - 1u) {                                   // the last pair of the walker to report
                            __threadfence_block();
                            const bool bad = atomicOr(&ctl[2 * idx + 1], 0u) != 0u;
                            ctl[2 * idx] = 0u;
                            ctl[2 * idx + 1] = 0u;
                            done(item, bad);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int NDIM>
__global__ __launch_bounds__(CH_BLOCK) void k_stretch_chain(const ChainArgs s)
{
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
    constexpr int TEAMS = CH_WAVES * Team9::PER_WAVE;                       // 56 nine-lane teams
    constexpr int TEAM_DOUBLES = TEAMS * Team9::DOUBLES;
    constexpr int TILE_DOUBLES = CH_WAVES * GF_WAVE * ND;
    // one buffer, two lives: the proposals' rows while a pass of the half-step is evaluated, the teams' slots while its parked
    // proposals are settled (their rows are in `pend_rows` by then)
    __shared__ __attribute__((aligned(16))) double uni[TEAM_DOUBLES > TILE_DOUBLES ? TEAM_DOUBLES : TILE_DOUBLES];
    __shared__ __attribute__((aligned(16))) double ctab[GF_MAX_DIM * 4 + 20];
    __shared__ unsigned long long pk_mask[CH_BLOCK];      // the pass's parked proposals: undecided bins ...
    __shared__ int pk_k[CH_BLOCK];                        // ... walker slot in the active half
    __shared__ unsigned int pk_ctl[2 * CH_BLOCK];         // per listed proposal: parts finished, one of them failed (zero between uses)
    __shared__ unsigned int pk_n, pk_head, pk_aux, lz_n;
    __shared__ __attribute__((aligned(16))) double wt[WT_DOUBLES];    // chain_settle: the Hamiltonian terms of the walkers being settled

    const int chain = blockIdx.x;
    const GfCommon& c = s.commons[s.nmodels > 1 ? chain : 0];
    const GfBsm* __restrict__ tb = s.nmodels > 1 ? s.tbs[chain] : s.tb;
    const double* __restrict__ ptab = s.ptabs[s.nmodels > 1 ? chain : 0];
    double* ttab = ctab + GF_MAX_DIM * 4;
    load_eval_tables(ctab, ptab, tb, true);
    for (int i = threadIdx.x; i < 2 * CH_BLOCK; i += CH_BLOCK) pk_ctl[i] = 0u;
    if (threadIdx.x == 0) lz_n = 0u;
    __syncthreads();

    const int ndim = NDIM ? NDIM : c.ndim;
    const int lane = threadIdx.x & (GF_WAVE - 1), wave = threadIdx.x / GF_WAVE;
    const int nw = s.nwalkers, nhalf = nw / 2;
    const uint64_t sid = s.stream_ids ? s.stream_ids[chain] : (uint64_t)chain;
    double* row = uni + (size_t)wave * GF_WAVE * ND + (size_t)lane * ndim;          // (stretch_body: tiles[wave] + lane * ndim)
    double* const my_pend = s.pend_rows + (size_t)chain * nhalf * GF_PEND_STRIDE;    // this chain's parked rows, by walker slot
    // proposals that are REJECTED WHATEVER THEIR VERDICT (the accept test fails even if they are unitary): the chain does not wait
    // for them -- the verdict only feeds the count of proposals the reference would have raised on.  Their rows queue up here
    // and are settled in bulk when the list fills and at the end of the launch.
    double* const lz_rows = s.lazy_rows + (size_t)chain * s.lazy_cap * GF_PEND_STRIDE;
    unsigned long long* const lz_mask = s.lazy_mask + (size_t)chain * s.lazy_cap;
    unsigned long long* const stat = s.stats ? s.stats + (size_t)chain * 8 : nullptr;
    auto flush_lazy = [&]() {                              // workgroup-uniform call; barriers inside
        const unsigned int n = lz_n;
        if (n != 0u) {
            const unsigned long long t0 = wall_clock64();
            if (threadIdx.x == 0) pk_head = 0u;
            __syncthreads();
            chain_settle(uni, wt, n, &pk_head, &pk_aux, pk_ctl, c, tb,
                         [&](unsigned int i) { return lz_rows + (size_t)i * GF_PEND_STRIDE; },
                         [&](unsigned int i) { return lz_mask[i]; },
                         [&](unsigned int, bool bad) { if (bad) atomicAdd(s.flags, 1u); });
            __syncthreads();
            if (threadIdx.x == 0) {
                lz_n = 0u;
                if (stat) { stat[2] += 10ull * (wall_clock64() - t0); stat[5] += n; stat[7] += 1ull; }
            }
            __syncthreads();
        }
    };

    for (int step = 0; step < s.nsteps; ++step) {
        const uint64_t iteration = s.iteration_base + (uint64_t)step;
        const int64_t run_step = s.run_step_base + step;
        const bool store_now = s.store != 0 && s.chain != nullptr && (run_step % s.thin) == 0;
        const int64_t store_index = s.store_base + (run_step + s.thin - 1) / s.thin;
        for (int half = 0; half < 2; ++half) {
            for (int kb = 0; kb < nhalf; kb += CH_BLOCK) {
                if (lz_n + (unsigned int)(nhalf < CH_BLOCK ? nhalf : CH_BLOCK) > (unsigned int)s.lazy_cap) flush_lazy();   // (uniform: lz_n is stable between barriers)
                if (threadIdx.x == 0) { pk_n = 0u; pk_head = 0u; }
                __syncthreads();
                const unsigned long long t_pass = wall_clock64();
                const int k = kb + (int)threadIdx.x;
                if (k < nhalf)
                    chain_propose<NDIM>(s, c, tb, (LdsD)ctab, (LdsD)ttab, (LdsD)row, chain, k, half, iteration, store_now, store_index, sid,
                                        my_pend, lz_rows, lz_mask, (LdsU)&pk_n, (LdsI)pk_k, (LdsL)pk_mask, (LdsU)&lz_n);
                __syncthreads();                                      // rows are done with; pk_n is final; this pass's updates are visible
                const unsigned int count = pk_n;
                const unsigned long long t_settle = wall_clock64();
                if (threadIdx.x == 0 && stat) { stat[0] += 10ull * (t_settle - t_pass); stat[6] += 1ull; }
                if (count != 0u) {
                    chain_settle(uni, wt, count, &pk_head, &pk_aux, pk_ctl, c, tb,
                                 [&](unsigned int i) { return my_pend + (size_t)pk_k[i] * GF_PEND_STRIDE; },
                                 [&](unsigned int i) { return pk_mask[i]; },
                                 [&](unsigned int i, bool bad) {
                                     // the walker's accept step, as k_stretch_settle ends it: the accept test itself has passed
                                     const double* prow = my_pend + (size_t)pk_k[i] * GF_PEND_STRIDE;
                                     const int w = half * nhalf + pk_k[i];
                                     const int64_t wi = (int64_t)chain * nw + w;
                                     const double lnq = prow[GF_MAX_DIM];
                                     const double lnk = s.lnp[wi];
                                     const bool accept = !bad;
                                     if (bad) atomicAdd(s.flags, 1u);
                                     double* pw = s.pos + wi * ndim;
                                     if (store_now) {
                                         double* dst = s.chain + (((int64_t)chain * s.nstore_cap + store_index) * nw + w) * ndim;
                                         for (int d = 0; d < ndim; ++d) dst[d] = accept ? prow[d] : pw[d];
                                         if (s.lnp_chain) s.lnp_chain[((int64_t)chain * s.nstore_cap + store_index) * nw + w] = accept ? lnq : lnk;
                                     }
                                     if (accept) {
                                         for (int d = 0; d < ndim; ++d) pw[d] = prow[d];
                                         s.lnp[wi] = lnq;
                                         s.naccept[wi] += 1u;
                                     }
                                 });
                    __syncthreads();                                  // the teams' slots become rows again; the settled walkers are in place
                    if (threadIdx.x == 0 && stat) { stat[1] += 10ull * (wall_clock64() - t_settle); stat[3] += count; stat[4] += 1ull; }
                }
            }
        }
    }
    flush_lazy();
}


// Ensemble mean of every stored step: chain [nchains][cap][nwalkers][ndim] -> mean [nchains][nstored][ndim]
// (the series emcee's acor works on, golemflavor/mcmc.py:45-51).  One block per (step, chain); thread t sums
// the elements t, t + 256, ... of the step's contiguous nwalkers x ndim block whose column is (t mod ndim)
// -- 256 mod ndim must be 0 for that, otherwise threads stride by the largest multiple of ndim <= 256 -- then
// a fixed LDS tree: deterministic, coalesced, one pass over the chain at HBM rate.
__global__ __launch_bounds__(GF_BLOCK) void k_walker_mean(const double* __restrict__ chain, int64_t cap, int64_t nstored,
                                                          int nwalkers, int ndim, double* __restrict__ mean)
{
    __shared__ double part[GF_BLOCK];
    const int64_t step = blockIdx.x;
    const int ch = blockIdx.y;
    const double* src = chain + ((int64_t)ch * cap + step) * nwalkers * ndim;
    const int stride = (GF_BLOCK / ndim) * ndim;            // threads in use; a multiple of ndim
    const int n = nwalkers * ndim;
    double acc = 0.0;
    if ((int)threadIdx.x < stride)
        for (int i = threadIdx.x; i < n; i += stride) acc += src[i];
    part[threadIdx.x] = (int)threadIdx.x < stride ? acc : 0.0;
    __syncthreads();
    // thread d < ndim folds the partial sums of its column in a fixed order
    if ((int)threadIdx.x < ndim) {
        double sum = 0.0;
        for (int t = threadIdx.x; t < stride; t += ndim) sum += part[t];
        mean[((int64_t)ch * nstored + step) * ndim + threadIdx.x] = sum / (double)nwalkers;
    }
}

template <int NDIM>
hipError_t launch_stretch_n(const GfCommon& c, const GfBsm* tb, const double* ptab, const StretchArgs& a, hipStream_t st)
{
    switch (c.mode) {
    case MODE_PRIOR_ONLY: return launch_stretch_nml<NDIM, MODE_PRIOR_ONLY, 1>(c, tb, ptab, a, st);
    case MODE_SM_GAUSS: return launch_stretch_nml<NDIM, MODE_SM_GAUSS, 1>(c, tb, ptab, a, st);
    default:
        switch (a.lpw) {
        case 2: return launch_stretch_nml<NDIM, MODE_BSM_GAUSS, 2>(c, tb, ptab, a, st);
        case 4: return launch_stretch_nml<NDIM, MODE_BSM_GAUSS, 4>(c, tb, ptab, a, st);
        case 16: return launch_stretch_nml<NDIM, MODE_BSM_GAUSS, 16>(c, tb, ptab, a, st);
        default: return launch_stretch_nml<NDIM, MODE_BSM_GAUSS, 1>(c, tb, ptab, a, st);
        }
    }
}

// the tabulated likelihood: the flux-averaged instance's lane counts
template <int NDIM>
hipError_t launch_stretch_table(const GfCommon& c, const GfBsm* tb, const double* ptab, const StretchArgs& a, hipStream_t st)
{
    switch (a.lpw) {
    case 2: return launch_stretch_nml<NDIM, MODE_BSM_TABLE, 2>(c, tb, ptab, a, st);
    case 4: return launch_stretch_nml<NDIM, MODE_BSM_TABLE, 4>(c, tb, ptab, a, st);
    case 16: return launch_stretch_nml<NDIM, MODE_BSM_TABLE, 16>(c, tb, ptab, a, st);
    default: return launch_stretch_nml<NDIM, MODE_BSM_TABLE, 1>(c, tb, ptab, a, st);
    }
}

}  // namespace

// ---- the launchers (gf_sampler_launch.h) ------------------------------------------------------------------------------------------
hipError_t gf_launch_fix_start(const int32_t* status, int64_t n, double* lnp, uint32_t* flags, hipStream_t st)
{
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_fix_start, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, status, n, lnp, flags);
    return hipGetLastError();
}

hipError_t gf_launch_tick(GfStepState* state, int nsteps, hipStream_t st)
{
    hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, st, state, nsteps);
    return hipGetLastError();
}

// threads and dynamic LDS of the persistent kernel; lds == 0: the ensemble does not fit one workgroup
void gf_persist_geometry(int nwalkers, int ndim, int* threads, size_t* lds, int* workers, int nchains, int cus)
{
    const int nhalf = nwalkers / 2;
    int nt = ((nhalf + GF_WAVE - 1) / GF_WAVE) * GF_WAVE;
    if (nt > 512) nt = 512;       // a workgroup of 1024 threads is capped at 128 VGPRs, which the likelihood instances overflow (32-256 B of
                                  // scratch per lane inside the step loop); the half-ensemble loop strides by the block size anyway
    // as many producer threads again while the block stays within 512 threads (k_stretch_persist) -- where a chain's LATENCY is what
    // counts: up to two ensembles per CU one 100-walker chain steps in 3.6 us instead of 4.1; with the GPU full of ensembles the
    // producers only take issue slots and LDS from the workers (4096 chains: 2.8e10 evals/s against 3.9e10; tools/bench_c1_chains.py)
    static const bool no_producers = gf_internal_env("GF_SAMPLER_NO_PRODUCERS", 0) != nullptr;       // diagnostics / A-B
    const size_t base = sizeof(double) * ((size_t)GF_MAX_DIM * 4 + (size_t)nwalkers * ndim + nwalkers + (size_t)nt * ndim) +
                        sizeof(uint32_t) * (size_t)((nwalkers + 1) & ~1);
    const size_t draws = (sizeof(double) * 4 + sizeof(int) * 2) * (size_t)nhalf;
    const bool producers = nt <= 256 && !no_producers && base + draws <= 64 * 1024 && nchains <= 2 * cus;
    const size_t bytes = base + (producers ? draws : 0);
    if (workers) *workers = nt;
    *threads = producers ? 2 * nt : nt;
    *lds = (bytes <= 64 * 1024 && nhalf <= 4 * 1024) ? bytes : 0;
}

hipError_t gf_launch_persist(int mode, int ndim, int nchains, int threads, size_t lds, const PersistArgs& a, hipStream_t st)
{
    switch (ndim) {
    case 4: return launch_persist_n<4>(mode, nchains, threads, lds, a, st);
    case 6: return launch_persist_n<6>(mode, nchains, threads, lds, a, st);
    case 7: return launch_persist_n<7>(mode, nchains, threads, lds, a, st);
    case 12: return launch_persist_n<12>(mode, nchains, threads, lds, a, st);
    default: return launch_persist_n<0>(mode, nchains, threads, lds, a, st);
    }
}

hipError_t gf_launch_chain(int ndim, int nchains, const ChainArgs& a, hipStream_t st)
{
    switch (ndim) {
    case 7: hipLaunchKernelGGL(k_stretch_chain<7>, dim3(nchains), dim3(CH_BLOCK), 0, st, a); break;
    case 12: hipLaunchKernelGGL(k_stretch_chain<12>, dim3(nchains), dim3(CH_BLOCK), 0, st, a); break;
    default: hipLaunchKernelGGL(k_stretch_chain<0>, dim3(nchains), dim3(CH_BLOCK), 0, st, a); break;
    }
    return hipGetLastError();
}

hipError_t gf_launch_stretch(const GfCommon& c, const GfBsm* tb, const double* ptab, const StretchArgs& a, hipStream_t st)
{
    if (a.ttabs)                            // the tabulated likelihood: the row widths of the BSM posteriors, then the lanes per walker
        switch (c.ndim) {
        case 7: return launch_stretch_table<7>(c, tb, ptab, a, st);
        case 12: return launch_stretch_table<12>(c, tb, ptab, a, st);
        default: return launch_stretch_table<0>(c, tb, ptab, a, st);
        }
    if (a.btabs)                            // the energy-resolved likelihood: one lane per walker, the row widths of the BSM posteriors
        switch (c.ndim) {
        case 7: return launch_stretch_nml<7, MODE_BSM_BINNED, 1>(c, tb, ptab, a, st);
        case 12: return launch_stretch_nml<12, MODE_BSM_BINNED, 1>(c, tb, ptab, a, st);
        default: return launch_stretch_nml<0, MODE_BSM_BINNED, 1>(c, tb, ptab, a, st);
        }
    switch (c.ndim) {
    case 4: return launch_stretch_n<4>(c, tb, ptab, a, st);
    case 6: return launch_stretch_n<6>(c, tb, ptab, a, st);
    case 7: return launch_stretch_n<7>(c, tb, ptab, a, st);
    case 12: return launch_stretch_n<12>(c, tb, ptab, a, st);
    default: return launch_stretch_n<0>(c, tb, ptab, a, st);
    }
}

hipError_t gf_launch_walker_mean(const double* d_chain, int64_t cap, int64_t nstored, int nchains, int nwalkers, int ndim, double* d_mean,
                                 hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (int ch0 = 0; ch0 < nchains && e == hipSuccess; ch0 += 65535) {          // gridDim.y <= 65535
        const int nch = nchains - ch0 < 65535 ? nchains - ch0 : 65535;
        hipLaunchKernelGGL(k_walker_mean, dim3((unsigned)nstored, (unsigned)nch), dim3(GF_BLOCK), 0, st,
                           d_chain + (size_t)ch0 * cap * nwalkers * ndim, cap, nstored, nwalkers, ndim, d_mean + (size_t)ch0 * nstored * ndim);
        e = hipGetLastError();
    }
    return e;
}
