// The stretch move (Goodman & Weare 2010; gf_sampler.hip's header has the algebra), written once for the launch shapes of the
// ensemble sampler -- the grid kernels, the persistent workgroup kernel and the one-workgroup-per-chain kernel: a half-step's draw,
// the left side of its accept test, and the proposal's row.  The shapes produce the same chain bit for bit because they call these
// pieces.  (The parking of an undecided proposal: gf_propose.hpp.  The end of a walker's half-step -- update and stored sample --
// stays written out in its five places: routed through one function it changes the register figures of the kernels around it,
// profiles/stretch_move/README.txt.)
#pragma once
#include "gf_propose.hpp"

namespace {

// The draw of walker slot `g` of a random stream at half-step counter `ctr` (= 2 * iteration + half): one Philox block, key = seed.
// u1 has 53 bits, the partner j in the complementary half of `nhalf` walkers and u3 32 bits each; z = ((a-1) u1 + 1)^2 / a.
__device__ __forceinline__ void stretch_draw(uint64_t seed, uint64_t g, uint64_t ctr, int nhalf, double a, double& z, int& j, double& u3)
{
    uint32_t r[4];
    philox_block((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const double u1 = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
    j = (int)(((uint64_t)r[2] * (uint64_t)nhalf) >> 32);
    u3 = ((double)r[3] + 0.5) * (1.0 / 4294967296.0);
    const double zr = fma(a - 1.0, u1, 1.0);
    z = zr * zr / a;
}

// ... and the left side of its accept test, ln(z^(ndim-1) / u3) > lnp(s_k) - lnp(q): it depends on the draw alone, so that a kernel
// may form it before the evaluation (the persistent kernel's producer threads, a half-step ahead) or after it
__device__ __forceinline__ double stretch_lhs(double z, double u3, int ndim)
{
    double zp = 1.0;
    for (int d = 1; d < ndim; ++d) zp *= z;
    return log(zp / u3);
}

// The proposal q = c_j - z (c_j - s_k).  NDIM: the dimension the kernel is compiled for, 0 = any (unrolled, with an early exit)
template <int NDIM>
__device__ __forceinline__ void stretch_row(double* row, const double* cj, const double* sk, double z, int ndim)
{
    constexpr int ND = NDIM ? NDIM : GF_MAX_DIM;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        if (!NDIM && d >= ndim) break;
        const double cv = cj[d];
        row[d] = fma(-z, cv - sk[d], cv);
    }
}

}  // namespace
