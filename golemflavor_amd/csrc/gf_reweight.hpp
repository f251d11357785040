// gf_reweight.hpp -- the log-weight of a stored sample under another target: lnw = l_t - l0, and the rows that
// carry no weight.  l0 is what the sample was drawn under (its stored ln_prob; on the measurement path the Gaussian block of the
// sampling model), l_t the same quantity under the target, status the row's verdict under the target (GF_ST_*).
//
// Compiles for the device (hipcc: gf_reweight.hip) and for the host (tests/reweight/reweight_host.cpp, g++ with contraction off).  One
// rounded subtraction, plain comparisons; the rules are tried in this order and a row is counted under the first that holds:
//   RW_BAD_BASE     l0 is not finite (-inf, +inf or NaN): the sample has no density to divide by
//   RW_NONUNITARY   status is GF_ST_NON_UNITARY: the reference would have raised on the row under the target
//   RW_OUTSIDE      l_t is -inf or NaN: the target puts no mass there (outside its box, a Gaussian below the underflow wall)
//   RW_KEPT         otherwise, lnw = l_t - l0
// Everything but RW_KEPT gives lnw = -inf, a weight of exactly zero in gf_nested_post.hpp's pipeline.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFRW_HD __host__ __device__ __forceinline__
#else
#define GFRW_HD inline
#endif

#if defined(__clang__)
#define GFRW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GFRW_NO_CONTRACT
#endif

namespace gfrw {

constexpr int MAX_TARGETS = 64;          // GF_REWEIGHT_MAX_TARGETS
constexpr int STATUS_NON_UNITARY = 2;    // GF_ST_NON_UNITARY
enum { RW_KEPT = 0, RW_BAD_BASE = 1, RW_NONUNITARY = 2, RW_OUTSIDE = 3 };

GFRW_HD double neg_inf() { return -__builtin_inf(); }
GFRW_HD bool finite(double x) { return x == x && x != __builtin_inf() && x != -__builtin_inf(); }

GFRW_HD int classify(double lt, double l0, int32_t status)
{
    if (!finite(l0)) return RW_BAD_BASE;
    if (status == STATUS_NON_UNITARY) return RW_NONUNITARY;
    if (lt != lt || lt == neg_inf()) return RW_OUTSIDE;
    return RW_KEPT;
}

GFRW_HD double lnw(double lt, double l0, int kind)
{
    GFRW_NO_CONTRACT
    return kind == RW_KEPT ? lt - l0 : neg_inf();
}

// the resampling stream of target t of the chain with Philox stream id `sid`
GFRW_HD uint64_t resample_id(uint64_t sid, int t) { return sid * (uint64_t)MAX_TARGETS + (uint64_t)t; }

}  // namespace gfrw
