// gf_table.hpp -- the tabulated flavour-plane likelihood: ln L of a composition by linear interpolation in a
// table over the triangular lattice of side N.
//
// The table holds ln L at the (N + 1)(N + 2) / 2 nodes (i, j), 0 <= i <= N, 0 <= j <= N - i: node (i, j) is the composition
// (fr_e, fr_mu) = (i / N, j / N) and lies at i (2N + 3 - i) / 2 + j.  Every value is finite or -inf.  For a composition fr:
//   u = fr[0] * N, v = fr[1] * N (one rounding each); a NaN in either makes ln L NaN
//   u clamped to [0, N], then v to [0, N - u] (N - u rounded once)
//   i = min(floor(u), N - 1), j = min(floor(v), N - 1 - i), fu = u - i, fv = v - j (both exact)
//   upward triangle, when fu + fv <= 1 (the sum rounded once) or j == N - 1 - i:
//       L = (T00 + fu * (T10 - T00)) + fv * (T01 - T00)
//   downward triangle otherwise:
//       L = (T11 + (1 - fu) * (T01 - T11)) + (1 - fv) * (T10 - T11)
//   with Tab the value at node (i + a, j + b); any of the three at -inf makes L -inf.
// No fma anywhere: every product and every sum is rounded on its own, in the order the parentheses give (the fu product is formed and added
// first).  The functions carry contract(off) themselves for the device build; the host build (tests/table/table_host.cpp) is compiled
// with contraction off as a whole.
//
// Compiles for the device (hipcc: gf_table.hip, gf_nested.hip, gf_simplex.hip) and for the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFTAB_HD __host__ __device__ __forceinline__
#else
#define GFTAB_HD inline
#endif

#define GF_TABLE_NSIDE_LIMIT 2048        // GF_TABLE_MAX_NSIDE of the public header (gf_model.hip asserts the two agree)

namespace gftab {

GFTAB_HD double neg_inf() { return -__builtin_inf(); }

// the nodes of a table of side N, and where node (i, j) lies
GFTAB_HD int64_t node_count(int N) { return ((int64_t)N + 1) * ((int64_t)N + 2) / 2; }
GFTAB_HD int64_t node_at(int N, int i, int j) { return (int64_t)i * (2 * (int64_t)N + 3 - i) / 2 + j; }

// the cell of a composition: the lower left node (i, j), the offsets into the cell and which of its two triangles
struct Cell {
    int i, j;
    double fu, fv;
    int up;
};

// false for a NaN in f0 or f1 (`c` is then not written)
GFTAB_HD bool locate(double f0, double f1, int N, Cell& c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double n = (double)N;
    double u = f0 * n;
    double v = f1 * n;
    if (u != u || v != v) return false;
    u = u < 0.0 ? 0.0 : (u > n ? n : u);
    const double vmax = n - u;
    v = v < 0.0 ? 0.0 : (v > vmax ? vmax : v);
    int i = (int)__builtin_floor(u);
    if (i > N - 1) i = N - 1;
    int j = (int)__builtin_floor(v);
    if (j > N - 1 - i) j = N - 1 - i;
    c.i = i;
    c.j = j;
    c.fu = u - (double)i;
    c.fv = v - (double)j;
    c.up = (c.fu + c.fv <= 1.0) || j == N - 1 - i;
    return true;
}

// the three nodes of the cell's triangle, in the order interp takes their values: upward (i, j), (i + 1, j), (i, j + 1); downward
// (i + 1, j + 1), (i, j + 1), (i + 1, j).  All three lie inside the table (a downward triangle has j <= N - 2 - i).
GFTAB_HD void nodes(const Cell& c, int N, int64_t at[3])
{
    const int64_t a00 = node_at(N, c.i, c.j);
    const int64_t a10 = a00 + (N + 1 - c.i);              // row i holds N + 1 - i nodes
    if (c.up) { at[0] = a00; at[1] = a10; at[2] = a00 + 1; }
    else { at[0] = a10 + 1; at[1] = a00 + 1; at[2] = a10; }
}

// ta, tb, tc: the values at nodes(...)'s three
GFTAB_HD double interp(const Cell& c, double ta, double tb, double tc)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (ta == neg_inf() || tb == neg_inf() || tc == neg_inf()) return neg_inf();
    if (c.up) {
        // ta = T00, tb = T10, tc = T01
        const double du = tb - ta;
        const double dv = tc - ta;
        const double pu = c.fu * du;
        const double pv = c.fv * dv;
        const double s = ta + pu;
        return s + pv;
    }
    // ta = T11, tb = T01, tc = T10
    const double gu = 1.0 - c.fu;
    const double gv = 1.0 - c.fv;
    const double du = tb - ta;
    const double dv = tc - ta;
    const double pu = gu * du;
    const double pv = gv * dv;
    const double s = ta + pu;
    return s + pv;
}

// ln L of the composition (f0, f1, .) under the table `tab` of side N
GFTAB_HD double lookup(const double* tab, int N, double f0, double f1)
{
    Cell c;
    if (!locate(f0, f1, N, c)) return __builtin_nan("");
    int64_t at[3];
    nodes(c, N, at);
    return interp(c, tab[at[0]], tab[at[1]], tab[at[2]]);
}

}  // namespace gftab
