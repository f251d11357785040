// gf_elements_exact.hpp -- the moduli |U_ij| of a row through the reference's own route: angles_to_u in the emulated 80-bit
// arithmetic of gf_x87.hpp (asin / acos / sin / cos, np.dot in index order: the CPU oracle's values bit for bit), hypot of each
// entry's parts, ONE rounding to float32.  For the rows gf_elements.hpp's fp64 moduli cannot settle: an absolute error of a few
// 1e-16 is below a float32 step only down to ~1e-7, and where an entry vanishes the reference does not return 0 but its own rounding
// noise (cos(pi/2 in 80 bits) = 2.7e-20), which the float32 table it histograms keeps.  ~40 000 instructions per row against ~300, so
// only rows with a modulus below GFEL_SMALL come here (gf_elements.hip: a second kernel over the rows the first one marked), and
// only where the plan asks for the float32 table (round32): with round32 off every row keeps gf_elements.hpp's fp64 value.
#pragma once
#include "gf_elements.hpp"
#include "gf_x87.hpp"

namespace gfel {

// v = hi + lo >= 0, a 64-bit significand, rounded once to float32: hi is first made v rounded to odd (53 bits >= 24 + 2), so that
// the conversion's rounding is v's
GFEL_HD double x87_to_f32(gfx87::x87 v)
{
    int64_t b = gfx87::x_bits(v.hi);
    if (v.lo != 0.0) {
        if (v.lo < 0.0) b -= 1;
        b |= 1;
    }
    return (double)(float)gfx87::x_from_bits(b);
}

// the U9 groups of a row again, as the float32 values of the exact moduli; the row's other groups are left as they are
GFEL_HD void element_row_exact(const gf_element_plan& p, const double* in, double* out)
{
    int o = 0;
    for (int g = 0; g < p.ngroups; ++g) {
        const gf_element_group& G = p.group[g];
        if (G.kind == GF_ELEMENT_U9) {
            const double ang[4] = {in[G.col[0]], in[G.col[1]], in[G.col[2]], in[G.col[3]]};
            gfx87::cx87 u[3][3];
            gfx87::angles_to_u(ang, u);
            for (int i = 0; i < 9; ++i) {
                const gfx87::x87 a = gfx87::c_abs(u[i / 3][i % 3]);
                out[o + i] = x87_to_f32(a);
            }
            o += 9;
        } else {
            o += G.kind == GF_ELEMENT_FR3 ? 3 : 1;
        }
    }
}

// one row, both steps (the host build; the device runs them as two kernels)
GFEL_HD void element_row(const gf_element_plan& p, const double* in, double* out)
{
    if (element_row_fast(p, in, out) && p.round32) element_row_exact(p, in, out);
}

}  // namespace gfel
