// gf_elements.hpp -- a sampled row in element space: the nine moduli |U_ij| from the four mixing columns and the source
// composition from the two source columns, i.e. the table golemflavor/plot.py:528-567 (chainer_plot, --plot-elements) builds from
// a chain with flat_angles_to_u (fr.py:165-167) and angles_to_fr (fr.py:82-113) before it draws the triangle.
//
// Compiles for the device (hipcc: gf_elements.hip; gf_device.hpp takes sincos_cw and angles_to_fr from here) and for the host
// (tests/elements/elements_host.cpp, g++ with contraction off): every fused multiply-add is written as fma(), nothing else can be
// contracted, so the two builds differ only where the square root does (below).  The library never evaluates this on the host.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/golemflavor_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GFEL_HD __host__ __device__ __forceinline__
#else
#define GFEL_HD inline
#endif

namespace gfel {

GFEL_HD double el_nan() { return __builtin_nan(""); }

// sqrt for x in [0, ~1e300).  Device: v_rsq_f64 seed + two Newton-Raphson (Goldschmidt) refinements, no denormal scaling, <= 1 ulp;
// x == 0 -> 0; x < 0 or NaN -> NaN.  Host: the correctly rounded one.
GFEL_HD double el_sqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    const double d = fma(-g, g, x);
    g = fma(d, h, g);
    return x == 0.0 ? 0.0 : g;
#else
    return std::sqrt(x);
#endif
}

// sin and cos of x, |x| < 2^20 * pi/2: three-step Cody-Waite reduction with FMA (33-bit pieces of pi/2, the published fdlibm
// split), then the fdlibm minimax kernels on [-pi/4, pi/4].  Absolute error <= ~2e-16.  Larger |x| (never a physical phase) and
// NaN give NaN.
GFEL_HD void sincos_cw(double x, double* sn, double* cs)
{
    if (!(fabs(x) < 1.6e6)) { *sn = el_nan(); *cs = el_nan(); return; }
    const double fn = rint(x * 6.36619772367581382433e-01);          // x * 2/pi
    double r = fma(-fn, 1.57079632673412561417e+00, x);              // pio2_1 (33 bits)
    r = fma(-fn, 6.07710050630396597660e-11, r);                     // pio2_2 (33 bits)
    r = fma(-fn, 2.02226624879595063154e-21, r);                     // pio2_2t: the rest of pi/2
    const int q = (int)fn;
    const double z = r * r;
    double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = fma(z, ps, 2.75573137070700676789e-06);
    ps = fma(z, ps, -1.98412698298579493134e-04);
    ps = fma(z, ps, 8.33333333332248946124e-03);
    ps = fma(z, ps, -1.66666666666666324348e-01);
    const double s = fma(r * z, ps, r);
    double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = fma(z, pc, -2.75573143513906633035e-07);
    pc = fma(z, pc, 2.48015872894767294178e-05);
    pc = fma(z, pc, -1.38888888888741095749e-03);
    pc = fma(z, pc, 4.16666666666666019037e-02);
    const double c = fma(z * z, pc, fma(-0.5, z, 1.0));
    // quadrant: (sin, cos)(x) = (s, c), (c, -s), (-s, -c), (-c, s) for q mod 4 = 0, 1, 2, 3
    const double ss = (q & 1) ? c : s;
    const double cc = (q & 1) ? s : c;
    *sn = (q & 2) ? -ss : ss;
    *cs = ((q + 1) & 2) ? -cc : cc;
}

// golemflavor/fr.py:82-113 angles_to_fr: (sin^4 phi, cos 2psi) -> composition.  sin^2(acos(c)/2) = (1-c)/2 exactly, so no
// trigonometry is needed.  No float32 cast (fr.py:110-112 is float(abs(..))).
GFEL_HD void angles_to_fr(double sphi4, double c2psi, double f[3])
{
    const double sphi2 = el_sqrt(sphi4);
    const double spsi2 = 0.5 * (1.0 - c2psi);
    const double cpsi2 = 1.0 - spsi2;
    f[0] = fabs(sphi2 * cpsi2);
    f[1] = fabs(sphi2 * spsi2);
    f[2] = fabs(1.0 - sphi2);
}

// |U_ij|, row-major e1 ... tau3, of U = P1 P2 P3 (fr.py:157-161 angles_to_u) from (s12^2, c13^4, s23^2, delta):
//   U_e.   = ( c12 c13,                        s12 c13,                        s13 e^{-id} )
//   U_mu.  = ( -c23 s12 - s23 s13 c12 e^{id},  c23 c12 - s23 s13 s12 e^{id},   s23 c13 )
//   U_tau. = (  s23 s12 - c23 s13 c12 e^{id}, -s23 c12 - c23 s13 s12 e^{id},   c23 c13 )
// Each entry's real and imaginary parts are formed from the six sines and cosines and cos d, sin d, then the modulus is taken:
// |U|^2 formed algebraically (gf_device.hpp pmns_abs2) and rooted loses half the digits where an entry vanishes.  The reference
// reaches the sines and cosines through asin / acos / sin / cos in 80-bit arithmetic; here they are square roots of values that are
// exact or well conditioned over the whole box:
//   c12^2 = 1 - s12^2 and c23^2 = 1 - s23^2    exact above 1/2 (Sterbenz), one rounding of a value >= 1/2 below it;
//   c13 = sqrt(sqrt(c13^4));
//   s13^2 = 1 - sqrt(x) = (1 - x) / (1 + sqrt(x)),  x = c13^4: the difference 1 - sqrt(x) itself cancels as x -> 1.
// The absolute error of every modulus is a few 1e-16 (measured: profiles/elements/README.txt).  A NaN, a value of the first three
// outside [0, 1] or a phase beyond sincos_cw's range gives NaN in all nine.
GFEL_HD void angles_to_absu(double s12_2, double c13_4, double s23_2, double dcp, double m[9])
{
    double sd, cd;
    sincos_cw(dcp, &sd, &cd);
    const bool ok = s12_2 >= 0.0 && s12_2 <= 1.0 && c13_4 >= 0.0 && c13_4 <= 1.0 && s23_2 >= 0.0 && s23_2 <= 1.0 && sd == sd;
    if (!ok) {
        for (int i = 0; i < 9; ++i) m[i] = el_nan();
        return;
    }
    const double s12 = el_sqrt(s12_2), c12 = el_sqrt(1.0 - s12_2);
    const double c13_2 = el_sqrt(c13_4);
    const double c13 = el_sqrt(c13_2), s13 = el_sqrt((1.0 - c13_4) / (1.0 + c13_2));
    const double s23 = el_sqrt(s23_2), c23 = el_sqrt(1.0 - s23_2);
    const double p1 = (s23 * s13) * c12, p2 = (s23 * s13) * s12;      // the e^{id} terms of the mu row
    const double q1 = (c23 * s13) * c12, q2 = (c23 * s13) * s12;      // ... of the tau row
    double re, im;
    m[0] = c12 * c13;
    m[1] = s12 * c13;
    m[2] = s13;
    re = fma(p1, cd, c23 * s12); im = p1 * sd;
    m[3] = el_sqrt(fma(re, re, im * im));
    re = fma(-p2, cd, c23 * c12); im = p2 * sd;
    m[4] = el_sqrt(fma(re, re, im * im));
    m[5] = s23 * c13;
    re = fma(-q1, cd, s23 * s12); im = q1 * sd;
    m[6] = el_sqrt(fma(re, re, im * im));
    re = fma(q2, cd, s23 * c12); im = q2 * sd;
    m[7] = el_sqrt(fma(re, re, im * im));
    m[8] = c23 * c13;
}

// The plan's output width for rows of width_in columns, or -1 where the plan is invalid: no group or more than
// GF_ELEMENT_MAX_WIDTH of them, an unknown kind, a column outside [0, width_in), more than GF_ELEMENT_MAX_WIDTH output columns.
inline int plan_width(const gf_element_plan* p, int width_in)
{
    if (!p || width_in < 1 || width_in > GF_MAX_DIM || p->ngroups < 1 || p->ngroups > GF_ELEMENT_MAX_WIDTH) return -1;
    int w = 0;
    for (int g = 0; g < p->ngroups; ++g) {
        const gf_element_group& G = p->group[g];
        const int nin = G.kind == GF_ELEMENT_COPY ? 1 : G.kind == GF_ELEMENT_U9 ? 4 : G.kind == GF_ELEMENT_FR3 ? 2 : 0;
        if (!nin) return -1;
        for (int k = 0; k < nin; ++k)
            if (G.col[k] < 0 || G.col[k] >= width_in) return -1;
        w += G.kind == GF_ELEMENT_COPY ? 1 : G.kind == GF_ELEMENT_U9 ? 9 : 3;
    }
    return w <= GF_ELEMENT_MAX_WIDTH ? w : -1;
}

// A modulus below this sends its row to gf_elements_exact.hpp: a float32 step there (>= 2^-44) is above the fp64 moduli's absolute
// error only down to ~1e-7, with a margin of 8 here.
#define GFEL_SMALL 9.5367431640625e-07      /* 2^-20 */

// One row: `in` [width_in] -> `out` [plan_width].  Returns whether a U9 group of the row has a modulus below GFEL_SMALL.  The plan's fields are read at uniform indices (scalar loads on the device).
// The moduli are written as (double)(float)v where round32 is set: the reference's table holds np.float32 values (fr.py:167).
// A NaN in either source column makes all three fractions NaN (angles_to_fr alone leaves phi_tau finite for a NaN cos 2psi).
GFEL_HD bool element_row_fast(const gf_element_plan& p, const double* in, double* out)
{
    int o = 0;
    bool small = false;
    for (int g = 0; g < p.ngroups; ++g) {
        const gf_element_group& G = p.group[g];
        if (G.kind == GF_ELEMENT_U9) {
            double m[9];
            angles_to_absu(in[G.col[0]], in[G.col[1]], in[G.col[2]], in[G.col[3]], m);
            for (int i = 0; i < 9; ++i) {
                small = small || m[i] < GFEL_SMALL;
                out[o + i] = p.round32 ? (double)(float)m[i] : m[i];
            }
            o += 9;
        } else if (G.kind == GF_ELEMENT_FR3) {
            const double a = in[G.col[0]], b = in[G.col[1]];
            double f[3];
            angles_to_fr(a, b, f);
            const bool bad = a != a || b != b;
            for (int i = 0; i < 3; ++i) out[o + i] = bad ? el_nan() : f[i];
            o += 3;
        } else {
            out[o++] = in[G.col[0]];
        }
    }
    return small;
}

}  // namespace gfel
