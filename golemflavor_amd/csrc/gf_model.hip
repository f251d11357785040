// gf_model.hip -- the model: descriptor validation, derivation of the per-run constants and their one upload, the model's stream,
// and its launches on that stream or a caller's.  Host code only; there is deliberately no CPU evaluation path in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "gf_devcache.h"                // large device allocations are cached, not handed back to the driver
#include "gf_host.h"
#include "gf_model.h"
#include "gf_spectrum.h"
#include "gf_table.hpp"

static_assert(GF_MAX_DIM == 16 && GF_MAX_BINS == 64, "header / device constant mismatch");
static_assert(GF_TABLE_MAX_NSIDE == GF_TABLE_NSIDE_LIMIT, "header / gf_table.hpp mismatch");

namespace {

typedef long double ld;
typedef std::complex<long double> cld;

// golemflavor/fr.py:116-162 in the algebraic form, long double, host side only:
// used once per model for the fixed-texture projectors.
void mixing_matrix_ld(const double ang[4], cld u[3][3])
{
    const ld s12_2 = ang[0], c13_4 = ang[1], s23_2 = ang[2], dcp = ang[3];
    const ld c13_2 = std::sqrt(c13_4);
    const ld s12 = std::sqrt(s12_2), c12 = std::sqrt(1.0L - s12_2);
    const ld c13 = std::sqrt(c13_2), s13 = std::sqrt(1.0L - c13_2);
    const ld s23 = std::sqrt(s23_2), c23 = std::sqrt(1.0L - s23_2);
    const cld ep(std::cos(dcp), std::sin(dcp)), em = std::conj(ep);
    u[0][0] = c12 * c13;                       u[0][1] = s12 * c13;                       u[0][2] = s13 * em;
    u[1][0] = -s12 * c23 - c12 * s23 * s13 * ep; u[1][1] = c12 * c23 - s12 * s23 * s13 * ep; u[1][2] = s23 * c13;
    u[2][0] = s12 * s23 - c12 * c23 * s13 * ep;  u[2][1] = -c12 * s23 - s12 * c23 * s13 * ep; u[2][2] = c23 * c13;
}

// golemflavor/fr.py:138-161 angles_to_u operation by operation in long double (np.float128 on x86-64, the same libm):
// U = np.dot(np.dot(p1, p2), p3), np.dot accumulating from zero in index order.  Host side, once per model, for the
// per-model matrices of the unitarity arbitration (gf_unitarity.hip) -- their entries must be the reference's to the
// last bit, not merely to 1e-19.
void angles_to_u_ref_ld(const double ang[4], cld u[3][3])
{
    const ld s12_2 = ang[0], c13_4 = ang[1], s23_2 = ang[2];
    const ld c13_2 = sqrtl(c13_4);
    const ld t12 = asinl(sqrtl(s12_2)), t13 = acosl(sqrtl(c13_2)), t23 = asinl(sqrtl(s23_2));
    const ld c12 = cosl(t12), s12 = sinl(t12), c13 = cosl(t13), s13 = sinl(t13), c23 = cosl(t23), s23 = sinl(t23);
    const ld dcp = ang[3];
    const cld em(cosl(dcp), -sinl(dcp)), ep(cosl(dcp), sinl(dcp));      // EXP(-+1j * dcp)
    auto mul = [](cld a, cld b) { return cld(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); };
    auto dot = [&](const cld a[3][3], const cld b[3][3], cld out[3][3]) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                cld acc(0.0L, 0.0L);
                for (int k = 0; k < 3; ++k) { const cld p = mul(a[i][k], b[k][j]); acc = cld(acc.real() + p.real(), acc.imag() + p.imag()); }
                out[i][j] = acc;
            }
    };
    const cld p1[3][3] = {{1.0L, 0.0L, 0.0L}, {0.0L, c23, s23}, {0.0L, -s23, c23}};
    const cld p2[3][3] = {{c13, 0.0L, cld(s13 * em.real(), s13 * em.imag())}, {0.0L, 1.0L, 0.0L}, {cld(-s13 * ep.real(), -s13 * ep.imag()), 0.0L, c13}};
    const cld p3[3][3] = {{c12, s12, 0.0L}, {-s12, c12, 0.0L}, {0.0L, 0.0L, 1.0L}};
    cld t[3][3];
    dot(p1, p2, t);
    dot(t, p3, u);
}

void split_matrix_ld(const cld u[3][3], double hi[18], double lo[18])
{
    for (int k = 0; k < 9; ++k) {
        const ld v[2] = {u[k / 3][k % 3].real(), u[k / 3][k % 3].imag()};
        for (int q = 0; q < 2; ++q) {
            hi[2 * k + q] = (double)v[q];
            lo[2 * k + q] = (double)(v[q] - (ld)hi[2 * k + q]);
        }
    }
}

bool finite_all(const double* p, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// the NP mixing angles a texture fixes (fr.py:370); false for GF_TEX_NONE, whose angles are the descriptor's
bool texture_angles(int texture, double ang[4])
{
    const double z = 0. + 1e-9;
    switch (texture) {
    case GF_TEX_OEU: ang[0] = 0.5; ang[1] = 1.0; ang[2] = z; ang[3] = z; return true;
    case GF_TEX_OET: ang[0] = z; ang[1] = 0.25; ang[2] = z; ang[3] = z; return true;
    case GF_TEX_OUT: ang[0] = z; ang[1] = 1.0; ang[2] = 0.5; ang[3] = z; return true;
    default: return false;
    }
}

// ---- gf_model_create, stage by stage: everything up to upload_constants works on the host alone ----

int validate_desc(const gf_model_desc* d)
{
    if (d->abi_version != GF_ABI_VERSION)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "descriptor abi_version %d != library %d", d->abi_version, GF_ABI_VERSION);
    if (d->ndim < 1 || d->ndim > GF_MAX_DIM) return GF_ERR_INVALID_ARG;
    if (d->mode < GF_MODE_PRIOR_ONLY || d->mode > GF_MODE_BSM_GAUSS) return GF_ERR_INVALID_ARG;
    auto idx_ok = [&](int i) { return i >= -1 && i < d->ndim; };
    for (int k = 0; k < 4; ++k)
        if (!idx_ok(d->idx_sm[k]) || !idx_ok(d->idx_mm[k])) return GF_ERR_INVALID_ARG;
    for (int k = 0; k < 2; ++k)
        if (!idx_ok(d->idx_mass[k]) || !idx_ok(d->idx_src[k])) return GF_ERR_INVALID_ARG;
    if (!idx_ok(d->idx_scale) || !idx_ok(d->idx_gamma)) return GF_ERR_INVALID_ARG;
    if ((d->idx_src[0] < 0) != (d->idx_src[1] < 0)) return GF_ERR_INVALID_ARG;
    if (!idx_ok(d->idx_src_x) || (d->idx_src_x >= 0 && d->idx_src[0] >= 0)) return GF_ERR_INVALID_ARG;
    if (d->idx_src_x >= 0 && d->mode == GF_MODE_BSM_GAUSS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "an astroX source column is not defined for the flux-averaged (BSM) posterior");
    // CP phases (dcp, and the NP matrix's for texture NONE): the kernels' sine / cosine reduce |x| < GF_PHASE_MAX
    // only (every paramset of the reference boxes them into [0, 2 pi]: scripts/fr.py:41, mc_unitary.py:39)
    auto phase_ok = [&](int idx, double fixed) {
        if (idx >= 0) return std::fabs(d->lo[idx]) <= GF_PHASE_MAX && std::fabs(d->hi[idx]) <= GF_PHASE_MAX;
        return std::fabs(fixed) <= GF_PHASE_MAX;
    };
    if (!phase_ok(d->idx_sm[3], d->sm_fixed[3]) ||
        (d->mode == GF_MODE_BSM_GAUSS && d->texture == GF_TEX_NONE && !phase_ok(d->idx_mm[3], d->mm_fixed[3])))
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "CP phase range or value beyond +-%g is not supported", GF_PHASE_MAX);
    return GF_OK;
}

void set_columns(const gf_model_desc* d, GfCommon& c)
{
    c.ndim = d->ndim;
    c.mode = d->mode;
    for (int k = 0; k < 4; ++k) { c.idx_sm[k] = d->idx_sm[k]; c.idx_mm[k] = d->idx_mm[k]; c.sm_fixed[k] = d->sm_fixed[k]; c.mm_fixed[k] = d->mm_fixed[k]; }
    for (int k = 0; k < 2; ++k) { c.idx_mass[k] = d->idx_mass[k]; c.idx_src[k] = d->idx_src[k]; c.mass_fixed[k] = d->mass_fixed[k]; }
    c.idx_scale = d->idx_scale;
    c.idx_gamma = d->idx_gamma;
    c.idx_src_x = d->idx_src_x;
    c.scale_fixed = d->scale_fixed;
}

// priors: llh.py:81-90 + scipy truncnorm.logpdf = ((-z^2/2 - log sqrt(2pi)) - log_mass) - log(sigma)
int set_priors(const gf_model_desc* d, GfCommon& c)
{
    const double logC = std::log(std::sqrt(2.0 * M_PI));
    double pc = 0.0;
    for (int i = 0; i < d->ndim; ++i) {
        c.lo[i] = d->lo[i];
        c.hi[i] = d->hi[i];
        const int kind = d->prior_kind[i];
        if (kind == GF_PRIOR_UNIFORM) {
            c.loc[i] = 0.0;
            c.inv_sigma[i] = 0.0;
        } else if (kind == GF_PRIOR_GAUSSIAN || kind == GF_PRIOR_LIMITEDGAUSS) {
            if (!(d->sigma[i] > 0.0) || !std::isfinite(d->loc[i]) || !std::isfinite(d->log_mass[i]))
                return gf_fail_msg(GF_ERR_INVALID_ARG, "column %d: Gaussian prior needs finite loc/log_mass and sigma > 0", i);
            c.loc[i] = d->loc[i];
            c.inv_sigma[i] = 1.0 / d->sigma[i];
            pc += ((-logC) - d->log_mass[i]) - std::log(d->sigma[i]);
        } else {
            return GF_ERR_INVALID_ARG;
        }
    }
    c.prior_const = pc;
    return GF_OK;
}

int set_likelihood(const gf_model_desc* d, GfCommon& c)
{
    for (int k = 0; k < 3; ++k) { c.src_fixed[k] = d->source_ratio[k]; c.bf[k] = d->bestfit_fr[k]; }
    c.src_fixed_sum = (d->source_ratio[0] + d->source_ratio[1]) + d->source_ratio[2];
    // multi_gaussian, llh.py:53-54 + scipy _multivariate.py:514-539: cov = smearing^2 I
    if (d->mode != GF_MODE_PRIOR_ONLY) {
        if (!(d->smearing > 0.0) || !finite_all(d->bestfit_fr, 3)) return GF_ERR_INVALID_ARG;
        gf_internal_gauss_consts(d->smearing, &c.inv_smear, &c.gauss_c0, &c.gauss_mh, &c.gauss_k);
    }
    c.offset = d->offset;
    c.flat_llh = d->flat_llh;
    static const double cosc[8] = {2.7117413873509064e-15, -7.641995277350052e-13, 1.605889634387573e-10,
                                   -2.505210587009456e-08, 2.75573191979119e-06, -0.00019841269841110079,
                                   0.008333333333332799, -0.16666666666666657};
    for (int k = 0; k < 8; ++k) c.cosc[k] = cosc[k];
    return GF_OK;
}

// BSM: the energy bins and the fixed texture's projectors
int set_bins(const gf_model_desc* d, GfBsm& b)
{
    if (d->nbins < 1 || d->nbins > GF_MAX_BINS || d->texture < GF_TEX_OEU || d->texture > GF_TEX_NONE) return GF_ERR_INVALID_ARG;
    if (d->texture == GF_TEX_NONE && (d->idx_mm[0] < 0 && !finite_all(d->mm_fixed, 4))) return GF_ERR_INVALID_ARG;
    b.texture = d->texture;
    b.dimension = d->dimension;
    b.nbins = d->nbins;
    for (int k = 0; k < d->nbins; ++k) {
        const double e = std::sqrt(d->bin_edges[k] * d->bin_edges[k + 1]);     // fr.py:413
        if (!(e > 0.0) || !std::isfinite(e)) return GF_ERR_INVALID_ARG;
        b.centre[k] = e;
        b.weight[k] = std::fabs(d->bin_edges[k + 1] - d->bin_edges[k]);        // fr.py:414
        b.inv2e[k] = 1.0 / (2 * e);                                            // fr.py:386
        b.epow[k] = std::pow(e, (double)(d->dimension - 3));                   // fr.py:394
        const double rho = b.epow[k] / b.inv2e[k];
        if (k == 0 || rho > b.rho_max) b.rho_max = rho;
        b.rho[k] = rho;
        b.wsum += b.weight[k];
    }
    double ang[4];
    if (texture_angles(d->texture, ang)) {
        cld u[3][3];
        mixing_matrix_ld(ang, u);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const cld t1 = u[i][1] * std::conj(u[j][1]);
                const cld t2 = u[i][2] * std::conj(u[j][2]);
                b.t1_re[3 * i + j] = (double)t1.real(); b.t1_im[3 * i + j] = (double)t1.imag();
                b.t2_re[3 * i + j] = (double)t2.real(); b.t2_im[3 * i + j] = (double)t2.imag();
            }
    }
    return GF_OK;
}

// Unitarity tiers (gf_bsm_device.hpp).  Tier 1: SM weight a >= 2e-11 -> unitary (80-bit residual <= 1.3e-19 / a
// over 30 000 pairs, tools/uni_weight_bound.py: five-fold margin; no walker with a > 1.1e-13 fails).  Tier 2, the
// fp64 estimate, measured against the 80-bit residual on 180 000 walkers of all (dimension, texture) pairs binned by
// a (tools/uni_estimate_spread.py, profiles/r02/uni_estimate_spread.txt): log10(estimate / residual) lies in
// [-2.2, +2.1] wherever fp64 resolves the SM term (a >= 1e-16) and in [-4.0, +4.5] below -- there the estimate
// acquits only with that margin and never condemns.  (GF_UNI_BAND_DECADES: symmetric override of the resolved
// regime's band, diagnostics; 0 = estimate only.)
void set_tiers(GfBsm& b)
{
    double lo_dec = 2.7, hi_dec = 2.6, lo_nl_dec = 4.6;
    b.uni_a_ok = 2e-11;
    b.uni_a_lin = 1e-16;
    if (const char* e = gf_internal_env("GF_UNI_BAND_DECADES", 1)) {
        const double v = std::atof(e);
        if (v >= 0.0 && v <= 12.0) { lo_dec = hi_dec = lo_nl_dec = v; if (v == 0.0) b.uni_a_lin = 0.0; }
    }
    b.uni_lo = 1e-7 * 2048.0 * std::pow(10.0, -lo_dec);
    b.uni_hi = 1e-7 * 2048.0 * std::pow(10.0, hi_dec);
    b.uni_lo_nl = 1e-7 * 2048.0 * std::pow(10.0, -lo_nl_dec);
    if (gf_internal_env("GF_UNI_NO_WEIGHT_GATE", 1)) b.uni_a_ok = 2.0;              // diagnostics: tier 1 off
    if (const char* e = gf_internal_env("GF_UNI_A_OK", 1)) b.uni_a_ok = std::atof(e);  // diagnostics: tier 1's threshold
    b.uni_own_bins_only = gf_internal_env("GF_UNI_OWN_BINS_ONLY", 1) ? 1 : 0;             // diagnostics: A/B of uni_arbitration_mask
    if (gf_internal_env("GF_UNI_DUMP", 1)) { b.uni_lo = b.uni_lo_nl = -1.0; b.uni_hi = 1e300; }   // diagnostics: fr[0] <- the estimate
}

// per-model matrices of the unitarity arbitration, in the reference's own operation order
void set_arbitration_matrices(const gf_model_desc* d, GfBsm& b)
{
    double np_ang[4];
    if (!texture_angles(d->texture, np_ang))
        for (int k = 0; k < 4; ++k) np_ang[k] = d->mm_fixed[k];                 // used only when idx_mm < 0
    cld u[3][3];
    angles_to_u_ref_ld(np_ang, u);
    split_matrix_ld(u, b.npu_hi, b.npu_lo);
    angles_to_u_ref_ld(d->sm_fixed, u);                                     // fr.py:313, 435
    split_matrix_ld(u, b.smu_hi, b.smu_lo);
}

// one upload: prior table, then (BSM) the bin / texture tables, into the model's constant block
hipError_t upload_constants(gf_model* m)
{
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = pool_block(m->device, &m->d_block);
    if (e != hipSuccess) return e;
    const GfCommon& c = m->c;
    alignas(16) unsigned char img[CONST_BLOCK_BYTES];
    double* tab = reinterpret_cast<double*>(img);
    for (int i = 0; i < GF_MAX_DIM; ++i) {
        tab[4 * i] = c.lo[i]; tab[4 * i + 1] = c.hi[i]; tab[4 * i + 2] = c.loc[i]; tab[4 * i + 3] = c.inv_sigma[i];
    }
    const bool bsm = c.mode == GF_MODE_BSM_GAUSS;
    if (bsm) std::memcpy(img + CONST_BSM_OFFSET, &m->hb, sizeof(GfBsm));
    std::memcpy(img + CONST_COMMON_OFFSET, &c, sizeof(GfCommon));          // kernels that take the constants by pointer
    // stream-ordered, never the null stream: a synchronous hipMemcpy issued while another host thread is
    // capturing a sampler graph fails on this runtime and poisons that capture.  The stream comes from the
    // pool and goes straight back (the model gets its own only when an entry point needs one).
    hipStream_t up = nullptr;
    e = pool_stream(m->device, &up);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_block, img, CONST_BLOCK_BYTES, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    if (up) pool_release(m->device, up, nullptr);
    m->d_ptab = reinterpret_cast<double*>(m->d_block);
    m->d_bsm = bsm ? reinterpret_cast<GfBsm*>(static_cast<unsigned char*>(m->d_block) + CONST_BSM_OFFSET) : nullptr;
    m->d_common = reinterpret_cast<GfCommon*>(static_cast<unsigned char*>(m->d_block) + CONST_COMMON_OFFSET);
    return e;
}

// owns a model under construction: one that holds nothing of the device yet is deleted without a call to the runtime
struct ModelDeleter {
    void operator()(gf_model* m) const { if (m->d_block) gf_model_destroy(m); else delete m; }
};

// One BSM launch with or without the verdict's workspace (the stream's, locked for the duration of the launches)
int launch_bsm_on(gf_model* m, hipStream_t st, const double* d_theta, int layout, int64_t n, int with_llh, double* d_lnprob, double* d_fr,
                  int32_t* d_status, const char* what)
{
    GfUniLease ws;                                     // stays empty without a status array: no verdict, no workspace
    if (d_status) {
        const int rw = pool_lease_workspace(m->device, st, layout, n, &ws);
        if (rw != GF_OK) return rw;
    }
    const hipError_t e = gf_launch_bsm(m->c, m->d_common, m->d_bsm, m->hb.nbins, m->d_ptab, d_theta, layout, n, with_llh, d_lnprob, d_fr, d_status,
                                       ws.d_uq, ws.uq_items, ws.d_wq, ws.wq_cap, ws.d_t2sn, ws.h_seen, m->cus, st);
    return e != hipSuccess ? gf_hip_fail(e, what) : GF_OK;
}

}  // namespace

int launch_lnprob(gf_model* m, hipStream_t st, const double* d_theta, int layout, int64_t n, double* d_lnprob, double* d_fr,
                  int32_t* d_status)
{
    if (n == 0) return GF_OK;
    if (m->table_nside > 0) {
        // DESIGN.md 6m.  The verdict is the propagate launch's, first on the same stream as for a binned model; k_bsm_table reads the
        // status it left and writes the composition it looks up (the propagate launch's, bit for bit) over that launch's
        if (d_status) {
            const int rc = launch_bsm_on(m, st, d_theta, layout, n, 0, nullptr, d_fr, d_status, "table lnprob: propagate launch");
            if (rc != GF_OK) return rc;
        }
        const hipError_t e = gf_launch_bsm_table(m->c, m->d_common, m->d_bsm, m->d_ptab, m->d_table, m->table_nside, d_theta, layout, n, d_lnprob,
                                                 d_fr, d_status, m->cus, st);
        return e != hipSuccess ? gf_hip_fail(e, "table lnprob launch") : GF_OK;
    }
    if (m->binned) {
        // DESIGN.md 6i.  The verdict (and the flux-averaged composition, if asked for) is the propagate launch's, first on the same
        // stream as in gf_propagate_bins; k_bsm_binned reads the status it left and turns it into lnprob's
        if (d_status || d_fr) {
            const int rc = launch_bsm_on(m, st, d_theta, layout, n, 0, nullptr, d_fr, d_status, "binned lnprob: propagate launch");
            if (rc != GF_OK) return rc;
        }
        const hipError_t e = gf_launch_bsm_binned(m->c, m->d_common, m->d_bsm, m->hb.nbins, m->d_ptab, m->d_btab, d_theta, layout, n, d_lnprob,
                                                  d_fr, d_status, m->cus, st);
        return e != hipSuccess ? gf_hip_fail(e, "binned lnprob launch") : GF_OK;
    }
    if (m->c.mode == GF_MODE_BSM_GAUSS) return launch_bsm_on(m, st, d_theta, layout, n, 1, d_lnprob, d_fr, d_status, "lnprob launch");
    const hipError_t e = gf_launch_lnprob_sm(m->c, m->d_ptab, d_theta, layout, n, d_lnprob, d_fr, d_status, m->cus, st);
    return e != hipSuccess ? gf_hip_fail(e, "lnprob launch") : GF_OK;
}

int launch_propagate(gf_model* m, hipStream_t st, const double* d_theta, int layout, int64_t n, double* d_fr, int32_t* d_status)
{
    if (n == 0) return GF_OK;
    if (m->c.mode == GF_MODE_BSM_GAUSS) return launch_bsm_on(m, st, d_theta, layout, n, 0, nullptr, d_fr, d_status, "propagate launch");
    const hipError_t e = gf_launch_propagate_sm(m->c, d_theta, layout, n, d_fr, d_status, m->cus, st);
    return e != hipSuccess ? gf_hip_fail(e, "propagate launch") : GF_OK;
}

int ensure_stream(gf_model* m)
{
    GF_HIP(hipSetDevice(m->device));
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->stream) return GF_OK;
    const hipError_t e = pool_stream(m->device, &m->stream);
    return e != hipSuccess ? gf_hip_fail(e, "hipStreamCreate") : GF_OK;
}

extern "C" {

// multi_gaussian, llh.py:53-54 + scipy _multivariate.py:514-539 for cov = smearing^2 I (gf_reweight.hip builds a measurement target's
// constants with it, so that they are the bits a model of that measurement holds)
void gf_internal_gauss_consts(double smearing, double* inv_smear, double* c0, double* mh, double* k)
{
    const double s = std::pow(smearing, 2);
    *inv_smear = std::sqrt(1.0 / s);
    *c0 = 3.0 * std::log(2.0 * M_PI) + ((std::log(s) + std::log(s)) + std::log(s));
    *mh = -0.5 * (*inv_smear * *inv_smear);
    *k = -0.5 * *c0;
}

int gf_model_create(const gf_model_desc* d, int device, gf_model** out)
{
    if (!d || !out) return GF_ERR_INVALID_ARG;
    *out = nullptr;
    gf_internal_set_error("");
    int rc = validate_desc(d);
    if (rc != GF_OK) return rc;
    std::unique_ptr<gf_model, ModelDeleter> m(new (std::nothrow) gf_model());
    if (!m) return GF_ERR_ALLOC;
    std::memset(&m->c, 0, sizeof(m->c));
    std::memset(&m->hb, 0, sizeof(m->hb));
    set_columns(d, m->c);
    rc = set_priors(d, m->c);
    if (rc == GF_OK) rc = set_likelihood(d, m->c);
    if (rc == GF_OK && d->mode == GF_MODE_BSM_GAUSS) {
        rc = set_bins(d, m->hb);
        if (rc == GF_OK) { set_tiers(m->hb); set_arbitration_matrices(d, m->hb); }
    }
    if (rc != GF_OK) return rc;
    // the last validation is behind us: from here on the device
    rc = pool_device(device, &m->cus);
    if (rc != GF_OK) return rc;
    m->device = device;
    const hipError_t e = upload_constants(m.get());
    if (e != hipSuccess) return gf_hip_fail(e, "gf_model_create");
    *out = m.release();
    return GF_OK;
}

void gf_model_destroy(gf_model* m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    pool_release(m->device, m->stream, m->d_block);
    if (m->d_theta) (void)gf_cached_free(m->d_theta);
    if (m->d_out) (void)gf_cached_free(m->d_out);
    if (m->d_status) (void)gf_cached_free(m->d_status);
    if (m->h_pin) (void)hipHostFree(m->h_pin);
    for (int k = 0; k < 2; ++k) {
        if (m->ev_up[k]) (void)hipEventDestroy(m->ev_up[k]);
        if (m->ev_down[k]) (void)hipEventDestroy(m->ev_down[k]);
    }
    if (m->d_cube) (void)gf_cached_free(m->d_cube);
    if (m->d_btab) (void)gf_cached_free(m->d_btab);
    if (m->d_table) (void)gf_cached_free(m->d_table);
    for (double* t : m->tables_retired) (void)gf_cached_free(t);
    delete m;
}

int gf_model_ndim(const gf_model* m) { return m ? m->c.ndim : -1; }
int gf_model_nbins(const gf_model* m) { return !m ? -1 : m->c.mode == GF_MODE_BSM_GAUSS ? m->hb.nbins : 0; }

// the per-bin measurement of a BSM model.  Everything is validated before the model is touched; the table
// {m_k[3], mh_k, k_k} is built on the host with the constants gf_model_create derives for a smearing, and uploaded stream-ordered on
// a pool stream (never the null stream: see upload_constants) behind whatever the model's own stream still has in flight.
int gf_model_set_binned_measurement(gf_model* m, int nbins, const double* fr_bins, const double* sigma)
{
    if (!m || !fr_bins || !sigma) return GF_ERR_INVALID_ARG;
    gf_internal_set_error("");
    if (m->c.mode != GF_MODE_BSM_GAUSS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_model_set_binned_measurement: the model has no energy bins (mode %d)", m->c.mode);
    if (m->table_nside > 0)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_model_set_binned_measurement: the model carries a tabulated likelihood (side %d)", m->table_nside);
    if (nbins != m->hb.nbins)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_binned_measurement: %d bins given, the model has %d", nbins, m->hb.nbins);
    double tab[GF_BINNED_STRIDE * GF_MAX_BINS];
    for (int k = 0; k < nbins; ++k) {
        if (!finite_all(fr_bins + 3 * k, 3) || !(sigma[k] > 0.0) || !std::isfinite(sigma[k]))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_binned_measurement: bin %d needs a finite composition and a width > 0", k);
        double inv_smear, c0;
        double* t = tab + GF_BINNED_STRIDE * k;
        t[0] = fr_bins[3 * k]; t[1] = fr_bins[3 * k + 1]; t[2] = fr_bins[3 * k + 2];
        gf_internal_gauss_consts(sigma[k], &inv_smear, &c0, &t[3], &t[4]);
        if (!std::isfinite(t[3]) || !std::isfinite(t[4]))
            return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_binned_measurement: the width of bin %d is outside the range of the Gaussian's constants", k);
    }
    std::lock_guard<std::mutex> lk(m->call_mu);
    GF_HIP(hipSetDevice(m->device));
    if (m->stream) GF_HIP(hipStreamSynchronize(m->stream));              // a replaced table may still be read there
    double* d = m->d_btab;
    if (!d) GF_HIP(gf_cached_malloc((void**)&d, sizeof(double) * GF_BINNED_STRIDE * GF_MAX_BINS));
    hipStream_t up = nullptr;
    hipError_t e = pool_stream(m->device, &up);
    if (e == hipSuccess) e = hipMemcpyAsync(d, tab, sizeof(double) * GF_BINNED_STRIDE * (size_t)nbins, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);                   // `tab` goes out of scope
    if (up) pool_release(m->device, up, nullptr);
    if (e != hipSuccess) {
        if (!m->d_btab) (void)gf_cached_free(d);
        return gf_hip_fail(e, "gf_model_set_binned_measurement");
    }
    m->d_btab = d;
    m->binned = 1;
    m->likelihood_sets += 1;
    return GF_OK;
}

int gf_model_is_binned(const gf_model* m) { return !m ? -1 : m->binned; }

int gf_model_binned(gf_model* m, const double** d_btab)
{
    if (d_btab) *d_btab = m && m->binned ? m->d_btab : nullptr;
    return m && m->binned ? 1 : 0;
}

// ln L at the nodes of the flavour triangle's lattice of side `nside` (gf_table.hpp).  Everything is validated before the
// model is touched; the upload is stream-ordered on a pool stream behind whatever the model's own stream still has in flight.
int gf_model_set_table_likelihood(gf_model* m, int nside, const double* values)
{
    if (!m || !values) return GF_ERR_INVALID_ARG;
    gf_internal_set_error("");
    if (m->c.mode != GF_MODE_BSM_GAUSS)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_model_set_table_likelihood: a table replaces the flux-averaged (BSM) Gaussian only (mode %d)", m->c.mode);
    if (m->binned)
        return gf_fail_msg(GF_ERR_UNSUPPORTED, "gf_model_set_table_likelihood: the model carries a binned measurement");
    if (nside < 1 || nside > GF_TABLE_MAX_NSIDE)
        return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_table_likelihood: side %d outside 1 .. %d", nside, GF_TABLE_MAX_NSIDE);
    const int64_t nodes = gftab::node_count(nside);
    bool any_finite = false;
    for (int64_t k = 0; k < nodes; ++k) {
        const double v = values[k];
        if (v != v || v == HUGE_VAL)
            return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_table_likelihood: node %lld is %s; a node is finite or -inf", (long long)k,
                               v != v ? "NaN" : "+inf");
        any_finite = any_finite || v != -HUGE_VAL;
    }
    if (!any_finite) return gf_fail_msg(GF_ERR_INVALID_ARG, "gf_model_set_table_likelihood: every node is -inf");
    std::lock_guard<std::mutex> lk(m->call_mu);
    GF_HIP(hipSetDevice(m->device));
    if (m->stream) GF_HIP(hipStreamSynchronize(m->stream));              // a replaced table may still be read there
    double* d = m->d_table;
    const bool grow = nodes > m->table_cap;
    if (grow) {
        d = nullptr;
        GF_HIP(gf_cached_malloc((void**)&d, sizeof(double) * (size_t)nodes));
    }
    hipStream_t up = nullptr;
    hipError_t e = pool_stream(m->device, &up);
    if (e == hipSuccess) e = hipMemcpyAsync(d, values, sizeof(double) * (size_t)nodes, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);                   // `values` is the caller's
    if (up) pool_release(m->device, up, nullptr);
    if (e != hipSuccess) {
        if (grow) (void)gf_cached_free(d);
        return gf_hip_fail(e, "gf_model_set_table_likelihood");
    }
    if (grow) {
        if (m->d_table) m->tables_retired.push_back(m->d_table);
        m->d_table = d;
        m->table_cap = nodes;
    }
    m->table_nside = nside;
    m->likelihood_sets += 1;
    return GF_OK;
}

int gf_model_table_nside(const gf_model* m) { return m ? m->table_nside : 0; }

int gf_model_table(gf_model* m, const double** d_table)
{
    const int ns = m ? m->table_nside : 0;
    if (d_table) *d_table = ns > 0 ? m->d_table : nullptr;
    return ns;
}

uint64_t gf_model_likelihood_sets(const gf_model* m) { return m ? m->likelihood_sets : 0; }

// internal (not in the public header): gf_modelset.hip reaches the model's constants and stream through these
int gf_model_internal(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, void** stream, int* device)
{
    if (!m) return GF_ERR_INVALID_ARG;
    GF_STREAM(m);
    *c = &m->c; *d_bsm = m->d_bsm; *d_ptab = m->d_ptab; *stream = (void*)m->stream; *device = m->device;
    return GF_OK;
}

// constants only: does not give the model a stream
int gf_model_constants(gf_model* m, const GfCommon** c, const GfBsm** d_bsm, const double** d_ptab, int* device, int* cus,
                       int* nbins)
{
    if (!m) return GF_ERR_INVALID_ARG;
    *c = &m->c; *d_bsm = m->d_bsm; *d_ptab = m->d_ptab; *device = m->device; *cus = m->cus;
    *nbins = m->c.mode == GF_MODE_BSM_GAUSS ? m->hb.nbins : 0;
    return GF_OK;
}

// the work items one pass of a bulk launch's capped grid covers on the model's device (gf_grid_for): a launch of more takes the
// kernels' stride loops round again.  The tests of those loops size their batches from this.
int gf_internal_pass_items(gf_model* m, int64_t* items)
{
    if (!m || !items) return GF_ERR_INVALID_ARG;
    *items = gf_pass_items(m->cus);
    return GF_OK;
}

void gf_model_peek_stream(const gf_model* m, int* device, void** stream)
{
    *device = m->device;
    *stream = (void*)m->stream;
}

// the model's kernels on a stream of the caller's (the sampler's)
int gf_model_lnprob_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_lnprob,
                       double* d_fr, int32_t* d_status)
{
    if (!m || n < 0) return GF_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(m->call_mu);
    return launch_lnprob(m, (hipStream_t)stream, d_theta, layout, n, d_lnprob, d_fr, d_status);
}

int gf_model_propagate_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_fr,
                          int32_t* d_status)
{
    if (!m || n < 0) return GF_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(m->call_mu);
    return launch_propagate(m, (hipStream_t)stream, d_theta, layout, n, d_fr, d_status);
}

// the composition at every energy bin (gf_spectrum.hip) on a stream of the caller's; values only, so no workspace and no lock
int gf_model_bins_on(gf_model* m, void* stream, const double* d_theta, int layout, int64_t n, double* d_fr_bins, int bin_major,
                     const int32_t* d_status)
{
    if (!m || n < 0) return GF_ERR_INVALID_ARG;
    if (m->c.mode != GF_MODE_BSM_GAUSS || m->hb.nbins < 1) return GF_ERR_UNSUPPORTED;
    const hipError_t e = gf_launch_bsm_bins(m->c, m->d_common, m->d_bsm, m->hb.nbins, m->d_ptab, d_theta, layout, n, d_fr_bins, bin_major,
                                            d_status, m->cus, (hipStream_t)stream);
    return e != hipSuccess ? gf_hip_fail(e, "bins launch") : GF_OK;
}

// internal, test hook (tests/test_gpu_x87_device.py): the model's own inputs of the emulated-x87 chain as the kernels read them --
// smu / npu split into (hi, lo) (18 doubles each, row-major (re, im) pairs), inv2e and epow (nbins doubles each; *nbins <- the count)
int gf_internal_bsm_tables(gf_model* m, double* smu_hi, double* smu_lo, double* npu_hi, double* npu_lo, double* inv2e, double* epow,
                           int* nbins)
{
    if (!m || !smu_hi || !smu_lo || !npu_hi || !npu_lo || !inv2e || !epow || !nbins || m->c.mode != GF_MODE_BSM_GAUSS) return GF_ERR_INVALID_ARG;
    const GfBsm& b = m->hb;
    std::memcpy(smu_hi, b.smu_hi, sizeof(b.smu_hi)); std::memcpy(smu_lo, b.smu_lo, sizeof(b.smu_lo));
    std::memcpy(npu_hi, b.npu_hi, sizeof(b.npu_hi)); std::memcpy(npu_lo, b.npu_lo, sizeof(b.npu_lo));
    std::memcpy(inv2e, b.inv2e, sizeof(double) * b.nbins); std::memcpy(epow, b.epow, sizeof(double) * b.nbins);
    *nbins = b.nbins;
    return GF_OK;
}

}  // extern "C"
