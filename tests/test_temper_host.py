"""Host side of the tempered sampler: the header's declarations against the binding and the library's exports, the
estimators of golemflavor_amd/tempering.py on a problem sampled exactly, the closed-form prior mass against quadratures of the oracle's
lnprior, and the host build of csrc/gf_temper.hpp.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from scipy.special import log_ndtr, ndtr

import temper_harness as TH
from golemflavor_amd import _lib, tempering
from golemflavor_amd.enums import ParamTag, PriorsCateg
from golemflavor_amd.param import Param, ParamSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("gf_model_lnprior_lnl", "gf_model_lnprior_lnl_device", "gf_sampler_create_tempered", "gf_sampler_tempered_series",
               "gf_sampler_swap_counts", "gf_sampler_betas")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    L = _lib.lib()
    assert L.gf_abi_version() == 5
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), "%s is not declared" % name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == args
    m = re.search(r"^int\s+gf_sampler_create_tempered\s*\(([^)]*)\)\s*;", hdr, re.M)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["gf_model* const* models", "int nmodels", "int ngroups", "int ntemps", "const double* betas", "int nwalkers", "uint64_t seed",
                      "double a", "int swap_every", "gf_sampler** out"]
    assert len(_lib.SIGNATURES["gf_sampler_create_tempered"][1]) == len(params)
    # every symbol is additive: the descriptor is the one ABI 5 has had
    assert L.gf_sizeof_model_desc() == C.sizeof(_lib.GfModelDesc) == 1480


def test_entry_points_refuse_null_handles():
    L = _lib.lib()
    assert L.gf_sampler_betas(None, None, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_sampler_swap_counts(None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_sampler_tempered_series(None, None, None, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_model_lnprior_lnl(None, None, 0, None, None, None) == _lib.GF_ERR_INVALID_ARG
    out = C.c_void_p()
    assert L.gf_sampler_create_tempered(None, 1, 1, 1, None, 24, 0, 2.0, 0, C.byref(out)) == _lib.GF_ERR_INVALID_ARG


# ---- the command line ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, says", [
    (["--stat-method", "frequentist"], "needs the Bayesian method"),
    (["--energy-resolved"], "flux-averaged likelihood only"),
    (["--posterior", "--datadir", "d"], "does not combine with"),
    (["--evidence-realisations", "4"], "does not combine with"),
    (["--temperatures", "64"], "--temperatures takes 1 to 63"),
    (["--beta-min", "1.0"], "--beta-min a value in (0, 1)"),
    (["--tempered-walkers", "23"], "--tempered-walkers"),
])
def test_sens_argument_errors(extra, says, capsys):
    from golemflavor_amd import sens
    with pytest.raises(SystemExit) as e:
        sens.parse_args(["--evidence-method", "stepping-stone"] + extra)
    assert e.value.code == 2
    assert says in capsys.readouterr().err


def test_sens_file_name_and_defaults():
    from golemflavor_amd import sens
    args = sens.parse_args(["--evidence-method", "stepping-stone", "--datadir", "dd"])
    assert (args.temperatures, args.beta_min, args.swap_every, args.tempered_steps) == (8, 1e-3, 8, 1500)
    stat = sens.output_paths(args)[0]
    f = sens.evidence_tempered_path(args)
    assert os.path.dirname(f) == os.path.dirname(stat) and os.path.basename(f) == "fr_evidence_tempered" + sens.identifier(args) + ".npz"
    one = sens.parse_args(["--evidence-method", "stepping-stone", "--datadir", "dd", "--eval-segment", "2"])
    assert os.path.basename(sens.evidence_tempered_path(one)).startswith("fr_evidence_tempered" + sens.identifier(one) + "_scale_")
    assert sens.parse_args([]).evidence_method == "nested"


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------
def test_geometric_ladder_shapes():
    b = tempering.geometric_ladder(8, 1e-3)
    assert b.shape == (9,) and b[0] == 1.0 and b[-2] == 1e-3 and b[-1] == 0.0
    assert np.all(np.diff(b) < 0)
    assert np.allclose(b[1:8] / b[0:7], 1e-3 ** (1 / 7), rtol=1e-12)
    assert np.array_equal(tempering.geometric_ladder(1, 0.5), [1.0, 0.0])
    assert np.array_equal(tempering.geometric_ladder(2, 0.25), [1.0, 0.25, 0.0])
    for bad in ((0, 0.1), (4, 0.0), (4, 1.0), (4, -0.5)):
        with pytest.raises(ValueError):
            tempering.geometric_ladder(*bad)


# ---- the estimators on a problem sampled exactly ------------------------------------------------------------------------------------------
# x ~ U(0, 1), L(x) = exp(-(x - MU)^2 / (2 S^2)): Z(beta) = S sqrt(2 pi / beta) (Phi(b) - Phi(a)) with a, b the box in units of
# S / sqrt(beta) around MU; the tempered posterior is that truncated Gaussian, the prior chain the uniform itself.
MU, S = 0.3, 0.05


def ln_z_exact(beta):
    if beta == 0.0:
        return 0.0
    s = S / math.sqrt(beta)
    return math.log(s * math.sqrt(2 * math.pi) * (ndtr((1.0 - MU) / s) - ndtr((0.0 - MU) / s)))


def draw_tempered(rng, beta, n):
    if beta == 0.0:
        return rng.uniform(0.0, 1.0, n)
    s = S / math.sqrt(beta)
    lo, hi = ndtr((0.0 - MU) / s), ndtr((1.0 - MU) / s)
    from scipy.special import ndtri
    return MU + s * ndtri(rng.uniform(lo, hi, n))


def synthetic_series(betas, nsteps, nw, seed, plant=None):
    """(ntemps, nsteps, 5) by the host build of gf_temper.hpp with the exponents `lnl_series()` uses, from independent draws"""
    rng = np.random.default_rng(seed)
    out = np.empty((len(betas), nsteps, 5))
    for k, b in enumerate(betas):
        x = draw_tempered(rng, b, nsteps * nw).reshape(nsteps, nw)
        lnl = -(x - MU) ** 2 / (2 * S * S)
        if plant is not None and k == plant:
            lnl[3, 5] = -np.inf
        d_up = betas[k - 1] - b if k > 0 else 0.0
        d_dn = b - betas[k + 1] if k + 1 < len(betas) else 0.0
        out[k] = TH.host_series(lnl, d_up, d_dn)
    return out


def test_stepping_stone_on_an_exactly_sampled_problem():
    betas = tempering.geometric_ladder(6, 1e-2)
    nw = 64
    ser = synthetic_series(betas, 400, nw, seed=5)
    est = tempering.stepping_stone(ser, betas, nbatch=16, nwalkers=nw)
    want = ln_z_exact(1.0) - ln_z_exact(0.0)
    err = est["ln_ratio_err"][0]
    print("stepping stone: %.5f +- %.5f, closed form %.5f; thermodynamic %.5f" % (est["ln_ratio"][0], err, want, est["ln_ratio_ti"][0]))
    assert 0 < err < 0.05
    assert abs(est["ln_ratio"][0] - want) <= 5 * err
    assert est["rungs"].shape == (1, 6) and np.allclose(est["rungs"][0].sum(), est["ln_ratio"][0])
    for k in range(6):
        rung = ln_z_exact(betas[k]) - ln_z_exact(betas[k + 1])
        assert abs(est["rungs"][0, k] - rung) <= 5 * est["rungs_err"][0, k] + 1e-12, k
    assert np.all(est["nonfinite_fraction"] == 0)
    assert np.isfinite(est["ln_ratio_ti"][0])
    # the trapezoid on seven rungs is a coarse quadrature of a steep integrand: finite, and of the right sign and size only
    assert est["ln_ratio_ti"][0] < 0
    # two groups are two independent estimates, and discard drops steps from the front
    two = tempering.stepping_stone(np.concatenate([ser, synthetic_series(betas, 400, nw, seed=6)]), betas, nwalkers=nw)
    assert two["ln_ratio"].shape == (2,) and two["ln_ratio"][0] == est["ln_ratio"][0] and two["ln_ratio"][1] != est["ln_ratio"][0]
    cut = tempering.stepping_stone(ser, betas, discard=100, nwalkers=nw)
    assert cut["ln_ratio"][0] != est["ln_ratio"][0] and abs(cut["ln_ratio"][0] - want) <= 5 * cut["ln_ratio_err"][0]


def test_a_planted_minus_infinity_makes_the_thermodynamic_integral_nan_and_leaves_stepping_stone_alone():
    betas = tempering.geometric_ladder(6, 1e-2)
    nw = 64
    clean = tempering.stepping_stone(synthetic_series(betas, 200, nw, seed=7), betas, nwalkers=nw)
    est = tempering.stepping_stone(synthetic_series(betas, 200, nw, seed=7, plant=6), betas, nwalkers=nw)     # in the prior chain
    assert np.isfinite(clean["ln_ratio_ti"][0]) and np.isnan(est["ln_ratio_ti"][0])
    assert est["nonfinite_fraction"][0, 6] == 1.0 / (200 * nw) and np.all(est["nonfinite_fraction"][0, :6] == 0)
    # L = 0 contributes 0 to the mean of L^(delta beta): one sample of 12 800 moves the estimate by about 1 / 12 800 of a rung's mean
    assert np.isfinite(est["ln_ratio"][0]) and abs(est["ln_ratio"][0] - clean["ln_ratio"][0]) < 1e-3
    assert abs(est["ln_ratio"][0] - (ln_z_exact(1.0) - ln_z_exact(0.0))) <= 5 * est["ln_ratio_err"][0]


# ---- the prior's mass ------------------------------------------------------------------------------------------------------------------------
def prior_paramset(ndim):
    """LIMITEDGAUSS, UNIFORM and GAUSSIAN columns in turn on boxes of different widths and offsets (the construction of
    tests/test_gpu_nested_exact.py, restated)"""
    kinds = [PriorsCateg.LIMITEDGAUSS, PriorsCateg.UNIFORM, PriorsCateg.GAUSSIAN]
    ps = []
    for i in range(ndim):
        lo, w = -1.0 + 0.37 * i, 1.0 + 0.25 * (i % 4)
        ps.append(Param(name="x%d" % i, value=lo + w * (0.35 + 0.03 * (i % 5)), ranges=[lo, lo + w], std=w * (0.12 + 0.02 * (i % 3)),
                        prior=kinds[i % 3], tag=ParamTag.NUISANCE))
    return ParamSet(ps)


def quadrature_lnz(oracle, ps, n=200001):
    """ln of the integral over the unit cube of exp(lnprior(theta(u))): lnprior is a sum over columns, so the product over the columns
    of 1-D midpoint quadratures of the oracle's PRIOR_ONLY lnprob along that column, the others held at a reference point"""
    om = oracle.make_model(ps, "PRIOR_ONLY", flat_llh=0.0)
    r = np.array(ps.ranges, dtype=np.float64)
    ref = np.array(ps.values, dtype=np.float64)
    lp0 = oracle.lnprob_batch(om, ref[None, :])[0]
    total = lp0
    u = (np.arange(n) + 0.5) / n
    for c in range(len(ps)):
        th = np.tile(ref, (n, 1))
        th[:, c] = (r[c, 1] - r[c, 0]) * u + r[c, 0]
        lp = oracle.lnprob_batch(om, th)
        m = lp.max()
        total += m + math.log(np.mean(np.exp(lp - m))) - lp0
    return total


@pytest.mark.parametrize("ndim", [1, 3, 7])
def test_prior_log_mass_against_quadratures_of_the_oracles_lnprior(oracle, ndim):
    ps = prior_paramset(ndim)
    got = tempering.ln_z0(ps)
    want = quadrature_lnz(oracle, ps)
    print("ndim %d: closed form %.12f, quadrature %.12f" % (ndim, got, want))
    assert abs(got - want) <= 1e-9
    # a truncated Gaussian is normalised over its box, a uniform column contributes 0: only the unbounded Gaussians lose mass
    lost = sum(math.log(ndtr((p.ranges[1] - p.nominal_value) / p.std) - ndtr((p.ranges[0] - p.nominal_value) / p.std))
               for p in ps if p.prior is PriorsCateg.GAUSSIAN)
    assert abs(tempering.prior_log_mass(ps) - lost) <= 1e-12
    assert tempering.prior_log_mass(ParamSet([p for p in ps if p.prior is PriorsCateg.UNIFORM])) == 0.0


def test_prior_log_mass_in_a_far_tail():
    """a box eight sigma out: log_ndtr's range, where Phi(b) - Phi(a) has lost every digit"""
    p = Param(name="x", value=0.0, ranges=[8.0, 10.0], std=1.0, prior=PriorsCateg.GAUSSIAN, tag=ParamTag.NUISANCE)    # nominal value 0
    want = log_ndtr(-8.0) + math.log1p(-math.exp(log_ndtr(-10.0) - log_ndtr(-8.0)))
    assert abs(tempering.prior_log_mass(ParamSet([p])) - want) <= 1e-12 * abs(want)


# ---- the host build of gf_temper.hpp ---------------------------------------------------------------------------------------------------------
def test_the_swap_draws_counter_is_never_a_stretch_draws():
    """The step word of a stretch draw is 2 * iteration + half: below 2^63 for iteration < 2^62.  The swap draw's has bit 63 set, the
    rung in bits 56..61 and the round below: the two words differ in bit 63 whatever the walker words are."""
    L = TH.build()
    assert L.tph_max_temps() == 64
    rounds = [0, 1, 2, 7, (1 << 56) - 1, 1 << 56, (1 << 63) - 1]
    its = [0, 1, 5, (1 << 31), (1 << 62) - 1]
    for it in its:
        for half in (0, 1):
            w = L.tph_stretch_step_word(it, half)
            assert w == 2 * it + half and w < (1 << 63)
    seen = set()
    for r in rounds:
        for t in (0, 1, 31, 62):
            w = L.tph_swap_step_word(r, t)
            assert w >> 63 == 1 and (w >> 56) & 0x3F == t and w & ((1 << 56) - 1) == r & ((1 << 56) - 1)
            assert w == TH.swap_step_word(r, t)
            seen.add(w)
    assert len(seen) == 4 * len({r & ((1 << 56) - 1) for r in rounds})
    assert L.tph_swap_walker_word(3, 24, 5) == 3 * 24 + 5


def test_the_swap_draw_and_the_walkers_scalar(oracle):
    L = TH.build()
    for seed, gsid, nw, w, r, t in ((7, 0, 24, 0, 0, 0), (2 ** 40 + 3, 5, 100, 99, 12, 3), (11, 2 ** 33, 24, 7, 2 ** 40, 62)):
        u = L.tph_swap_uniform(seed, gsid * nw + w, TH.swap_step_word(r, t))
        assert 0.0 < u < 1.0 and u == TH.swap_uniform(oracle, seed, gsid, nw, w, r, t)
    rng = np.random.default_rng(3)
    for lp, lnl, beta in zip(rng.normal(-5, 3, 200), rng.normal(-300, 50, 200), rng.uniform(0, 1, 200)):
        assert L.tph_temper(lp, lnl, beta) == float(TH.temper(lp, lnl, beta))
        assert L.tph_temper(lp, lnl, 1.0) == lp + lnl
    assert L.tph_temper(-3.0, -np.inf, 0.0) == -3.0                       # the prior chain: no product
    assert L.tph_temper(-3.0, -np.inf, 0.5) == -np.inf
    assert L.tph_swap_log_ratio(1.0, 0.25, -10.0, -4.0) == 0.75 * 6.0
    assert np.isnan(L.tph_swap_log_ratio(0.5, 0.0, -np.inf, -np.inf))


def test_series_of_the_host_build():
    """the five outputs against their definitions in np.longdouble; a step without a finite lnl; NaN counts as non-finite"""
    rng = np.random.default_rng(9)
    for nw in (24, 100, 257, 600):
        lnl = rng.normal(-330.0, 8.0, size=(6, nw))
        lnl[1, ::3] = -np.inf
        lnl[2, 0] = np.nan
        lnl[3, :] = -np.inf
        out = TH.host_series(lnl, 0.75, 0.125)
        for s in range(6):
            fin = np.isfinite(lnl[s])
            assert out[s, 0] == fin.sum()
            if not fin.any():
                assert out[s, 1] == 0 and out[s, 2] == -np.inf and out[s, 3] == 0 and out[s, 4] == 0
                continue
            x = lnl[s][fin].astype(np.longdouble)
            assert out[s, 2] == lnl[s][fin].max()
            assert abs(out[s, 1] - float(x.sum())) <= 1e-13 * abs(float(x.sum()))
            for col, d in ((3, 0.75), (4, 0.125)):
                want = float(np.exp(np.longdouble(d) * (x - x.max())).sum())
                assert abs(out[s, col] - want) <= 1e-12 * want
    one = TH.host_series(np.full((1, 24), -3.0), 0.0, 2.0)
    assert one[0].tolist() == [24.0, -72.0, -3.0, 24.0, 24.0]
