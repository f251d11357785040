"""Host side of the nested sampler (golemflavor_amd.nested, golemflavor_amd.sens, configs.sens_paramsets): the evidence
accounting against an exact problem, the sens.py paramsets, scale list and file names, the Bayes-factor limit, the CLI and
the C declarations.  No GPU needed."""
import ast
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import nested
from golemflavor_amd.enums import ParamTag, PriorsCateg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. evidence_from_dead on a problem with exact constrained draws --------------------------------------------------------
def _exact_nested(rng, n, sigma, nlive, b, tol=0.01, f=0.0):
    """Nested sampling of L = N(u; c, sigma^2 I) on [0,1]^n with EXACT constrained draws: {L > L*} is a ball around c (cut by
    the cube), sampled uniformly by rejection.  Where u_0 < f the likelihood is zero (lnL = -inf): a plateau of prior mass f,
    and c_0 sits mid-way in [f, 1].  Same removal, start and termination rules as the device (nested.nlive_sequence: the
    i-th plateau point of the run sees nlive - i live points).  Returns (evidence_from_dead, nlive_seq, dead lnL,
    final live lnL)."""
    c = np.full(n, 0.5)
    c[0] = 0.5 * (1.0 + f)
    lnorm = -0.5 * n * math.log(2 * math.pi * sigma * sigma)

    def lnl(u):
        out = lnorm - 0.5 * np.sum((u - c) ** 2, axis=-1) / (sigma * sigma)
        return np.where(u[..., 0] < f, -np.inf, out)

    def draw(k, lstar):
        out = []
        rho = math.inf if lstar == -math.inf else math.sqrt(max(2 * sigma * sigma * (lnorm - lstar), 0.0))
        while len(out) < k:
            if rho > 0.5 * (1.0 - f):
                u = rng.uniform(size=(4 * k, n))
                u[:, 0] = f + (1.0 - f) * u[:, 0]
            else:
                d = rng.normal(size=(4 * k, n))
                d /= np.linalg.norm(d, axis=1)[:, None]
                u = c + d * (rho * rng.uniform(size=(4 * k, 1)) ** (1.0 / n))
            inside = np.all((u >= 0) & (u <= 1), axis=1) & (u[:, 0] >= f) & (np.sum((u - c) ** 2, axis=1) < rho * rho)
            out.extend(u[inside])
        return np.array(out[:k])

    live = rng.uniform(size=(nlive, n))
    ll = lnl(live)
    dead, seq = [], []
    lnz, lnx, nplat = -math.inf, 0.0, 0
    while True:
        lmax = ll.max()
        if lnz > -math.inf and np.logaddexp(lnz, lmax + lnx) - lnz < tol:
            break
        order = np.argsort(ll, kind="stable")[:b]
        for j, i in enumerate(order):
            nl = nlive - (nplat if ll[i] == -math.inf else j)
            nplat += ll[i] == -math.inf
            dx = 1.0 / nl
            lnz = np.logaddexp(lnz, ll[i] + lnx + math.log(-math.expm1(-dx)))
            lnx -= dx
            dead.append(ll[i])
            seq.append(nl)
        new = draw(b, ll[order[-1]])
        live[order] = new
        ll[order] = lnl(new)
    return nested.evidence_from_dead(dead, seq, live_lnl=ll), np.array(seq), np.array(dead), ll


def _exact_lnz(n, sigma, f):
    """ln of the integral of N(u; c, sigma^2 I) over [f, 1] x [0, 1]^(n-1), c as in _exact_nested."""
    half = 0.5 * (1.0 - f)
    return math.log(math.erf(half / (sigma * math.sqrt(2)))) + (n - 1) * math.log(math.erf(0.5 / (sigma * math.sqrt(2))))


@pytest.mark.parametrize("batch_of", [lambda k: 1, lambda k: k // 8], ids=["b1", "b_nlive_over_8"])
def test_evidence_from_dead_exact_problem(batch_of):
    n, sigma, nlive = 3, 0.05, 160
    exact = n * math.log(math.erf(0.5 / (sigma * math.sqrt(2))))
    assert abs(_exact_lnz(n, sigma, 0.0) - exact) < 1e-15
    for seed in range(4):
        res, seq, dead, live = _exact_nested(np.random.default_rng(seed), n, sigma, nlive, batch_of(nlive))
        err = math.sqrt(res["info"] / nlive)
        assert res["info"] > 1.0 and abs(res["lnz_err"] - err) < 1e-15 and res["plateau_var"] == 0.0
        assert abs(res["lnz"] - exact) < 4 * err, (seed, res["lnz"], exact, err)
        assert seq.min() == nlive - batch_of(nlive) + 1
        assert np.array_equal(seq, nested.nlive_sequence(dead, nlive, batch_of(nlive)))


@pytest.mark.parametrize("f", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("batch_of", [lambda k: 1, lambda k: k // 8], ids=["b1", "b_nlive_over_8"])
def test_evidence_with_a_zero_likelihood_plateau(f, batch_of):
    """A region of prior mass f where L = 0: ln Z within 4 sigma of the closed form, sigma including the plateau's compression
    variance.  The old per-batch rule (every removal of an iteration sees nlive - j, plateau or not) is off by about
    -1.06 f - ln(1 - f) for a batch of nlive / 8: more than 4 sigma at f = 0.9."""
    n, sigma, nlive = 3, 0.03, 400
    b = batch_of(nlive)
    exact = _exact_lnz(n, sigma, f)
    for seed in range(4):
        res, seq, dead, live = _exact_nested(np.random.default_rng(100 + seed), n, sigma, nlive, b, f=f)
        nd = len(dead)
        plat = dead == -np.inf
        assert np.array_equal(seq, nested.nlive_sequence(dead, nlive, b))
        if f == 0.0:
            assert not plat.any() and res["plateau_var"] == 0.0
        else:
            k = int(plat.sum())
            assert plat[:k].all() and not plat[k:].any()             # the plateau comes first
            assert abs(k / nlive - f) < 5 * math.sqrt(f * (1 - f) / nlive), (k, f)
            assert np.array_equal(seq[:k], nlive - np.arange(k))
            assert res["plateau_var"] == pytest.approx(np.sum(1.0 / seq[:k].astype(float) ** 2), rel=1e-12)
        sig = math.sqrt(res["info"] / nlive + res["plateau_var"])
        assert res["lnz_err"] == pytest.approx(sig, rel=1e-12)
        assert abs(res["lnz"] - exact) < 4 * sig, (f, seed, res["lnz"], exact, sig)
        if f == 0.9 and b > 1:
            old = nested.evidence_from_dead(dead, np.tile(nlive - np.arange(b), nd // b), live_lnl=live)
            assert old["lnz"] - exact > 4 * sig, (seed, old["lnz"], exact, sig)


def test_evidence_from_dead_accounting_small_cases():
    # one dead point seen by 2 live points, then a live set of one: Z = L0 (1 - e^-1/2) + L1 e^-1/2
    r = nested.evidence_from_dead([math.log(2.0)], [2], live_lnl=[math.log(5.0)])
    assert abs(math.exp(r["lnz"]) - (2 * (1 - math.exp(-0.5)) + 5 * math.exp(-0.5))) < 1e-14
    assert abs(r["lnx"] + 0.5) < 1e-15
    # -inf points carry no weight but still shrink X
    r = nested.evidence_from_dead([-math.inf, 0.0], [3, 2])
    assert abs(math.exp(r["lnz"]) - math.exp(-1 / 3) * (1 - math.exp(-0.5))) < 1e-14
    assert r["plateau_var"] == 1 / 9 and r["lnz_err"] == math.sqrt(r["info"] / 3 + 1 / 9)
    # the plateau is counted without replacement across batches; finite points keep the per-batch rule
    inf = -math.inf
    seq = nested.nlive_sequence([inf, inf, inf, inf, inf, 1.0, 2.0, 3.0], 10, 3)
    assert seq.tolist() == [10, 9, 8, 7, 6, 8, 10, 9]
    assert nested.nlive_sequence([1.0, 2.0, 3.0, 4.0], 5, 2).tolist() == [5, 4, 5, 4]


# ---- 2. sens.py:34-108 paramsets, scale list and output paths ----------------------------------------------------------------
SENS_NUISANCE = [  # scripts/sens.py:40-66: name, value, seed, ranges, std, prior, tag
    ("s_12_2", 0.307, [0.26, 0.35], [0., 1.], 0.013, PriorsCateg.LIMITEDGAUSS, ParamTag.SM_ANGLES),
    ("c_13_4", (1 - 0.02206) ** 2, [0.950, 0.961], [0., 1.], 0.00147, PriorsCateg.LIMITEDGAUSS, ParamTag.SM_ANGLES),
    ("s_23_2", 0.538, [0.31, 0.75], [0., 1.], 0.069, PriorsCateg.LIMITEDGAUSS, ParamTag.SM_ANGLES),
    ("dcp", 4.08404, [1e-9, 2 * np.pi - 1e-9], [0., 2 * np.pi], 2.0, PriorsCateg.UNIFORM, ParamTag.SM_ANGLES),
    ("m21_2", 7.40E-23, [7.2E-23, 7.6E-23], [6.80E-23, 8.02E-23], 2.1E-24, PriorsCateg.GAUSSIAN, ParamTag.SM_ANGLES),
    ("m3x_2", 2.494E-21, [2.46E-21, 2.53E-21], [2.399E-21, 2.593E-21], 3.3E-23, PriorsCateg.GAUSSIAN, ParamTag.SM_ANGLES),
    ("convNorm", 1., [0.5, 2.], [0.1, 10.], 0.4, PriorsCateg.LIMITEDGAUSS, ParamTag.NUISANCE),
    ("promptNorm", 0., [0., 6.], [0., 20.], 2.4, PriorsCateg.LIMITEDGAUSS, ParamTag.NUISANCE),
    ("muonNorm", 1., [0.1, 2.], [0., 10.], 0.1, PriorsCateg.UNIFORM, ParamTag.NUISANCE),
    ("astroNorm", 8.0, [0., 5.], [0., 20.], 1.5, PriorsCateg.UNIFORM, ParamTag.NUISANCE),
    ("astroDeltaGamma", 2.5, [2.4, 3.], [-5., 5.], 0.1, PriorsCateg.UNIFORM, ParamTag.NUISANCE),
]


def _check_param(p, name, value, seed, ranges, std, prior, tag):
    assert p.name == name
    assert p.value == pytest.approx(value, rel=1e-15, abs=0)
    assert list(p.seed) == pytest.approx(seed, rel=1e-15)
    assert list(p.ranges) == pytest.approx(ranges, rel=1e-15)
    assert p.std == pytest.approx(std, rel=1e-15)
    assert p.prior == prior and p.tag == tag


@pytest.mark.parametrize("dimension", [3, 6, 8])
@pytest.mark.parametrize("injected", [(1, 1, 1), (1, 2, 0), (0, 1, 0)])
def test_sens_paramsets_match_reference(dimension, injected):
    asimov, llh = Cf.sens_paramsets(dimension, injected)
    assert list(llh.names) == [r[0] for r in SENS_NUISANCE] + ["logLam"]
    for p, row in zip(llh, SENS_NUISANCE):
        _check_param(p, *row)
    sc = llh[11]
    b = Cf.SCALE_BOUNDARIES[dimension]
    assert sc.tag == ParamTag.SCALE and sc.std == 3 and sc.prior == PriorsCateg.UNIFORM
    assert tuple(sc.ranges) == tuple(b) and sc.value == np.mean(b)
    # asimov: the NUISANCE-tagged params (same values), then the two flavor angles of the normalised injected ratio
    assert list(asimov.names) == [r[0] for r in SENS_NUISANCE[6:]] + ["astroFlavorAngle1", "astroFlavorAngle2"]
    for p, row in zip(asimov, SENS_NUISANCE[6:]):
        _check_param(p, *row)
    ang = fr_utils.fr_to_angles(np.asarray(injected, float) / np.sum(injected))
    _check_param(asimov[5], "astroFlavorAngle1", ang[0], [0., 1.], [0., 1.], 0.2, PriorsCateg.UNIFORM, ParamTag.BESTFIT)
    _check_param(asimov[6], "astroFlavorAngle2", ang[1], [-1., 1.], [-1., 1.], 0.2, PriorsCateg.UNIFORM, ParamTag.BESTFIT)
    real, _ = Cf.sens_paramsets(dimension, injected, data="REAL")
    assert tuple(real.from_tag(ParamTag.BESTFIT, values=True)) == pytest.approx(fr_utils.fr_to_angles([1, 1, 1]))


def test_fr_paramsets_unchanged_by_the_astro_norm_option():
    _, ps = Cf.fr_paramsets(6, (0.5, 0.0))
    assert ps["astroNorm"].value == 6.9


@pytest.mark.parametrize("dimension,segments", [(3, 10), (6, 10), (6, 4), (8, 2)])
def test_sens_scale_list(dimension, segments):
    b = Cf.SCALE_BOUNDARIES[dimension]
    ref = np.concatenate([[-100.], np.linspace(b[0], b[1], segments - 1)])      # sens.py:226-229
    assert np.array_equal(nested.sens_scales(dimension, segments), ref)


def test_sens_output_paths_follow_reference_naming(golden_meta):
    from golemflavor_amd import sens
    rows = ast.literal_eval(golden_meta["g16_identifiers"]) if isinstance(golden_meta["g16_identifiers"], str) \
        else golden_meta["g16_identifiers"]
    checked = 0
    for row in rows:
        if row["texture"] == "NONE":
            continue
        # sens.py names its files after the NORMALISED ratios (process_args runs before gen_identifier); the golden identifiers
        # were made from the raw ones, so only the rows where normalising does not change the name apply
        from golemflavor_amd.mcmc import solve_ratio
        if any(solve_ratio(fr_utils.normalize_fr(np.asarray(row[k], float))) != solve_ratio(row[k])
               for k in ("source_ratio", "injected_ratio") if k == "source_ratio" or row["data"] != "REAL"):
            continue
        checked += 1
        argv = ["--dimension", str(row["dimension"]), "--texture", row["texture"], "--data", row["data"], "--datadir", "/d",
                "--source-ratio", *map(str, row["source_ratio"]), "--injected-ratio", *map(str, row["injected_ratio"])]
        a = sens.parse_args(argv)
        stat, llh = sens.output_paths(a)
        base = "/d/bayesian/{0}/".format(row["data"].lower())
        assert stat == base + "fr_stat" + row["identifier"]
        assert llh == base + "fr_maxllh" + row["identifier"]
        a = sens.parse_args(argv + ["--eval-segment", "3", "--segments", "10"])
        sc = nested.sens_scales(row["dimension"], 10)[3]
        assert sens.output_paths(a)[0] == base + "fr_stat" + row["identifier"] + "_scale_{0:.0E}".format(10 ** sc)
    assert checked >= 3


# ---- 3. Bayes-factor limit -----------------------------------------------------------------------------------------------------
def test_bayes_factor_limit_linear_curve():
    scales = np.linspace(-56, -30, 9)
    for slope in (0.5, 1.0, 2.0):
        st = -slope * (scales - scales[0])
        lim = nested.bayes_factor_limit(scales, st)
        # collinear, evenly spaced points: the interpolating parametric spline is the line itself
        cross = scales[0] + math.log(10.) / slope
        assert lim is not None
        assert cross - np.log10(2.) <= lim + 1e-9 <= cross - np.log10(2.) + 26.0 / 999 + 1e-9, (slope, lim, cross)


def test_bayes_factor_limit_none_cases():
    scales = np.concatenate([[-100.], np.linspace(-56, -30, 9)])
    # nothing crosses ln(10)
    assert nested.bayes_factor_limit(scales, np.zeros(10) - 0.01 * np.arange(10)) is None
    # a dip that comes back: the large scales are not excluded
    st = np.zeros(10)
    st[3] = -6.0
    assert nested.bayes_factor_limit(scales, st) is None
    # only the last scanned point lies beyond the threshold
    st = np.zeros(10)
    st[-1] = -5.0
    assert nested.bayes_factor_limit(scales, st) is None
    # evidence rising above the null: the reference's 'Discovered LV!' test compares statistic[0] - max (never > 0) with
    # ln(10^K), so it cannot fire; nothing crosses downwards either
    st = np.zeros(10)
    st[5:] = 4.0
    assert nested.bayes_factor_limit(scales, st) is None


# ---- 4. CLI and C declarations ---------------------------------------------------------------------------------------------------
def test_sens_cli_help():
    out = subprocess.run([sys.executable, "-m", "golemflavor_amd.sens", "--help"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--dimension", "--texture", "--source-ratio", "--injected-ratio", "--segments", "--eval-segment", "--seed",
                "--datadir", "--overwrite", "--mn-live-points", "--mn-tolerance"):
        assert opt in out.stdout


def test_nested_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    for name in ("gf_nested_create", "gf_nested_run", "gf_nested_result", "gf_nested_get_dead", "gf_nested_destroy",
                 "gf_nested_set_run_ids", "gf_nested_set_tolerance"):
        assert name + "(" in hdr and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


def test_nested_create_validates_before_touching_the_device():
    import ctypes as C
    L = _lib.lib()
    h = C.c_void_p()
    cols = (C.c_int32 * 1)(0)
    base = (C.c_double * 2)(0.0, 0.0)
    models = (C.c_void_p * 1)(None)
    # batch must lie in [1, nlive); nlive <= 4096; on_nonunitary 0 or 1; a model handle
    assert L.gf_nested_create(models, 1, 1, cols, base, 100, 100, 25, 0, 0, C.byref(h)) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_create(models, 1, 1, cols, base, 5000, 10, 25, 0, 0, C.byref(h)) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_create(models, 1, 1, cols, base, 100, 10, 25, 0, 2, C.byref(h)) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_create(models, 1, 1, cols, base, 100, 10, 25, 0, 0, C.byref(h)) == _lib.GF_ERR_INVALID_ARG
