"""The evidence of a nested run under other measurements, on the host (no GPU): the g++ build of gf_ns_toys.hpp against Python --
the tree sum against math.fsum, the classification rules, the definitions against numpy on a crafted run --, the limits of an
ensemble row by row, the header and the binding, and the driver's parser."""
import math
import os
import re

import numpy as np
import pytest

import ns_toys_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import nested
from golemflavor_amd import realisations as R
from golemflavor_amd import sens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
NU = 2                                   # GF_ST_NON_UNITARY


@pytest.mark.parametrize("n", [1, 255, 256, 257, H.LEAF - 1, H.LEAF, H.LEAF + 1, 2 * H.LEAF + 77, 257 * H.LEAF + 5])
def test_tree_sum_against_fsum(n):
    rng = np.random.default_rng(n)
    e = np.exp(-rng.exponential(8.0, n))                    # weights exp(x - max x): a few near 1, most small
    got, exact = H.host_tree_sum(e), math.fsum(e.tolist())
    bound = H.tree_depth(n) * H.U * exact                   # all terms positive: sum |e| = the sum
    print("n = %d: tree sum off by %.3e, bound %.3e" % (n, abs(got - exact), bound))
    assert abs(got - exact) <= bound


def test_classification_table():
    x = H.build().nth_x
    assert x(-3.0, -2.0, -5.0, 0) == -3.0 + (-5.0 - -2.0)
    assert x(-3.0, -2.0, -2.0, 0) == -3.0                                    # the run's own measurement: x = lnw exactly
    assert x(-0.1, -2.5, -2.5, 1) == -0.1                                    # a status other than non-unitary keeps the point
    for lnw, l0, lt, st in [(-INF, -2.0, -5.0, 0),                          # lnw = -inf
                            (-3.0, -2.0, -5.0, NU),                          # the reference would have raised
                            (-3.0, -INF, -5.0, 0), (-3.0, INF, -5.0, 0), (-3.0, NAN, -5.0, 0),     # l0 not finite
                            (-3.0, -2.0, -INF, 0), (-3.0, -2.0, NAN, 0),     # lt -inf or NaN
                            (-INF, -INF, -INF, NU), (-INF, -2.0, INF, 0), (-INF, NAN, NAN, 0)]:
        assert x(lnw, l0, lt, st) == -INF, (lnw, l0, lt, st)
    assert x(-3.0, -2.0, INF, 0) == INF                                      # gf_reweight.hpp keeps lt = +inf; a Gaussian never gives it
    ess = H.build().nth_ess
    assert ess(0.0, 0.0, 0) == 0.0 and ess(3.0, 2.0, 5) == 4.5


def crafted_run(n, seed, smearing=0.05):
    """lnw, fr, status of a run-shaped point set: lnw rising as a run's, a plateau of -inf in front, a few non-unitary points, some
    compositions far enough for every Gaussian to be -inf."""
    rng = np.random.default_rng(seed)
    fr = np.array([1 / 3, 1 / 3, 1 / 3]) + 1.5 * smearing * rng.standard_normal((n, 3))
    lnw = np.sort(rng.normal(-30.0, 10.0, n))
    status = np.zeros(n, np.int32)
    pick = rng.random(n)
    lnw[: n // 20] = -INF
    status[(pick > 0.9) & (pick < 0.93)] = NU
    fr[pick > 0.97] += 2.0
    return lnw, fr, status


@pytest.mark.parametrize("n", [700, H.LEAF, H.LEAF + 1, 2 * H.LEAF + 300])
def test_host_build_against_numpy(n):
    lnw, fr, status = crafted_run(n, n)
    sm = np.array([0.05, 0.05, 0.07, 0.06])
    bf = np.array([[1 / 3, 1 / 3, 1 / 3], [0.36, 0.31, 0.33], [0.30, 0.38, 0.32], [5.0, 5.0, 5.0]])   # the run's own first; the last is out of reach
    meas, off = H.consts(bf, sm), -320.0
    got = H.host_evidence(lnw, fr, status, meas[0], meas, off, want_x=True)
    l0 = H.host_gauss(fr, meas[0], off)
    for t in range(4):
        lt = H.host_gauss(fr, meas[t], off)
        with np.errstate(invalid="ignore"):
            want = np.where(np.isfinite(lnw) & (status != NU) & np.isfinite(l0) & ~np.isnan(lt) & (lt != -INF), lnw + (lt - l0), -INF)
        assert H.same_bits(got["x"][t], want), t
        assert got["kept"][t] == np.isfinite(want).sum()
        if not np.isfinite(want).any():
            assert t == 3 and got["m"][t] == -INF and got["s"][t] == 0.0 and got["s2"][t] == 0.0 and got["ess"][t] == 0.0
            assert nested.evidence_lnz(got["m"][t:t + 1], got["s"][t:t + 1])[0] == -INF
            continue
        assert got["m"][t] == want.max()
        e = np.exp(want - want.max())
        s, s2 = math.fsum(e.tolist()), math.fsum((e * e).tolist())
        tol = (H.tree_depth(n) + 4) * H.U                    # the tree's bound and the header's exp (below one ulp)
        assert abs(got["s"][t] - s) <= tol * s and abs(got["s2"][t] - s2) <= 2 * tol * s2
        assert got["ess"][t] == got["s"][t] * got["s"][t] / got["s2"][t]
    assert H.same_bits(got["x"][0], np.where(np.isfinite(got["x"][0]), lnw, -INF))          # own measurement: x = lnw where kept
    empty = H.host_evidence(lnw[:0], fr[:0], status[:0], meas[0], meas[:1], off)
    assert np.isnan(empty["m"][0]) and np.isnan(empty["s"][0]) and empty["ess"][0] == 0.0 and empty["kept"][0] == 0


def test_limits_row_by_row():
    scales = nested.sens_scales(6, 8)
    fall = np.array([0.0, 0.0, 0.0, -0.2, -1.0, -4.0, -8.0, -12.0])         # crosses ln 10 and stays below: a limit
    flat = np.array([0.0, -0.1, -0.2, -0.1, -0.3, -0.2, -0.4, -0.3])          # never falls by ln 10: none
    lnz = np.stack([fall - 7.0, flat + 3.0, fall - 7.0])
    lnz[2, 2] = NAN                                                           # a row with a hole has no limit
    got = R.evidence_limits(scales, lnz)
    want = nested.bayes_factor_limit(scales, lnz[0])
    assert want is not None and got["limits"][0] == want
    assert nested.bayes_factor_limit(scales, lnz[1]) is None and np.isnan(got["limits"][1]) and np.isnan(got["limits"][2])
    assert not got["discovered"].any() and not got["low_ess"].any()
    assert R.evidence_limits(scales, lnz, k=1.5)["limits"][0] == nested.bayes_factor_limit(scales, lnz[0], 1.5) != want
    # get_limit raises 'Discovered LV!' where lnz[0] - max(lnz) > ln 10^k, which takes k < 0: at k = -0.5 a null point within 1.15 of
    # the best scale raises, a curve with one point above it has a limit, one with two such points has none
    one = np.array([0.0, 2.0, 0.5, -0.9, -1.8, -3.0, -4.5, -6.0])
    two = np.array([0.0, 2.0, 2.0, -0.9, -1.8, -3.0, -4.5, -6.0])
    rows = np.stack([one, two, fall])
    got = R.evidence_limits(scales, rows, k=-0.5)
    want = nested.bayes_factor_limit(scales, one, -0.5)
    assert want is not None and got["limits"][0] == want
    assert nested.bayes_factor_limit(scales, two, -0.5) is None and np.isnan(got["limits"][1])
    with pytest.raises(AssertionError, match="Discovered LV!"):
        nested.bayes_factor_limit(scales, fall, -0.5)
    assert np.isnan(got["limits"][2]) and got["discovered"].tolist() == [False, False, True]
    frac = np.ones((3, 8))
    frac[0, 5] = 0.01
    cut = R.evidence_limits(scales, rows, k=-0.5, ess_fraction=frac, min_ess_fraction=0.05)
    assert cut["low_ess"].tolist() == [True, False, False] and np.isnan(cut["limits"][0]) and cut["discovered"][2]
    assert not R.evidence_limits(scales, rows, k=-0.5, ess_fraction=frac)["low_ess"].any()             # off by default
    band = R.sensitivity_band(got["limits"])
    assert band["n"] == 3 and band["n_without_limit"] == 2 and band["limits"][2] == want


def test_save_evidence_realisations(tmp_path):
    T, S = 3, 4
    res = dict(scales=nested.sens_scales(6, S), measurements=np.zeros((T, 3)), smearings=np.full(T, 0.1), lnz=np.zeros((T, S)), ess=np.ones((T, S)),
               ess_fraction=np.ones((T, S)), kept=np.ones((T, S), np.int64), lnz_run=np.zeros(S), lnz_err_run=np.ones(S), ess_run=np.ones(S),
               bayes=np.zeros((T, S)), limits=np.array([-30.0, NAN, -31.0]), discovered=np.zeros(T, bool), low_ess=np.zeros(T, bool),
               seconds=1.0, seconds_nested=0.9, seconds_reweight=0.1)
    band = R.save_evidence_realisations(str(tmp_path / "e.npz"), res)
    z = np.load(str(tmp_path / "e.npz"))
    assert set(R.EVIDENCE_SAVED) <= set(z.files) and z["band_without_limit"] == 1 and np.array_equal(z["band_limits"], band["limits"])
    assert z["band_limits"][2] == -30.5


def test_header_and_binding_declare_the_entry_point():
    with open(os.path.join(ROOT, "include", "golemflavor_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define GF_ABI_VERSION 5\b", text) and _lib.GF_ABI_VERSION == 5
    decl = re.search(r"int gf_nested_toys_evidence\(([^;]*)\);", text)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert [a.rsplit(" ", 1)[0].strip() for a in args] == ["gf_nested*", "const double*", "const double*", "int", "int", "double*", "double*",
                                                           "double*", "double*", "int64_t*"]
    restype, argtypes = _lib.SIGNATURES["gf_nested_toys_evidence"]
    assert restype is _lib.C.c_int and len(argtypes) == 10 and argtypes[3] is _lib.C.c_int and argtypes[9] is _lib._lp


BASE = ["--segments", "4"]


def _refused(argv, capsys):
    with pytest.raises(SystemExit):
        sens.parse_args(argv)
    return capsys.readouterr().err


def test_parser(capsys):
    a = sens.parse_args(BASE + ["--evidence-realisations", "3", "--realisation-seed", "2"])
    assert a.evidence_realisations == 3 and a.realisation_seed == 2 and a.realisations is None
    assert sens.parse_args(BASE).evidence_realisations is None
    assert "Bayesian" in _refused(BASE + ["--evidence-realisations", "3", "--stat-method", "frequentist"], capsys)
    assert "T >= 1" in _refused(BASE + ["--evidence-realisations", "0"], capsys)
    assert "--energy-resolved" in _refused(BASE + ["--evidence-realisations", "3", "--energy-resolved"], capsys)
    assert "--eval-segment" in _refused(BASE + ["--evidence-realisations", "3", "--eval-segment", "1"], capsys)
    # --realisations keeps its meaning and its error text
    assert "--realisations needs --stat-method frequentist (it profiles mock measurements)" in _refused(BASE + ["--realisations", "3"], capsys)
    assert "--realisations needs --stat-method frequentist" in _refused(BASE + ["--realisations", "3", "--evidence-realisations", "3"], capsys)
    f = sens.parse_args(BASE + ["--realisations", "3", "--stat-method", "frequentist"])
    assert f.realisations == 3 and f.evidence_realisations is None
    assert os.path.basename(sens.evidence_realisations_path(a)).startswith("fr_evidence_realisations")
    assert os.path.dirname(sens.evidence_realisations_path(a)) == os.path.dirname(sens.output_paths(a)[0])
