"""Host side of the profile-likelihood maximiser (golemflavor_amd.profile_llh): the speculative Nelder-Mead restatement against
scipy bit for bit, the frequentist limit, the CLI's frequentist options and the gf_simplex_* C ABI (no GPU needed)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import nested
from golemflavor_amd import profile_llh as P
from golemflavor_amd import sens
from golemflavor_amd.enums import StatCateg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C = np.array([0.31, 0.67, 0.52, 0.23])
_W = np.array([1.0, 2.3, 0.7, 1.9])

FUNCS = {
    "quadratic": lambda x: float(np.sum(_W[:len(x)] * (x - _C[:len(x)]) ** 2)),
    "rosenbrock": lambda x: float(np.sum(100.0 * (x[1:] - x[:-1] ** 2.0) ** 2.0 + (1 - x[:-1]) ** 2.0)),
    "outside": lambda x: float(np.sum(_W[:len(x)] * (x - 1.3 + 0.1 * np.arange(len(x))) ** 2)),     # optimum beyond the box
    "inf_region": lambda x: np.inf if x[0] + 0.8 * x[-1] > 1.1 else float(np.sum(_W[:len(x)] * (x - 0.45) ** 2)),
}


def _scipy(f, x0, adaptive, opts):
    from scipy.optimize import minimize
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return minimize(f, x0, method="Nelder-Mead", bounds=[(0, 1)] * len(x0), options=dict(adaptive=adaptive, **opts))


def _cases():
    for name in FUNCS:
        for n in (2, 3, 4):
            for adaptive in (False, True):
                for x0 in (np.full(n, 0.1), np.linspace(0.05, 0.9, n), np.zeros(n), np.full(n, 0.99)):
                    for opts in (dict(maxiter=200 * n), dict(maxiter=7), dict(xatol=1e-9, fatol=1e-11, maxiter=3000)):
                        if name == "inf_region" and not np.isfinite(FUNCS[name](x0)):
                            continue
                        yield name, n, adaptive, x0, opts


def test_speculative_nelder_mead_matches_scipy_bit_for_bit():
    seen = dict(shrink=0, clip=0, maxiter=0, tolerance=0, inf=0)
    per_func = dict.fromkeys(FUNCS, 0)
    for name, n, adaptive, x0, opts in _cases():
        f = FUNCS[name]
        evals = []

        def fb(U):
            evals.append(len(U))
            return np.array([f(u) for u in U])
        h = P.nelder_mead_speculative(fb, x0, adaptive=adaptive, xatol=opts.get("xatol", 1e-4), fatol=opts.get("fatol", 1e-4),
                                      maxiter=opts["maxiter"])
        if h["ties"]:
            continue                      # numpy's argsort need not keep ties in index order
        r = _scipy(f, x0, adaptive, opts)
        assert np.array_equal(r.x, h["x"]) and r.fun == h["fun"], (name, n, adaptive, x0, opts)
        assert r.nit == h["nit"] and r.nfev == h["nfev"], (name, n, adaptive, x0, opts, r.nit, h["nit"], r.nfev, h["nfev"])
        assert h["devals"] == sum(evals) and h["devals"] >= h["nfev"]
        per_func[name] += 1
        seen["shrink"] += n in evals[1:]
        seen["clip"] += bool(np.any((r.x == 0) | (r.x == 1)))
        seen["maxiter"] += r.nit == opts["maxiter"]
        seen["tolerance"] += r.nit < opts["maxiter"]
        seen["inf"] += name == "inf_region"
    assert min(per_func.values()) >= 10, per_func
    assert min(seen.values()) >= 3, seen


def test_speculative_restarts_equal_calling_scipy_again():
    f = FUNCS["quadratic"]
    for x0 in np.random.default_rng(1).uniform(0.05, 0.6, size=(20, 3)):
        h = P.nelder_mead_speculative(lambda U: np.array([f(u) for u in U]), x0, adaptive=True, restarts=3)
        if not h["ties"] and len(h["calls"]) > 1:
            break
    assert not h["ties"] and len(h["calls"]) > 1
    x, nit, nfev, prev = x0, 0, 0, None
    for call in h["calls"]:
        r = _scipy(f, x, True, dict(maxiter=600))
        assert np.array_equal(r.x, call[0]) and r.fun == call[1] and r.nit == call[2] and r.nfev == call[3]
        x, nit, nfev = r.x, nit + r.nit, nfev + r.nfev
    assert (h["nit"], h["nfev"]) == (nit, nfev)
    assert len(h["calls"]) == 4 or h["calls"][-2][1] - h["calls"][-1][1] <= 1e-4


def test_speculative_nonunitary_counts_only_evaluated_points():
    # xe lies in the "non-unitary" region only when scipy does not evaluate it: nothing is counted, nothing fails
    def fb(U):
        f = np.array([FUNCS["quadratic"](u) for u in U])
        return f, np.zeros(len(U), dtype=bool)
    ref = P.nelder_mead_speculative(fb, np.full(3, 0.2), on_nonunitary="raise")
    spec = []

    def fb_bad(U):
        f, bad = fb(U)
        if len(U) == 4:
            spec.append(1)
            bad = bad.copy()
            bad[1] = True                 # flag every xe
        return f, bad
    h = P.nelder_mead_speculative(fb_bad, np.full(3, 0.2), on_nonunitary="-inf")
    expansions = sum(1 for _ in spec)
    assert expansions > 0
    # counted exactly where scipy evaluates xe: where fxr < fsim[0]
    assert 0 < h["nonunitary"] < expansions and h["nfev"] == ref["nfev"]
    assert h["nonunitary"] + h["nonunitary_speculative"] == expansions and h["nonunitary_speculative"] > 0
    assert np.array_equal(h["x"], ref["x"]) and h["fun"] == ref["fun"]
    with_raise = P.nelder_mead_speculative(fb_bad, np.full(3, 0.2), on_nonunitary="raise")
    assert with_raise["failed"]


def test_profile_likelihood_limit_linear_curves():
    scales = np.linspace(-40, -20, 10)
    lnl = -3.0 * (scales - scales[0])                    # -2 dlnL = 6 (s - s0): crosses 3.84 at s0 + 0.64
    lim = P.profile_likelihood_limit(scales, lnl)
    assert lim is not None and abs(lim + np.log10(2) - (scales[0] + 3.8414588206941254 / 6)) < 0.03
    lim2 = P.profile_likelihood_limit(scales, lnl, threshold=12.0)
    assert abs(lim2 + np.log10(2) - (scales[0] + 2.0)) < 0.03


def test_profile_likelihood_limit_none_cases_and_nonfinite_rows():
    scales = np.linspace(-40, -20, 10)
    assert P.profile_likelihood_limit(scales, np.zeros(10)) is None                  # flat: no exclusion
    dip = -3.0 * (scales - scales[0])
    dip[5:] = -1.0                                                                     # comes back: large scales not excluded
    assert P.profile_likelihood_limit(scales, dip) is None
    one = np.zeros(10)
    one[-1] = -10.0                                                                    # one point beyond the threshold
    assert P.profile_likelihood_limit(scales, one) is None
    lnl = -3.0 * (scales - scales[0])
    with_inf = lnl.copy()
    with_inf[[7, 9]] = -np.inf
    got = P.profile_likelihood_limit(scales, with_inf)
    want = P.profile_likelihood_limit(np.delete(scales, [7, 9]), np.delete(lnl, [7, 9]))
    assert got is not None and got == want
    assert P.profile_likelihood_limit(scales[:3], lnl[:3]) is None
    no_null = lnl.copy()
    no_null[0] = -np.inf                                  # the null row itself: no statistic against another scale
    assert P.profile_likelihood_limit(scales, no_null) is None
    assert P.profile_likelihood_limit(scales[::-1], no_null[::-1]) is None


def test_sens_cli_frequentist_options():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "golemflavor_amd.sens", "--help"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0
    for opt in ("--pl-starts", "--pl-seed-points", "--pl-xatol", "--pl-fatol", "--pl-maxiter", "--pl-restarts", "--pl-adaptive"):
        assert opt in out.stdout
    a = sens.parse_args(["--stat-method", "frequentist", "--datadir", "/d", "--segments", "4"])
    assert a.stat_method is StatCateg.FREQUENTIST and a.pl_starts == 64 and a.pl_seed_points == 8192 and a.pl_adaptive
    stat, llh = sens.output_paths(a)
    assert stat.startswith(os.path.join("/d", "frequentist", "asimov", "fr_stat"))
    assert llh.startswith(os.path.join("/d", "frequentist", "asimov", "fr_maxllh"))
    a2 = sens.parse_args(["--stat-method", "frequentist", "--datadir", "/d", "--segments", "4", "--eval-segment", "2"])
    assert sens.output_paths(a2)[1].endswith("_scale_{0:.0E}".format(10 ** nested.sens_scales(6, 4)[2]))


def test_simplex_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(gf_simplex_[a-z_]+)\s*\(", hdr, re.M))
    assert declared == {"gf_simplex_" + n for n in ("create", "set_run_ids", "set_starts", "set_options", "destroy", "run",
                                                    "result", "get_starts")}
    L = _lib.lib()
    for n in declared:
        assert n in _lib.SIGNATURES and hasattr(L, n)


def test_simplex_create_validates_before_touching_the_device():
    L = _lib.lib()
    h = C.c_void_p()
    models = (C.c_void_p * 1)(None)
    cols = (C.c_int32 * 1)(0)
    base = (C.c_double * 1)(0.0)
    bad = [(models, 0, 1, cols, base, 4, 16, 0, 0),           # no runs
           (models, 1, 0, cols, base, 4, 16, 0, 0),           # no columns
           (models, 1, 17, cols, base, 4, 16, 0, 0),          # too many columns
           (models, 1, 1, cols, base, 32, 16, 0, 0),          # more starts than seed points
           (models, 1, 1, cols, base, -1, 16, 0, 0),
           (models, 1, 1, cols, base, 4, 16, 0, 2),           # on_nonunitary
           (models, 1, 1, cols, base, 4, 16, 0, 0)]           # null model
    for args in bad:
        assert L.gf_simplex_create(*args, C.byref(h)) == _lib.GF_ERR_INVALID_ARG, args
    assert L.gf_simplex_set_options(None, 1e-4, 1e-4, 10, 0, 0) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_simplex_run(None, 1) == _lib.GF_ERR_INVALID_ARG
