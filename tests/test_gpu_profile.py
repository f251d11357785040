"""The device profile-likelihood maximiser (golemflavor_amd.profile_llh, gf_simplex.hip) on the GPU: planted maxima, scipy's
Nelder-Mead from fixed starts, the commit logic against its host restatement on the device's own values, determinism, the
unitarity options and the frequentist CLI."""
import argparse
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import nested
from golemflavor_amd import profile_llh as P
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def sens_args(texture=Texture.OET, smearing=0.02):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=texture,
                              binning=Cf.default_bin_edges(), smearing=smearing, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


def notebook_model():
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    bf = fr_utils.angles_to_fr(asimov.values)
    return asimov, ps, bf


def oracle():
    from oracle import oracle as O
    return O


def cube_f(model, cols, base):
    """f(u) = -ln_prob(theta(u)) on the device's bulk path, theta formed as the device forms it."""
    lo, hi = np.asarray(model.desc.lo)[cols], np.asarray(model.desc.hi)[cols]

    def f_batch(U):
        th = np.tile(base, (len(U), 1))
        th[:, cols] = (hi - lo) * np.asarray(U) + lo
        lp, st = model.lnprob(th, want_status=True)
        bad = st == _lib.GF_ST_NON_UNITARY
        f = np.where(bad | ~(lp > -np.inf), np.inf, -lp)
        return f, bad
    return f_batch


def test_planted_maximum_notebook():
    # the notebook posterior with its Asimov composition replaced by the oracle's composition at the prior centres and a
    # (1, 0, 0) source: lnprior and the Gaussian likelihood then peak at the same theta*, and the maximum is ln_prob there
    _, ps, _ = notebook_model()
    O = oracle()
    theta_star = np.array(ps.values, dtype=float)
    theta_star[4:6] = np.asarray(fr_utils.fr_to_angles((1., 0., 0.)), dtype=float)
    _, fr0 = O.lnprob_batch(O.make_model(ps, "SM_GAUSS", smearing=0.02), theta_star[None], want_fr=True)
    bf = tuple(fr0[0])
    ref = O.lnprob_batch(O.make_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02), theta_star[None])[0]
    cols = list(range(len(ps)))
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02)) as m:
        with P.SimplexMaximizer([m], cols, theta_star, nstarts=16, nseed=2048, seed=3, xatol=1e-10, fatol=1e-12,
                                maxiter=4000, adaptive=True, restarts=2) as s:
            res = s.run()
        assert res["nstarts"][0] == 16
        got = res["max_lnl"][0]
        assert ref - 1e-6 <= got <= ref + 1e-9, (got, ref)
        again = m.lnprob(res["argmax_theta"][:1])[0]
        assert again[0] == got


@pytest.mark.parametrize("scale", [-100.0, -45.0])
def test_planted_maximum_sens(scale):
    # inject the composition the oracle computes at the prior centres: the maximum is ln_prob there
    O = oracle()
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    sp = nested._scale_paramset(ps, scale)
    centre = np.array(sp.values, dtype=float)
    kw = dict(texture="OET", dimension=6, binning=args.binning, source_ratio=args.source_ratio, bestfit_fr=(1 / 3, 1 / 3, 1 / 3),
              smearing=0.02)
    _, fr0 = O.lnprob_batch(O.make_model(sp, "BSM_GAUSS", **kw), centre[None], want_fr=True)
    kw["bestfit_fr"] = tuple(fr0[0])
    ref = O.lnprob_batch(O.make_model(sp, "BSM_GAUSS", **kw), centre[None])[0]
    names = list(sp.names)
    cols = [i for i in range(len(names)) if names[i] != "logLam"]
    kw["texture"] = Texture.OET
    with Model(compile_model(sp, "BSM_GAUSS", **kw)) as m:
        u0 = (centre[cols] - np.asarray(m.desc.lo)[cols]) / (np.asarray(m.desc.hi)[cols] - np.asarray(m.desc.lo)[cols])
        with P.SimplexMaximizer([m], cols, centre, nstarts=16, nseed=1024, seed=5, starts=[np.clip(u0 + 0.01, 0, 1)],
                                xatol=1e-10, fatol=1e-12, maxiter=6000, adaptive=True, restarts=2) as s:
            res = s.run()
        got = res["max_lnl"][0]
        assert ref - 1e-6 <= got <= ref + 1e-9 + 1e-10 * abs(ref), (got, ref)
        assert m.lnprob(res["argmax_theta"][:1])[0][0] == got


def test_scipy_parity_from_fixed_starts_sm():
    from scipy.optimize import minimize
    asimov, ps, bf = notebook_model()
    O = oracle()
    om = O.make_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02)
    cols = [0, 1, 2, 3]
    base = np.array(ps.values, dtype=float)
    rng = np.random.default_rng(11)
    starts = rng.uniform(0.2, 0.8, size=(12, 4))
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02)) as m:
        lo, hi = np.asarray(m.desc.lo)[cols], np.asarray(m.desc.hi)[cols]

        def f(u):
            th = base.copy()
            th[cols] = (hi - lo) * u + lo
            v = O.lnprob_batch(om, th[None])[0]
            return -v if v > -np.inf else np.inf
        for adaptive in (False, True):
            with P.SimplexMaximizer([m], cols, base, nstarts=0, nseed=0, starts=starts, adaptive=adaptive, restarts=0) as s:
                s.run()
                dev = s.starts(0)
            checked = 0
            for j, x0 in enumerate(starts):
                h = P.nelder_mead_speculative(lambda U: np.array([f(u) for u in U]), x0, adaptive=adaptive)
                if h["ties"]:
                    continue
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    r = minimize(f, x0, method="Nelder-Mead", bounds=[(0, 1)] * 4, options=dict(adaptive=adaptive, maxiter=800))
                assert dev["nit"][j] == r.nit and dev["nfev"][j] == r.nfev, (j, dev["nit"][j], r.nit)
                assert abs(-dev["lnl"][j] - r.fun) <= 1e-12 * abs(r.fun)
                checked += 1
            assert checked >= 6


@pytest.mark.parametrize("lpw", ["1", "4", "16"])
def test_commit_logic_matches_host_restatement(lpw):
    # the device's trajectories against nelder_mead_speculative fed the device's own values through the bulk path, which gives
    # the same bits as the maximiser's evaluation kernel at any lanes per walker.  Three runs of three starts, one restart:
    # scale -45 twice (the starts in two orders) and scale -30, where the likelihood underflows everywhere: every vertex is
    # +inf there, so every iteration shrinks.
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    sps = [nested._scale_paramset(ps, sc) for sc in (-45.0, -45.0, -30.0)]
    names = list(ps.names)
    cols = [i for i in range(len(names)) if names[i] != "logLam"]
    bases = np.array([p_.values for p_ in sps], dtype=float)
    x0s = np.random.default_rng(4).uniform(0.05, 0.95, size=(3, len(cols)))
    starts = np.stack([x0s, x0s[::-1], x0s])
    old = os.environ.get("GF_SIMPLEX_LPW")
    os.environ["GF_SIMPLEX_LPW"] = lpw
    models = [Model(nested._bsm_desc(args, asimov, p_, 0.02)) for p_ in sps]
    try:
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts, maxiter=150, adaptive=True,
                                restarts=1) as s:
            res = s.run()
            shrunk = 0
            for r in range(3):
                dev = s.starts(r)
                for j in range(3):
                    h = P.nelder_mead_speculative(cube_f(models[r], cols, bases[r]), starts[r, j], adaptive=True, maxiter=150,
                                                  restarts=1)
                    assert np.array_equal(dev["cube"][j], h["x"]), (r, j)
                    assert -dev["lnl"][j] == h["fun"] and dev["nit"][j] == h["nit"] and dev["nfev"][j] == h["nfev"], (r, j)
                    shrunk += h["devals"] != (len(cols) + 1) * len(h["calls"]) + 4 * (h["nit"] - len(h["calls"]))
            assert res["nevals"].sum() > res["nfev"].sum()
            assert shrunk >= 3, "no trajectory shrank"
            assert res["max_lnl"][2] == -np.inf and np.isfinite(res["max_lnl"][0])
    finally:
        for m in models:
            m.close()
        if old is None:
            os.environ.pop("GF_SIMPLEX_LPW", None)
        else:
            os.environ["GF_SIMPLEX_LPW"] = old


def test_determinism_and_run_independence():
    args = sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)
    kw = dict(nstarts=4, nseed=512, maxiter=200, restarts=1, adaptive=True, seed=9)
    a = P.profile_scan(args, asimov, ps, scales, run_ids=np.arange(4), **kw)
    b = P.profile_scan(args, asimov, ps, scales, run_ids=np.arange(4), **kw)
    c = P.profile_scan(args, asimov, ps, scales[2:3], run_ids=np.array([2]), **kw)
    for k in ("max_lnl", "argmax_theta", "nfev", "niter", "nevals", "nstarts", "starts_agreeing"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][2:3], c[k]), k


def _oeu_nonunitary_scale():
    """texture OEU: the first scale where a few per cent of the prior draws fail the reference's unitarity assert and some
    lnprob is finite."""
    args = sens_args(texture=Texture.OEU)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    rng = np.random.default_rng(5)
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    for s_ in np.linspace(lo, hi, 27):
        sp = nested._scale_paramset(ps, float(s_))
        f = llh_utils.bsm_ln_prob(args, asimov, sp, on_nonunitary="-inf", check_unitarity=True)
        try:
            box = np.array(sp.ranges, dtype=float)
            th = rng.uniform(box[:, 0], box[:, 1], size=(20000, len(sp)))
            th[:, list(sp.names).index("logLam")] = s_
            lp, st = f.model.lnprob(th, want_status=True)
        finally:
            f.close()
        if np.mean(st == _lib.GF_ST_NON_UNITARY) > 0.02 and np.any(np.isfinite(lp)):
            return float(s_)
    return None


def test_nonunitary_options():
    # the seed points meet non-unitary points there, so "-inf" counts them and "raise" fails the run
    args = sens_args(texture=Texture.OEU)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    sc = _oeu_nonunitary_scale()
    assert sc is not None
    kw = dict(nstarts=4, nseed=4096, maxiter=100, restarts=0, seed=7)
    res = P.profile_scan(args, asimov, ps, np.array([sc]), on_nonunitary="-inf", **kw)
    assert res["nonunitary"][0] > 0 and np.isfinite(res["max_lnl"][0])
    with pytest.raises(AssertionError, match="scale %.6g" % sc):
        P.profile_scan(args, asimov, ps, np.array([sc]), on_nonunitary="raise", **kw)


def test_sens_cli_frequentist_end_to_end(tmp_path):
    base = [sys.executable, "-m", "golemflavor_amd.sens", "--stat-method", "frequentist", "--segments", "4",
            "--smearing", "0.1", "--pl-starts", "8", "--pl-seed-points", "1024", "--datadir", str(tmp_path), "--seed", "3"]
    out = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    stat, mx = np.load(line["fr_stat"]), np.load(line["fr_maxllh"])
    assert "/frequentist/" in line["fr_stat"]
    assert stat.shape == (4, 2) and mx.shape == (4, 2)
    assert np.all(np.isfinite(stat)) and np.array_equal(stat, mx)
    assert np.array_equal(stat[:, 0], nested.sens_scales(6, 4))
    assert line["limit"] is None or np.isfinite(line["limit"])
    assert len(line["ts"]) == 4 and line["ts"][0] == 0.0
    out2 = subprocess.run(base + ["--eval-segment", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out2.returncode == 0, out2.stderr[-3000:]
    row = np.load(json.loads(out2.stdout.strip().splitlines()[-1])["fr_maxllh"])
    assert row.shape == (1, 2) and np.array_equal(row[0], mx[2])


def test_parked_and_settled_candidates_match_host_restatement():
    # texture OEU where a few per cent of the cube is non-unitary, no seeding (so every non-unitary count is a candidate's), on
    # "-inf": candidates are parked and settled by the emulated-x87 completion.  Every trajectory and every run's count of
    # non-unitary points must be those of nelder_mead_speculative on the same values, which counts only the points scipy
    # evaluates -- speculative non-unitary candidates (an xe scipy never evaluates, say) must occur and stay uncounted.
    sc = _oeu_nonunitary_scale()
    assert sc is not None
    args = sens_args(texture=Texture.OEU)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    sp = nested._scale_paramset(ps, sc)
    names = list(sp.names)
    cols = [i for i in range(len(names)) if names[i] != "logLam"]
    base = np.array(sp.values, dtype=float)
    starts = np.random.default_rng(8).uniform(0.0, 1.0, size=(2, 12, len(cols)))
    with Model(nested._bsm_desc(args, asimov, sp, 0.02)) as m:
        with P.SimplexMaximizer([m, m], cols, base, nstarts=0, nseed=0, starts=starts, maxiter=200, adaptive=True,
                                restarts=1, on_nonunitary="-inf") as s:
            res = s.run()
            fb = cube_f(m, cols, base)
            spec = 0
            for r in range(2):
                dev = s.starts(r)
                counted = 0
                for j in range(starts.shape[1]):
                    h = P.nelder_mead_speculative(fb, starts[r, j], adaptive=True, maxiter=200, restarts=1,
                                                  on_nonunitary="-inf")
                    assert np.array_equal(dev["cube"][j], h["x"]), (r, j)
                    assert dev["nit"][j] == h["nit"] and dev["nfev"][j] == h["nfev"], (r, j)
                    # the same point and the same theta (cube_to_theta rounds the product and the sum as cube_f does): the same bits
                    assert -dev["lnl"][j] == h["fun"], (r, j, -dev["lnl"][j], h["fun"])
                    counted += h["nonunitary"]
                    spec += h["nonunitary_speculative"]
                assert res["nonunitary"][r] == counted, (r, res["nonunitary"][r], counted)
            assert res["parked"].sum() > 0, "no candidate went through the settle kernel"
            assert res["nonunitary"].sum() > 0 and spec > 0, (res["nonunitary"], spec)


@pytest.mark.parametrize("nscan", [1, 2, 3])
def test_few_scanned_columns(nscan):
    # fewer than four rows per simplex: the round's four candidates still have rows of their own.  Two runs of three starts
    # each against the host restatement (and scipy's nit and nfev where no vertex ties)
    from scipy.optimize import minimize
    _, ps, bf = notebook_model()
    cols = list(range(nscan))
    base = np.array(ps.values, dtype=float)
    starts = np.random.default_rng(nscan).uniform(0.1, 0.9, size=(2, 3, nscan))
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02)) as m:
        fb = cube_f(m, cols, base)
        for adaptive in (False, True):
            with P.SimplexMaximizer([m, m], cols, base, nstarts=0, nseed=0, starts=starts, adaptive=adaptive, restarts=1) as s:
                s.run()
                for r in range(2):
                    dev = s.starts(r)
                    for j in range(3):
                        h = P.nelder_mead_speculative(fb, starts[r, j], adaptive=adaptive, restarts=1)
                        assert np.array_equal(dev["cube"][j], h["x"]), (adaptive, r, j)
                        assert -dev["lnl"][j] == h["fun"] and dev["nit"][j] == h["nit"] and dev["nfev"][j] == h["nfev"]
                        if not h["ties"]:
                            x0, first = starts[r, j], h["calls"][0]
                            with warnings.catch_warnings():
                                warnings.simplefilter("ignore")
                                sc = minimize(lambda u: float(fb(u[None])[0][0]), x0, method="Nelder-Mead",
                                              bounds=[(0, 1)] * nscan, options=dict(adaptive=adaptive, maxiter=200 * nscan))
                            assert np.array_equal(sc.x, first[0]) and sc.nit == first[2] and sc.nfev == first[3]
