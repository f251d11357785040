"""The evidence of a nested sampler's runs under other Gaussian measurements, on the GPU (gf_ns_toys.hip through
NestedSampler.reweight_evidence and realisations.evidence_realisation_scan):

  1. a realisation equal to a run's own measurement gives posterior()'s lnz_check and ess bit for bit;
  2. m, s, s2, ess and kept equal the host build of gf_ns_toys.hpp (tests/ns_toys_harness.py) fed with dead()'s lnw and
     Model.propagate's compositions, at runs below one leaf of 4096 points, of exactly 4096, of 4097 and past two leaves, for 1, 3 and
     130 realisations (past one tile of 64), shared and per run, a smearing per realisation;
  3. neither the runs that share the sampler nor the batching of the realisations change a bit;
  4. the rules: non-unitary points and the plateau's lnw = -inf points are not kept, a realisation out of every point's reach has
     kept 0, ess 0 and lnz -inf, a failed or never-run sampler gives NaN; the refusals;
  5. ln Z under three realisations against 2-D quadrature of the oracle's lnprob, within 4 lnz_err of the run;
  6. against a second nested run on models compiled with the realisation;
  7. the scan and the driver.

The bit-for-bit tests use smearings of 0.05 and more, and the harness asserts that no Gaussian exponent lies in the subnormal band.

The run past two leaves has nlive = 1024: with 256 live points 8192 points are a run 31 e-folds deep, where the live points' lnL tie
in double precision; 1024 live points reach them at a depth of 13."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ns_toys_harness as H
import test_gpu_realisations as TR
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import nested
from golemflavor_amd import realisations as R
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SEED, IDS, SMEAR = 3, [5, 6, 7], [0.05, 0.08, 0.12]
KW = dict(nlive=100, batch=12, walks=10, seed=SEED)
NU = _lib.GF_ST_NON_UNITARY


def _tutorial(smearing):
    asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=smearing)
    return llh_utils.tutorial_ln_prob(asimov, ps)


def _model(s, r):
    return getattr(s.models[r], "model", s.models[r])


def own_measurement(s, r):
    """(bf [3], smearing, offset) of run r's model"""
    d = _model(s, r).desc
    return np.array([d.bestfit_fr[k] for k in range(3)]), float(d.smearing), float(d.offset)


def raw_evidence(s, bf, smearing):
    """gf_nested_toys_evidence itself: dict(m, s, s2, ess, kept), each [nruns][T]"""
    bf = np.ascontiguousarray(bf, dtype=np.float64)
    T = bf.shape[-2]
    sm = np.ascontiguousarray(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (T,)))
    out = {k: np.empty((s.nruns, T)) for k in ("m", "s", "s2", "ess")}
    out["kept"] = np.empty((s.nruns, T), np.int64)
    _lib.check(s._L.gf_nested_toys_evidence(s._h, bf.ctypes.data_as(_lib._dp), sm.ctypes.data_as(_lib._dp), T, int(bf.ndim == 3),
                                            *[out[k].ctypes.data_as(_lib._dp) for k in ("m", "s", "s2", "ess")],
                                            out["kept"].ctypes.data_as(_lib._lp)), "gf_nested_toys_evidence")
    return out


def run_points(s, r):
    """what the host build is fed for run r: dead()'s lnw, Model.propagate's composition and status of dead()'s theta"""
    d = s.dead(r)
    fr, st = _model(s, r).propagate(d["theta"])
    return d["lnw"], fr, st


def host_reference(s, r, bf, smearing, points=None):
    lnw, fr, st = points if points is not None else run_points(s, r)
    obf, osm, off = own_measurement(s, r)
    return H.host_evidence(lnw, fr, st, H.consts([obf], osm)[0], H.consts(bf, smearing), off)


def assert_equals_host(got, r, ref, what):
    for k in ("m", "s", "s2", "ess"):
        assert H.same_bits(got[k][r], ref[k]), (what, r, k, got[k][r], ref[k])
    assert np.array_equal(got["kept"][r], ref["kept"]), (what, r, got["kept"][r], ref["kept"])


def realisations_of(bf, T, seed):
    """T measurements around bf, a smearing each, 0.05 and more"""
    rng = np.random.default_rng(seed)
    return bf + 0.06 * rng.standard_normal((T, 3)), rng.uniform(0.05, 0.09, T)


@pytest.fixture(scope="module")
def three():
    """three tutorial runs of different smearing, below one leaf each; (sampler, models, result, per run the host build's points)"""
    fs = [_tutorial(sm) for sm in SMEAR]
    s = nested.NestedSampler(fs, [0, 1], np.zeros(2), run_ids=IDS, **KW)
    res = s.run()
    yield s, fs, res, [run_points(s, r) for r in range(3)]
    s.close()
    for f in fs:
        f.close()


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------
def check_identity(s, what):
    post = s.posterior()
    bf = np.stack([own_measurement(s, r)[0] for r in range(s.nruns)])[:, None, :]           # [nruns][1][3]: each run's own
    sms = {own_measurement(s, r)[1] for r in range(s.nruns)}
    assert len(sms) == 1 and min(sms) >= 0.05
    got = s.reweight_evidence(bf)                                                           # the smearing: the models' own
    for k in ("lnz", "ess", "kept", "max_x"):
        assert got[k].shape == (1, s.nruns), k
    assert np.all(np.isfinite(post["lnz_check"])) and np.all(post["ess"] > 1.0)
    assert np.array_equal(got["lnz"][0], post["lnz_check"]), (what, got["lnz"][0], post["lnz_check"])
    assert np.array_equal(got["ess"][0], post["ess"]), (what, got["ess"][0], post["ess"])
    for r in range(s.nruns):
        lnw = s.dead(r)["lnw"]
        assert got["kept"][0, r] == np.isfinite(lnw).sum() and got["max_x"][0, r] == lnw.max(), (what, r)


def test_identity_notebook_posterior():
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    bf = fr_utils.angles_to_fr(asimov.values)
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.05)) as m:
        base = np.array(ps.values, dtype=np.float64)
        with nested.NestedSampler([m, m], list(range(len(ps))), base, nlive=128, walks=10, seed=4, run_ids=[1, 2]) as s:
            s.run()
            check_identity(s, "notebook")


def test_identity_sens_posterior():
    args = TR.sens_args(smearing=0.05)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)[[0, 2]]
    res = nested.evidence_scan(args, asimov, ps, scales, run_ids=[0, 2], nlive=128, walks=10, seed=7, on_nonunitary="-inf", return_sampler=True)
    try:
        assert np.all(np.isfinite(res["lnz"]))
        check_identity(res["sampler"], "sens")
    finally:
        res["sampler"].close()
        for m in res["models"]:
            m.close()


# ---- 2. the host build -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 130])
def test_equals_host_build_shared_and_per_run(three, T):
    s, fs, res, pts = three
    bf0 = own_measurement(s, 0)[0]
    bf, sm = realisations_of(bf0, T, seed=T)
    got = raw_evidence(s, bf, sm)
    for r in range(3):
        ref = host_reference(s, r, bf, sm, pts[r])
        assert_equals_host(got, r, ref, "shared T=%d" % T)
        assert np.all(ref["kept"] > 0) and np.all(ref["ess"] > 1.0)
    per = np.stack([realisations_of(bf0, T, seed=100 * (r + 1) + T)[0] for r in range(3)])       # [3][T][3]
    got = raw_evidence(s, per, sm)
    for r in range(3):
        assert_equals_host(got, r, host_reference(s, r, per[r], sm, pts[r]), "per run T=%d" % T)
    # the Python layer: the same numbers, [T][nruns], ln Z with the C library's log
    py = s.reweight_evidence(per, sm)
    assert H.same_bits(py["ess"], got["ess"].T) and np.array_equal(py["kept"], got["kept"].T) and H.same_bits(py["max_x"], got["m"].T)
    want = np.array([[m_ + math.log(s_) for m_, s_ in zip(mr, sr)] for mr, sr in zip(got["m"], got["s"])])
    assert H.same_bits(py["lnz"], want.T)


def stop_tolerance(f, nlive, batch, k, seed, run_id):
    """The evidence tolerance at which the run of (nlive, batch, seed, run_id) on f stops at iteration k, n = k * batch + nlive points:
    the stopping rule ln(Z + L_max X) - ln Z < tol (k_ns_select) restated on the points of a longer run -- the tolerance ends a
    run and changes nothing before its end."""
    with nested.NestedSampler([f], [0, 1], np.zeros(2), nlive=nlive, batch=batch, walks=10, seed=seed, tol=1e-9, run_ids=[run_id]) as s:
        s.run()
        d = s.dead(0)
    nd = d["ndead"]
    assert nd >= (k + 1) * batch, (nd, k, batch)
    lnl, lnw = d["lnl"], d["lnw"]
    lnz = np.logaddexp.accumulate(lnw[:nd])                         # after the first j + 1 dead points
    lnx = -np.cumsum(1.0 / d["nlive_seq"][:nd])
    lmax = np.maximum.accumulate(lnl[::-1])[::-1]                   # the best point still alive before dead point j
    c = np.array([np.logaddexp(lnz[i * batch - 1], lmax[i * batch] + lnx[i * batch - 1]) - lnz[i * batch - 1] for i in range(1, k + 1)])
    tol = math.sqrt(c[k - 2] * c[k - 1])
    assert c[:k - 1].min() > tol > c[k - 1], c[-3:]
    return tol


SHAPES = {"exact": (256, 128, 30, H.LEAF), "plus_one": (256, 167, 23, H.LEAF + 1)}


@pytest.fixture(scope="module")
def shaped():
    """single runs of the tutorial posterior (smearing 0.05) with exactly 4096 points, with 4097, and past two leaves"""
    f = _tutorial(0.05)
    out = {}
    try:
        for name, (nlive, batch, k, n) in SHAPES.items():
            tol = stop_tolerance(f, nlive, batch, k, SEED, 11)
            s = nested.NestedSampler([f], [0, 1], np.zeros(2), nlive=nlive, batch=batch, walks=10, seed=SEED, tol=tol, run_ids=[11])
            s.run()
            out[name] = s
        s = nested.NestedSampler([f], [0, 1], np.zeros(2), nlive=1024, batch=128, walks=10, seed=SEED, tol=1e-4, run_ids=[12])
        s.run()
        out["long"] = s
        yield out
    finally:
        for s in out.values():
            s.close()
        f.close()


@pytest.mark.parametrize("name", ["exact", "plus_one", "long"])
def test_equals_host_build_at_the_leaf_edges(shaped, name):
    s = shaped[name]
    pts = run_points(s, 0)
    n = len(pts[0])
    print("%s: %d points, %d leaves" % (name, n, -(-n // H.LEAF)))
    if name in SHAPES:
        assert n == SHAPES[name][3]
    else:
        assert n > 2 * H.LEAF
    assert s.posterior()["npoints"][0] == n
    bf0 = own_measurement(s, 0)[0]
    for T in (3, 130):
        bf, sm = realisations_of(bf0, T, seed=7 * T)
        bf[0], sm[0] = bf0, 0.05                                    # the first: the run's own
        got = raw_evidence(s, bf, sm)
        ref = host_reference(s, 0, bf, sm, pts)
        assert_equals_host(got, 0, ref, "%s T=%d" % (name, T))
        post = s.posterior()
        assert got["ess"][0, 0] == post["ess"][0] and got["m"][0, 0] + math.log(got["s"][0, 0]) == post["lnz_check"][0]


# ---- 3. company and batching -------------------------------------------------------------------------------------------------------
def test_company_and_batching_change_nothing(three, monkeypatch):
    s, fs, res, pts = three
    bf, sm = realisations_of(own_measurement(s, 0)[0], 130, seed=9)
    among = raw_evidence(s, bf, sm)
    with nested.NestedSampler([fs[1]], [0, 1], np.zeros(2), run_ids=[IDS[1]], **KW) as alone:
        ra = alone.run()
        assert ra["lnz"][0] == res["lnz"][1] and ra["niter"][0] == res["niter"][1]
        one = raw_evidence(alone, bf, sm)
    for k in among:
        assert H.same_bits(one[k][0], among[k][1]), k
    # 3 runs of one leaf: 108 bytes of partials per realisation, so 1000 bytes hold 9 and 130 go in 15 batches
    monkeypatch.setenv("GF_NS_TOYS_SCRATCH_BYTES", "1000")
    try:
        batched = raw_evidence(s, bf, sm)
        per = np.stack([bf, bf[::-1], bf + 0.01])
        batched_per = raw_evidence(s, per, sm)
    finally:
        monkeypatch.delenv("GF_NS_TOYS_SCRATCH_BYTES")
    whole_per = raw_evidence(s, per, sm)
    for k in among:
        assert H.same_bits(batched[k], among[k]), k
        assert H.same_bits(batched_per[k], whole_per[k]), k
    assert "GF_NS_TOYS_SCRATCH_BYTES=1000" in _lib.diagnostic_overrides()


# ---- 4. the rules ------------------------------------------------------------------------------------------------------------------
def _oeu_scale():
    """texture OEU: the first scale where a few per cent of the prior draws fail the reference's unitarity assert and some lnprob is
    finite (tests/test_gpu_realisations.py's oeu_scale)"""
    args = TR.sens_args(texture=Texture.OEU)
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
        if np.mean(st == NU) > 0.02 and np.any(np.isfinite(lp)):
            return float(s_)
    raise AssertionError("no scale with non-unitary draws")


def test_rules_nonunitary_plateau_and_out_of_reach():
    sc = _oeu_scale()
    args = TR.sens_args(texture=Texture.OEU, smearing=0.05)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    res = nested.evidence_scan(args, asimov, ps, np.array([sc]), run_ids=[3], nlive=256, walks=10, seed=7, on_nonunitary="-inf",
                               return_sampler=True)
    s = res["sampler"]
    try:
        assert res["nonunitary"][0] > 0 and np.isfinite(res["lnz"][0])
        lnw, fr, st = pts = run_points(s, 0)
        n_nu, n_plat = int((st == NU).sum()), int((lnw == -np.inf).sum())
        print("OEU scale %.4g: %d points, %d non-unitary, %d with lnw = -inf" % (sc, len(lnw), n_nu, n_plat))
        assert n_nu > 0 and n_plat >= n_nu and np.all(lnw[st == NU] == -np.inf)
        bf0, sm0, _ = own_measurement(s, 0)
        bf = np.stack([bf0, bf0 + np.array([0.05, -0.05, 0.0]), np.array([5.0, 5.0, 5.0])])
        sm = np.array([sm0, 0.06, 0.01])                             # the last: so far and so narrow that every lt is -inf
        got = raw_evidence(s, bf, sm)
        assert_equals_host(got, 0, host_reference(s, 0, bf, sm, pts), "OEU")
        keep = np.isfinite(lnw) & (st != NU)
        assert got["kept"][0, 0] == keep.sum() == np.isfinite(lnw).sum() and 0 < got["kept"][0, 1] <= keep.sum()
        py = s.reweight_evidence(bf, sm)
        assert py["kept"][2, 0] == 0 and py["ess"][2, 0] == 0.0 and py["lnz"][2, 0] == -np.inf and py["max_x"][2, 0] == -np.inf
        assert np.isfinite(py["lnz"][:2, 0]).all() and py["lnz"][0, 0] == s.posterior()["lnz_check"][0]
    finally:
        s.close()
        for m in res["models"]:
            m.close()
    # a run that failed (raise mode met a non-unitary point) beside nothing else, and a sampler that never ran
    res = None
    cols, models, bases, labels = nested._scan_models(args, asimov, ps, np.array([sc]), 0.05, 0)
    try:
        with nested.NestedSampler(models, cols, bases, nlive=256, walks=10, seed=7, run_ids=[3]) as failed:
            never = failed.reweight_evidence(bf, sm)
            assert failed.run(check=False)["failed"][0]
            out = failed.reweight_evidence(bf, sm)
        for o in (never, out):
            assert np.isnan(o["lnz"]).all() and np.isnan(o["max_x"]).all() and np.all(o["ess"] == 0.0) and np.all(o["kept"] == 0)
    finally:
        for m in models:
            m.close()


def test_refusals(three):
    s, fs, res, pts = three
    bf = np.tile(own_measurement(s, 0)[0], (2, 1))
    for bad in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(_lib.GolemHipError, match="smearing > 0"):
            s.reweight_evidence(bf, [0.1, bad])
    with pytest.raises(_lib.GolemHipError, match="finite measurement"):
        s.reweight_evidence([[0.3, 0.3, np.nan], [0.3, 0.3, 0.4]], 0.1)
    with pytest.raises(ValueError, match=r"\[T\]\[3\]"):
        s.reweight_evidence(np.zeros((2, 2, 3)), 0.1)               # per run needs nruns = 3 leading
    with pytest.raises(ValueError, match="share one smearing"):
        s.reweight_evidence(bf)                                      # the three runs' models differ in smearing
    # models without a flux-averaged Gaussian measurement
    import test_gpu_nested_exact as TE
    ps = TE.prior_paramset(3)
    with Model(compile_model(ps, "PRIOR_ONLY", flat_llh=0.0)) as m:
        with nested.NestedSampler([m], [0, 1], np.array(ps.values, dtype=np.float64), nlive=64, walks=5, seed=1) as p:
            p.run()
            with pytest.raises(_lib.GolemHipError, match="no Gaussian measurement") as e:
                raw_evidence(p, bf, 0.1)
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED
    args = TR.sens_args(smearing=0.1)
    asimov, sps = Cf.sens_paramsets(6, (1., 1., 1.))
    cols, models, bases, _ = nested._scan_models(args, asimov, sps, nested.sens_scales(6, 4)[:1], 0.1, 0)
    try:
        binned = llh_utils.BinnedMeasurement.constant(TR.model_bf(asimov), 0.1, np.asarray(args.binning, dtype=float))
        models[0].set_binned_measurement(binned)
        with nested.NestedSampler(models, cols, bases, nlive=64, walks=5, seed=1) as b:
            with pytest.raises(_lib.GolemHipError, match="binned measurement") as e:
                raw_evidence(b, bf, 0.1)
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="energy-resolved"):
            R.evidence_realisation_scan(args, asimov, sps, nested.sens_scales(6, 4), ntoys=2, binned=binned)
    finally:
        for m in models:
            m.close()


# ---- 5. truth ----------------------------------------------------------------------------------------------------------------------
def test_truth_against_quadrature(oracle):
    """SM_GAUSS (the notebook posterior) over its two source angles, the mixing parameters at their base values, nlive = 256; the
    model's own measurement and shifts of one and two smearings along (1, -1, 0) / sqrt 2.

    Measured on an MI355X: lnz_err 0.1001; (lnz - exact) / lnz_err = -0.348, -0.136, -0.015; the differences to realisation 0,
    0.212 and 0.333 (profiles/evidence_realisations/README.txt).  The bound of 4 is the run's own error: a CPU simulation of exact
    nested sampling finds the reweighted error equal to lnz_err to within a per cent out to three widths."""
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    bf0, sm = fr_utils.angles_to_fr(asimov.values), 0.05
    cols, base = [4, 5], np.array(ps.values, dtype=np.float64)
    shift = sm * np.array([1.0, -1.0, 0.0]) / math.sqrt(2.0)
    meas = np.stack([bf0, bf0 + shift, bf0 + 2.0 * shift])
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf0, smearing=sm)) as m:
        with nested.NestedSampler([m], cols, base, nlive=256, seed=11) as s:
            res = s.run()
            got = s.reweight_evidence(meas)
    err = res["lnz_err"][0]
    assert err > 0 and np.isfinite(res["lnz"][0])
    n = 2001
    u = (np.arange(n) + 0.5) / n
    box = np.array(ps.ranges, dtype=np.float64)
    th = np.tile(base, (n * n, 1))
    A, B = np.meshgrid(u, u, indexing="ij")
    th[:, 4] = (box[4, 1] - box[4, 0]) * A.ravel() + box[4, 0]
    th[:, 5] = (box[5, 1] - box[5, 0]) * B.ravel() + box[5, 0]
    exact = np.empty(3)
    for t in range(3):
        lp = oracle.lnprob_batch(oracle.make_model(ps, "SM_GAUSS", bestfit_fr=meas[t], smearing=sm), th, threads=16)
        top = lp.max()
        exact[t] = top + math.log(np.mean(np.exp(lp - top)))
    dev = (got["lnz"][:, 0] - exact) / err
    ddev = ((got["lnz"][:, 0] - got["lnz"][0, 0]) - (exact - exact[0])) / err
    print("truth: lnz_err %.4f, ln Z exact %s, reweighted %s, ess %s" % (err, exact.tolist(), got["lnz"][:, 0].tolist(), got["ess"][:, 0].tolist()))
    print("truth: deviations / lnz_err %s, of the differences to realisation 0 %s" % (dev.tolist(), ddev.tolist()))
    # realisation 0 is the run's own measurement: its ln Z is the run's, up to the rounding of two summation orders
    assert abs(got["lnz"][0, 0] - res["lnz"][0]) < 1e-9 * max(1.0, abs(res["lnz"][0]))
    assert np.all(np.abs(dev) <= 4.0), dev
    assert np.all(np.abs(ddev) <= 4.0), ddev


# ---- 6. against a re-run -----------------------------------------------------------------------------------------------------------
def test_against_a_rerun_under_the_realisation():
    """Measured on an MI355X: (lnz_rw - lnz_rerun) / sigma = -1.20, 1.49, -2.09, 0.19 (profiles/evidence_realisations/README.txt)."""
    args = TR.sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)[[0, 2]]
    meas = R.draw_realisations(TR.model_bf(asimov), 0.1, 2, seed=1)
    kw = dict(nlive=128, seed=7, on_nonunitary="-inf")             # the default walks: the runs' own accuracy is what is compared
    res = nested.evidence_scan(args, asimov, ps, scales, run_ids=[0, 2], return_sampler=True, **kw)
    try:
        got = res["sampler"].reweight_evidence(meas)                 # [2][2]
    finally:
        res["sampler"].close()
        for m in res["models"]:
            m.close()
    models, bases = [], []
    try:
        for t in range(2):
            for sc in scales:
                sp = nested._scale_paramset(ps, float(sc))
                models.append(Model(TR.sens_desc(args, sp, meas[t], 0.1)))
                bases.append(np.array(sp.values, dtype=np.float64))
        cols = [i for i in range(len(ps)) if i != list(ps.names).index("logLam")]
        with nested.NestedSampler(models, cols, bases, run_ids=[10, 11, 12, 13], **kw) as again:
            rr = again.run()
    finally:
        for m in models:
            m.close()
    lnz2, err2 = rr["lnz"].reshape(2, 2), rr["lnz_err"].reshape(2, 2)
    sig = np.sqrt(res["lnz_err"][None, :] ** 2 + err2 ** 2)
    dev = (got["lnz"] - lnz2) / sig
    print("re-run: reweighted %s, re-run %s, deviations / sigma %s, ess %s" % (got["lnz"].tolist(), lnz2.tolist(), dev.tolist(), got["ess"].tolist()))
    assert np.all(np.isfinite(lnz2)) and np.all(np.abs(got["lnz"] - lnz2) <= 4.0 * sig), dev


# ---- 7. the scan and the driver ----------------------------------------------------------------------------------------------------
def test_scan_equals_reweight_evidence_on_the_scan_sampler():
    args = TR.sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)
    meas = R.draw_realisations(TR.model_bf(asimov), 0.1, 3, seed=5)
    kw = dict(run_ids=np.arange(4), nlive=128, walks=10, seed=3, on_nonunitary="-inf")
    out = R.evidence_realisation_scan(args, asimov, ps, scales, measurements=meas, **kw)
    res = nested.evidence_scan(args, asimov, ps, scales, return_sampler=True, **kw)
    try:
        ref = res["sampler"].reweight_evidence(meas, 0.1)
        ess_run = res["sampler"].posterior()["ess"]
    finally:
        res["sampler"].close()
        for m in res["models"]:
            m.close()
    for k in ("lnz", "ess", "kept", "max_x"):
        assert out[k].shape == (3, 4) and H.same_bits(out[k], ref[k]), k
    assert np.array_equal(out["lnz_run"], res["lnz"]) and np.array_equal(out["lnz_err_run"], res["lnz_err"]) and np.array_equal(out["ess_run"], ess_run)
    assert np.array_equal(out["measurements"], meas) and out["smearings"].tolist() == [0.1] * 3 and np.array_equal(out["scales"], scales)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out["bayes"], ref["lnz"] - ref["lnz"][:, :1], equal_nan=True)
        assert np.array_equal(out["ess_fraction"], ref["ess"] / ess_run[None, :], equal_nan=True)
    lim = R.evidence_limits(scales, ref["lnz"])
    assert np.array_equal(out["limits"], lim["limits"], equal_nan=True) and np.array_equal(out["discovered"], lim["discovered"])
    assert out["n_low_ess"] == 0 and out["seconds"] >= out["seconds_nested"] > 0 and out["seconds_reweight"] > 0
    # the default measurements are realisation_scan's for the same seed
    drawn = R.evidence_realisation_scan(args, asimov, ps, scales, ntoys=3, toy_seed=5, **kw)
    assert np.array_equal(drawn["measurements"], meas) and H.same_bits(drawn["lnz"], out["lnz"])


def test_sens_cli_evidence_realisations_end_to_end(tmp_path):
    base = [sys.executable, "-m", "golemflavor_amd.sens", "--segments", "4", "--mn-live-points", "128", "--mn-walks", "10", "--smearing", "0.1",
            "--seed", "3"]
    with_opt = subprocess.run(base + ["--datadir", str(tmp_path / "a"), "--evidence-realisations", "3", "--realisation-seed", "2"], cwd=ROOT,
                              capture_output=True, text=True, timeout=600)
    assert with_opt.returncode == 0, with_opt.stderr[-3000:]
    without = subprocess.run(base + ["--datadir", str(tmp_path / "b")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert without.returncode == 0, without.stderr[-3000:]
    line, plain = json.loads(with_opt.stdout.strip().splitlines()[-1]), json.loads(without.stdout.strip().splitlines()[-1])
    for k in ("fr_stat", "fr_maxllh"):
        with open(line[k], "rb") as fa, open(plain[k], "rb") as fb:
            assert fa.read() == fb.read(), k
    assert "evidence_realisations" not in plain
    toys = line["evidence_realisations"]
    assert os.path.dirname(toys["file"]) == os.path.dirname(line["fr_stat"]) and os.path.basename(toys["file"]).startswith("fr_evidence_realisations")
    z = np.load(toys["file"])
    scales = nested.sens_scales(6, 4)
    asimov, ps = Cf.sens_paramsets(6, fr_utils.normalize_fr((1., 1., 1.)))
    meas = R.draw_realisations(TR.model_bf(asimov), 0.1, 3, seed=2)
    assert np.array_equal(z["scales"], scales) and np.array_equal(z["measurements"], meas) and z["smearings"].tolist() == [0.1] * 3
    for k in ("lnz", "ess", "ess_fraction", "kept", "bayes"):
        assert z[k].shape == (3, 4), k
    assert z["limits"].shape == (3,) and z["discovered"].shape == (3,) and np.array_equal(z["lnz_run"], np.load(line["fr_stat"])[:, 1])
    assert toys["n"] == 3 and toys["seed"] == 2 and toys["band_quantiles"] == [2.5, 16., 50., 84., 97.5]
    assert toys["without_limit"] == int(np.isnan(z["limits"]).sum())
    # the library call reproduces the file
    args = TR.sens_args(smearing=0.1)
    args.seed, args.mn_live_points, args.mn_walks = 3, 128, 10
    ref = R.evidence_realisation_scan(args, asimov, ps, scales, measurements=meas, run_ids=np.arange(4))
    for s_ in range(4):
        assert H.same_bits(z["lnz"][:, s_], ref["lnz"][:, s_]), s_
    assert np.array_equal(z["limits"], ref["limits"], equal_nan=True)
