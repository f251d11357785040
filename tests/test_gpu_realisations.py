"""Realisation ensembles on the GPU (gf_toys.hip, gf_toys_set_measurements, golemflavor_amd.realisations): the device
selection against the host build of gf_toys.hpp, the scores against the bulk lnprob of a model compiled with the realisation, the scan
against profile_scan and against stand-alone maximisers of such models, independence of batching and company, the refusals and the
CLI.  Every comparison is of bits."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toys_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import nested
from golemflavor_amd import profile_llh as P
from golemflavor_amd import realisations as R
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHUNK = 1024                   # gf_toys.hpp: seeds per part of the seed range


def sens_args(texture=Texture.OET, smearing=0.02):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=texture,
                              binning=Cf.default_bin_edges(), smearing=smearing, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


def sens_desc(args, ps, bf, smearing):
    """the sens posterior of `ps` (its scale column fixed) under the measurement (bf, smearing)"""
    return compile_model(ps, "BSM_GAUSS", bestfit_fr=bf, smearing=smearing, source_ratio=args.source_ratio, texture=args.texture,
                         dimension=args.dimension, binning=args.binning)


def model_bf(asimov):
    return fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))


@pytest.fixture(scope="module")
def oeu_scale():
    """texture OEU: the first scale where a few per cent of the prior draws fail the reference's unitarity assert and some lnprob is
    finite (tests/test_gpu_profile.py's _oeu_nonunitary_scale)."""
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
    raise AssertionError("no scale with non-unitary draws")


# ---- 1. the selection ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return H.build()


def check_selection(host, lp, fr, status, bf, sm, off, K, what):
    want = H.host_select(lp, fr, status, H.measurements(bf, sm, off), K, host)
    got = R.toy_select(lp, fr, status, bf, sm, off, K)
    for g, w, name in zip(got, want, ("index", "score", "count")):
        assert H.same_bits(g, w), (what, name)
    return got


@pytest.mark.parametrize("K", [1, 4, 16])
def test_selection_equals_the_host_build(host, K):
    """gf_toy_select against the host build of gf_toys.hpp on crafted seed sets (ties between indices, -inf, NaN, non-unitary rows,
    Gaussians at -inf): indices, scores and counts, at every lane count around a wave and every seed count around K, a tile and a
    part of the seed range."""
    nseeds = [1, K - 1, K, 255, 256, 257, CHUNK + 1, 3 * CHUNK + 5]
    for ntoys in (1, 63, 64, 65, 130):
        for nseed in nseeds:
            lp, fr, status, bf, sm, off = H.crafted(max(nseed, 1), ntoys, seed=1000 * K + 7 * ntoys + nseed)
            if nseed == 0:                                          # K - 1 at K = 1: no seed set
                with pytest.raises(_lib.GolemHipError):
                    R.toy_select(lp[:0], fr[:0], status[:0], bf, sm, off, K)
                continue
            index, score, count = check_selection(host, lp, fr, status, bf, sm, off, K, (ntoys, nseed))
            if nseed >= 255:
                assert np.all(count == K), (ntoys, nseed)
    for kind, nseed in (("ties", 3 * CHUNK + 5), ("neginf", CHUNK + 1), ("ties", 257), ("neginf", 256)):
        lp, fr, status, bf, sm, off = H.crafted(nseed, 65, seed=50 + K, kind=kind)
        index, score, count = check_selection(host, lp, fr, status, bf, sm, off, K, (kind, nseed))
        if kind == "ties":
            assert np.all(index == np.arange(K))
        else:
            assert np.all(count == 0) and np.all(index == -1)


def check_handle_against_standalone(sel, sd, standalone, K):
    """A seed set's select() (sel; sd: its scales' seeds()) against standalone(s), the stand-alone selection of scale s's seeds under the
    same measurements: index, score and count bit for bit, and the cube points gathered from the selected seeds, NaN behind the count."""
    for s in range(len(sd)):
        index, score, count = standalone(s)
        assert np.array_equal(sel["index"][s], index) and H.same_bits(sel["score"][s], score) and np.array_equal(sel["count"][s], count), s
        have = np.arange(K)[None, :] < count[:, None]
        assert np.array_equal(index >= 0, have) and np.all(index[~have] == -1) and np.all(score[~have] == -np.inf)
        assert H.same_bits(sel["cube"][s][have], sd[s]["cube"][index[have]]) and np.isnan(sel["cube"][s][~have]).all(), s


@pytest.mark.parametrize("K", [1, 5])
def test_handle_selection_equals_the_standalone_selection(oeu_scale, K):
    """The two routes through the selection: ToySeeds.select over two scales, with shared and with per-scale measurements, against
    toy_select per scale on that scale's seeds() arrays and the set's offset.  CHUNK + 1 seeds are two parts of the seed range, the second
    of one seed; 65 realisations are two workgroups of the select kernel, the second with one live lane.  The last two realisations are
    narrow: one leaves scale 0 a few finite seeds, the other leaves no scale any."""
    args = sens_args(texture=Texture.OEU, smearing=0.05)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    M, T, sm = CHUNK + 1, 65, 0.008
    cols, models, bases, _ = nested._scan_models(args, asimov, ps, np.array([oeu_scale - 0.5, oeu_scale]), 0.05, 0)
    try:
        off = float(getattr(models[0], "model", models[0]).desc.offset)
        with R.ToySeeds(models, cols, bases, nseed=M, seed=11) as seeds:
            sd = [seeds.seeds(s) for s in range(2)]
            fr = sd[0]["fr"][sd[0]["status"] == _lib.GF_ST_OK]
            mh, k = H.gauss_consts(sm)
            centre, u = fr.mean(axis=0), np.array([1., -1., 0.]) / np.sqrt(2.)
            # a measurement centre + D u leaves seed i above the underflow wall (-1075 ln 2) exactly when D < cross_i, for D of that size
            q = (fr - centre) @ u
            with np.errstate(invalid="ignore"):
                cross = q + np.sqrt((-745.1332191019411 - k) / mh - (np.sum((fr - centre) ** 2, axis=1) - q * q))
            cross = np.sort(cross[np.isfinite(cross)])
            few = 0.5 * (cross[-4] + cross[-3])
            sms = np.full(T, 0.05)
            sms[-2:] = sm
            shared = R.draw_realisations(model_bf(asimov), 0.05, T, seed=21)
            shared[-2:] = centre + few * u, centre + 2.0 * u
            other = R.draw_realisations(model_bf(asimov), 0.05, T, seed=22)
            other[-1] = centre + 2.0 * u
            for meas in (shared, np.stack([shared, other])):
                sel = seeds.select(meas, sms, K)
                assert sel["cube"].shape == (2, T, K, len(cols))
                check_handle_against_standalone(sel, sd, lambda s: R.toy_select(sd[s]["lp"], sd[s]["fr"], sd[s]["status"],
                                                                                meas[s] if meas.ndim == 3 else meas, sms, off, K), K)
                print("K = %d, %s measurements: counts of the narrow realisations %s" % (K, "per-scale" if meas.ndim == 3 else "shared",
                                                                                         sel["count"][:, -2:].tolist()))
                # conditions on the inputs: full lists, a list cut short by the wall, and empty ones
                assert np.any(sel["count"] == K) and sel["count"][0, -2] == min(K, 3) and np.all(sel["count"][:, -1] == 0)
    finally:
        for m in models:
            m.close()


# ---- 2. the score ----------------------------------------------------------------------------------------------------------------------
def check_scores(seeds, make_model, meas, sms, what):
    """seeds: a ToySeeds of one scale.  scores[t] against the bulk lnprob of a model compiled with (meas[t], sms[t]) at the seeds' theta,
    and the selection against the ranking of those values."""
    sd = seeds.seeds(0)
    scores = seeds.scores(meas, sms)[0]
    sel = seeds.select(meas, sms, 4)
    nfinite = 0
    for t in range(len(meas)):
        with make_model(meas[t], sms[t]) as m:
            lp, st = m.lnprob(sd["theta"], want_status=True)
        assert np.array_equal(st, sd["status"])                    # the verdicts do not depend on the measurement
        want = np.where((st == _lib.GF_ST_NON_UNITARY) | np.isnan(lp), -np.inf, lp)
        differ = np.sum(scores[t].view(np.int64) != want.view(np.int64))
        print("%s realisation %d: %d seeds, %d finite, %d non-unitary, %d scores differ from Model.lnprob" %
              (what, t, len(lp), np.isfinite(want).sum(), (st == _lib.GF_ST_NON_UNITARY).sum(), differ))
        assert H.same_bits(scores[t], want), (what, t, differ)
        windex, wscore, wcount = H.lexsort_select(want[None], 4)
        assert np.array_equal(sel["index"][0, t], windex[0]) and H.same_bits(sel["score"][0, t], wscore[0]) and sel["count"][0, t] == wcount[0]
        have = windex[0] >= 0
        assert H.same_bits(sel["cube"][0, t][have], sd["cube"][windex[0][have]])
        nfinite += int(np.isfinite(want).sum())
    return nfinite


def test_score_equals_model_lnprob_notebook():
    """SM: the notebook posterior, 256 seeds over all six columns, 3 realisations with smearings of their own."""
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    bf = fr_utils.angles_to_fr(asimov.values)
    meas = R.draw_realisations(bf, 0.05, 3, seed=2)
    sms = np.array([0.02, 0.05, 0.1])
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=0.02)) as m0:
        with R.ToySeeds([m0], np.arange(6), np.array(ps.values, dtype=float), nseed=256, seed=4) as seeds:
            lp0 = m0.lnprob(seeds.seeds(0)["theta"], want_status=False)
            assert H.same_bits(seeds.seeds(0)["lnprob"], lp0)
            n = check_scores(seeds, lambda b, s: Model(compile_model(ps, "SM_GAUSS", bestfit_fr=b, smearing=s)), meas, sms, "notebook")
    assert n > 300                                                  # the wide realisations keep most seeds above the underflow wall


def test_score_equals_model_lnprob_sens(oeu_scale):
    """BSM: the sens posterior, texture OEU at a scale where seeds fail the unitarity assert: 256 seeds, 3 realisations."""
    args = sens_args(texture=Texture.OEU)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    sp = nested._scale_paramset(ps, oeu_scale)
    names = list(sp.names)
    cols = [i for i in range(len(names)) if names[i] != "logLam"]
    bf = model_bf(asimov)
    meas = R.draw_realisations(bf, 0.05, 3, seed=3)
    sms = np.array([0.02, 0.05, 0.1])
    with Model(sens_desc(args, sp, bf, 0.02)) as m0:
        with R.ToySeeds([m0], cols, np.array(sp.values, dtype=float), nseed=256, seed=6) as seeds:
            assert seeds.nonunitary_seeds[0] == np.sum(seeds.seeds(0)["status"] == _lib.GF_ST_NON_UNITARY) > 0
            n = check_scores(seeds, lambda b, s: Model(sens_desc(args, sp, b, s)), meas, sms, "sens OEU")
    assert n > 100


# ---- 3. the anchor ---------------------------------------------------------------------------------------------------------------------
OPTS = dict(maxiter=200, restarts=1, adaptive=True)


def test_own_measurement_equals_profile_scan():
    """One realisation that is the model's own measurement: the scan is profile_scan's, bit for bit."""
    args = sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)
    ref = P.profile_scan(args, asimov, ps, scales, run_ids=np.arange(4), nstarts=4, nseed=512, seed=9, on_nonunitary="-inf", **OPTS)
    res = R.realisation_scan(args, asimov, ps, scales, measurements=[model_bf(asimov)], smearings=[0.1], nstarts=4, nseed=512, seed=9,
                             run_ids=np.arange(4), on_nonunitary="-inf", **OPTS)
    assert np.all(np.isfinite(ref["max_lnl"])) and np.all(ref["nstarts"] == 4)
    assert H.same_bits(res["max_lnl"][0], ref["max_lnl"])
    assert H.same_bits(res["argmax_theta"][0], ref["argmax_theta"])
    for k in ("niter", "nfev", "nstarts"):
        assert np.array_equal(res[k][0], ref[k]), k
    assert np.array_equal(res["nonunitary"][0].astype(np.int64) + res["nonunitary_seeds"], ref["nonunitary"])
    assert res["ts"].shape == (1, 4) and res["ts"][0, 0] == 0.0
    assert H.same_bits(res["ts"][0], -2.0 * (ref["max_lnl"] - ref["max_lnl"][0]))
    lim = P.profile_likelihood_limit(scales, ref["max_lnl"])
    assert (np.isnan(res["limits"][0]) and lim is None) or res["limits"][0] == lim


# ---- 4. the per-run measurement ----------------------------------------------------------------------------------------------------------
def check_against_standalone(args, scales, meas, sms, seed, nstarts=4, nseed=512):
    """Every (t, s) of a scan against a maximiser of its own over Model_t_s, the sens posterior compiled with (m_t, smearing_t), from the
    same selected seeds; and max_lnl against that model's bulk lnprob of argmax_theta (DESIGN.md 6i's invariant)."""
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    res = R.realisation_scan(args, asimov, ps, scales, measurements=meas, smearings=sms, nstarts=nstarts, nseed=nseed, seed=seed,
                             on_nonunitary="-inf", **OPTS)
    T, S = res["max_lnl"].shape
    assert (T, S) == (len(meas), len(scales))
    for s in range(S):
        sp = nested._scale_paramset(ps, float(scales[s]))
        names = list(sp.names)
        cols = [i for i in range(len(names)) if names[i] != "logLam"]
        base = np.array(sp.values, dtype=float)
        for t in range(T):
            c = int(res["start_count"][t, s])
            if c == 0:                                                   # no seed with a finite value under this realisation: no run
                assert res["max_lnl"][t, s] == -np.inf and res["nstarts"][t, s] == 0 and np.isnan(res["argmax_theta"][t, s][cols]).all()
                assert res["nfev"][t, s] == 0 and res["niter"][t, s] == 0 and not res["failed"][t, s]
                continue
            with Model(sens_desc(args, sp, meas[t], sms[t])) as m:
                with P.SimplexMaximizer([m], cols, base, nstarts=0, nseed=0, starts=res["start_cube"][t, s, :c][None], on_nonunitary="-inf",
                                        **OPTS) as mx:
                    one = mx.run()
                for k in ("max_lnl", "argmax_theta"):
                    assert H.same_bits(res[k][t, s], one[k][0]), (k, t, s)
                for k in ("niter", "nfev", "nstarts", "nonunitary", "parked"):
                    assert res[k][t, s] == one[k][0], (k, t, s, res[k][t, s], one[k][0])
                assert np.isfinite(res["max_lnl"][t, s])
                assert H.same_bits(m.lnprob(res["argmax_theta"][t, s][None], want_status=False), res["max_lnl"][t, s:s + 1]), (t, s)
    return res


def test_per_run_measurement_equals_standalone_models_oet():
    scales = nested.sens_scales(6, 4)[[0, 2]]
    meas = R.draw_realisations((1 / 3, 1 / 3, 1 / 3), 0.1, 3, seed=12)
    check_against_standalone(sens_args(smearing=0.1), scales, meas, np.array([0.1, 0.08, 0.12]), seed=3)


def test_per_run_measurement_equals_standalone_models_oeu_parked(oeu_scale):
    """texture OEU where a few per cent of the cube is non-unitary, on "-inf": candidates are parked and settled under the run's own
    measurement."""
    scales = np.array([oeu_scale - 0.5, oeu_scale])
    meas = R.draw_realisations((1 / 3, 1 / 3, 1 / 3), 0.05, 3, seed=13)
    res = check_against_standalone(sens_args(texture=Texture.OEU, smearing=0.05), scales, meas, np.array([0.05, 0.04, 0.06]), seed=5)
    print("OEU: parked %s, non-unitary %s, seeds %s" % (res["parked"].tolist(), res["nonunitary"].tolist(), res["nonunitary_seeds"].tolist()))
    assert res["parked"].sum() > 0


def test_fewer_finite_seeds_than_starts():
    """24 seeds, 8 starts asked for, and narrow realisations placed so that the underflow wall of their Gaussian (37.6 smearings from the
    measurement) cuts through the null scale's cloud of seed compositions: the runs of one maximiser keep different numbers of starts,
    and each still equals a maximiser of its own from exactly those."""
    args = sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)[[0, 2]]
    cols, models, bases, _ = nested._scan_models(args, asimov, ps, scales, 0.1, 0)
    try:
        with R.ToySeeds(models, cols, bases, nseed=24, seed=3) as seeds:
            fr = seeds.seeds(0)["fr"]
    finally:
        for m in models:
            m.close()
    assert np.isfinite(fr).all()
    sm = 0.008
    mh, k = H.gauss_consts(sm)
    centre, u = fr.mean(axis=0), np.array([1., -1., 0.]) / np.sqrt(2.)

    def nfinite(d):                                                   # seeds above the wall under a measurement d along u from the cloud
        return int(np.sum(mh * np.sum((fr - (centre + d * u)) ** 2, axis=1) + k > -745.0))
    ds = np.arange(0.0, 1.0, 0.001)
    n = np.array([nfinite(d) for d in ds])
    few, some = ds[np.argmax((n >= 1) & (n <= 3))], ds[np.argmax((n >= 4) & (n <= 7))]
    assert 1 <= nfinite(few) <= 3 and 4 <= nfinite(some) <= 7, (n.tolist())
    meas = np.array([centre, centre + some * u, centre + few * u, centre + 2.0 * u])
    res = check_against_standalone(args, scales, meas, np.array([0.1, sm, sm, sm]), seed=3, nstarts=8, nseed=24)
    counts = res["start_count"]
    print("starts kept per (realisation, scale): %s" % counts.tolist())
    assert np.array_equal(res["nstarts"], counts)
    assert counts[0, 0] == 8 and 4 <= counts[1, 0] <= 7 and 1 <= counts[2, 0] <= 3 and counts[3, 0] == 0    # a condition on the inputs


# ---- 5. independence -------------------------------------------------------------------------------------------------------------------
KEYS = ("max_lnl", "ts", "argmax_theta", "nstarts", "nfev", "niter", "nonunitary", "parked", "failed", "limits", "start_cube", "start_score",
        "start_count")


def test_batching_and_company_change_nothing():
    args = sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)
    meas = R.draw_realisations(model_bf(asimov), 0.1, 5, seed=21)
    kw = dict(nstarts=4, nseed=512, seed=9, on_nonunitary="-inf", maxiter=100, restarts=1, adaptive=True)

    def scan(m, **more):
        return R.realisation_scan(args, asimov, ps, scales, measurements=m, **kw, **more)

    def same(a, b, rows=slice(None)):
        for k in KEYS:
            x, y = np.asarray(a[k])[rows], np.asarray(b[k])
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype == np.float64), k
    a = scan(meas)
    assert np.all(np.isfinite(a["max_lnl"])) and np.all(a["ts"][:, 0] == 0.0)
    assert len(np.unique(a["max_lnl"][:, 1])) == 5                      # the realisations are not copies of each other
    same(a, scan(meas))                                                 # two identical calls
    same(a, scan(meas, batch=2))                                        # maximisers of 2 + 2 + 1 realisations
    same(a, scan(meas[:2]), slice(0, 2))                                # calls of 2 + 3
    same(a, scan(meas[2:]), slice(2, 5))
    same(a, scan(meas[3:4]), slice(3, 4))                               # a realisation on its own
    per_scale = scan(np.tile(meas[None], (4, 1, 1)))                    # [S][T][3] with the same throws at every scale
    same(a, per_scale)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    args = sens_args(smearing=0.1)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, 4)[:2]
    cols, models, bases, _ = nested._scan_models(args, asimov, ps, scales, 0.1, 0)
    bf = np.tile(model_bf(asimov), (2, 1))
    starts = np.full((2, 1, len(cols)), 0.5)
    try:
        # nseed > 0: the set's own seeding would score under the models' measurement
        with P.SimplexMaximizer(models, cols, bases, nstarts=2, nseed=64) as mx:
            with pytest.raises(_lib.GolemHipError, match="seed points"):
                mx.set_measurements(bf, 0.1)
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts, maxiter=5, restarts=0) as mx:
            for bad in (0.0, -0.1, np.inf, np.nan):
                with pytest.raises(_lib.GolemHipError, match="smearing > 0"):
                    mx.set_measurements(bf, [0.1, bad])
            with pytest.raises(_lib.GolemHipError, match="finite measurement"):
                mx.set_measurements([[0.3, 0.3, np.nan], [0.3, 0.3, 0.4]], 0.1)
            mx.set_measurements(bf, 0.1)                                 # accepted, and again
            mx.set_measurements(bf, [0.1, 0.2])
            mx.run()
            with pytest.raises(_lib.GolemHipError, match="before the first run"):
                mx.set_measurements(bf, 0.1)
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts) as mx:
            for bad in ([0, 2], [-1, 1]):
                with pytest.raises(_lib.GolemHipError, match="keeps"):
                    _lib.check(mx._L.gf_toys_set_start_counts(mx._h, np.array(bad, np.int32).ctypes.data_as(_lib._ip)), "counts")
        with P.SimplexMaximizer(models, cols, bases, nstarts=2, nseed=64) as mx:
            with pytest.raises(_lib.GolemHipError, match="of its own"):
                _lib.check(mx._L.gf_toys_set_start_counts(mx._h, np.array([0, 0], np.int32).ctypes.data_as(_lib._ip)), "counts")
        # K beyond GF_TOY_MAX_STARTS
        with R.ToySeeds(models, cols, bases, nseed=64, seed=1) as seeds:
            for K in (0, 17):
                with pytest.raises(_lib.GolemHipError, match="1 to 16"):
                    seeds.select(bf, 0.1, K)
            with pytest.raises(_lib.GolemHipError, match="smearing > 0"):
                seeds.select(bf, [0.1, 0.0], 4)
            assert seeds.select(bf, 0.1, 16)["count"].shape == (2, 2)
        lp, fr, status, tbf, sm, off = H.crafted(40, 3, seed=1)
        with pytest.raises(_lib.GolemHipError, match="1 to 16"):
            R.toy_select(lp, fr, status, tbf, sm, off, 17)
        with pytest.raises(ValueError, match="1 to 16"):
            R.realisation_scan(args, asimov, ps, scales, ntoys=2, nstarts=17)
        # a binned set
        binned = llh_utils.BinnedMeasurement.constant(model_bf(asimov), 0.1, np.asarray(args.binning, dtype=float))
        for m in models:
            m.set_binned_measurement(binned)
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts) as mx:
            with pytest.raises(_lib.GolemHipError, match="binned measurement"):
                mx.set_measurements(bf, 0.1)
        with pytest.raises(_lib.GolemHipError, match="binned measurement"):
            R.ToySeeds(models, cols, bases, nseed=64)
        with pytest.raises(ValueError, match="energy-resolved"):
            R.realisation_scan(args, asimov, ps, scales, ntoys=2, binned=binned)
    finally:
        for m in models:
            m.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------------------
def test_sens_cli_realisations_end_to_end(tmp_path):
    cmd = [sys.executable, "-m", "golemflavor_amd.sens", "--stat-method", "frequentist", "--segments", "4", "--smearing", "0.1",
           "--pl-starts", "4", "--pl-seed-points", "512", "--realisations", "3", "--realisation-starts", "4", "--realisation-seed", "2",
           "--datadir", str(tmp_path), "--seed", "3"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    toys = line["realisations"]
    assert os.path.dirname(toys["file"]) == os.path.dirname(line["fr_maxllh"]) and os.path.basename(toys["file"]).startswith("fr_realisations")
    z = np.load(toys["file"])
    scales = nested.sens_scales(6, 4)
    assert np.array_equal(z["scales"], scales) and z["measurements"].shape == (3, 3) and z["smearings"].tolist() == [0.1] * 3
    for k in ("max_lnl", "ts", "nstarts", "nfev", "niter", "nonunitary", "failed"):
        assert z[k].shape == (3, 4), k
    assert z["argmax_theta"].shape[:2] == (3, 4) and z["limits"].shape == (3,) and z["nonunitary_seeds"].shape == (4,)
    assert np.all(z["ts"][:, 0] == 0.0) and np.all(np.isfinite(z["max_lnl"])) and np.all(z["nstarts"] == 4)
    asimov, _ = Cf.sens_paramsets(6, fr_utils.normalize_fr((1., 1., 1.)))
    assert np.array_equal(z["measurements"], R.draw_realisations(model_bf(asimov), 0.1, 3, seed=2))
    assert toys["band_quantiles"] == [2.5, 16., 50., 84., 97.5] and len(toys["band_limits"]) == 5
    assert toys["n"] == 3 and toys["without_limit"] == int(np.isnan(z["limits"]).sum()) and len(toys["ts_q95"]) == 4
    band = R.sensitivity_band(z["limits"])
    assert np.array_equal(np.asarray(toys["band_limits"], dtype=float), band["limits"], equal_nan=True)
    # the Asimov outputs are what the command writes without --realisations
    mx = np.load(line["fr_maxllh"])
    assert mx.shape == (4, 2) and np.array_equal(mx[:, 0], scales) and np.array_equal(mx[:, 1], np.asarray(line["max_lnl"]))
