"""Realisation ensembles of the energy-resolved likelihood on the GPU (gf_toys_binned.hip, gf_toys_set_binned_measurements,
golemflavor_amd.realisations): the scores against the bulk lnprob of a model given the realisation, the device selection against the host
build of gf_toys_binned.hpp, the scan against profile_scan(binned=) and against stand-alone maximisers of such models, independence of
batching and company, the start counts, the refusals and the CLI.  Every comparison is of bits.

The set-up is tests/test_gpu_realisations.py's: the sens posterior of dimension 6, texture OEU at a scale inside the region where the
reference's unitarity assert fails for a few per cent of the prior draws, so that every test has seeds the reference would have raised
on -- each asserts that it has."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toys_binned_harness as H
from test_gpu_realisations import check_handle_against_standalone
from test_gpu_realisations import model_bf, oeu_scale, sens_args, sens_desc  # noqa: F401  (oeu_scale is a fixture)
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import nested
from golemflavor_amd import profile_llh as P
from golemflavor_amd import realisations as R
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.llh import BinnedMeasurement
from golemflavor_amd.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHUNK = 1024                   # gf_toys.hpp: seeds per part of the seed range
WALL = -745.1332191019411      # the underflow wall of a Gaussian term, -1075 ln 2: below it log(exp(.)) is -inf
U = np.array([1., -1., 0.]) / np.sqrt(2.)
OPTS = dict(maxiter=200, restarts=1, adaptive=True)


def oeu_args(nbins=20, smearing=0.1):
    args = sens_args(texture=Texture.OEU, smearing=smearing)
    args.binning = Cf.default_bin_edges((6e4, 1e7, nbins))
    return args


def own_measurement(args, asimov):
    return BinnedMeasurement.constant(model_bf(asimov), args.smearing, np.asarray(args.binning, dtype=float))


def wall_crossings(frb, sigma):
    """The bin in which the seeds' compositions frb [n][nb][3] spread widest along U, and the throws that put the wall through them: a
    measurement c + D U of that bin with width sigma, c the seeds' mean there, leaves seed i above the wall (a finite term) exactly when
    D < D_i.  Returns (bin, c, D_i).  Plain numpy: it places the test's inputs, it checks nothing."""
    mh, k = H.gauss_consts(sigma)
    b = int(np.argmax((frb @ U).std(axis=0)))
    fr_k = frb[:, b]
    c = fr_k.mean(axis=0)
    q = (fr_k - c) @ U
    perp2 = np.sum((fr_k - c) ** 2, axis=1) - q * q
    with np.errstate(invalid="ignore"):
        return b, c, q + np.sqrt((WALL - k) / mh - perp2)


def scale_models(args, scales, binned):
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    return nested._scan_models(args, asimov, ps, np.asarray(scales, dtype=float), args.smearing, 0, binned=binned)


def failing_scale(args, binned):
    """oeu_scale's search for another binning (the verdict is per energy bin, so the failing region moves with the bins): the first scale
    where a few per cent of the seed points fail the reference's unitarity assert and some lnprob is finite."""
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    for s_ in np.linspace(lo, hi, 27):
        cols, models, bases, _ = scale_models(args, [s_], binned)
        try:
            with R.BinnedToySeeds(models, cols, bases, nseed=2000, seed=5) as seeds:
                if seeds.nonunitary_seeds[0] > 40 and np.any(np.isfinite(seeds.seeds(0)["lnprob"])):
                    return float(s_)
        finally:
            models[0].close()
    raise AssertionError("no scale with non-unitary seeds")


# ---- 1. the score ----------------------------------------------------------------------------------------------------------------------
SCORE_CASES = {
    # nbins, seeds, realisations, per-scale throws, per-realisation widths
    "20 bins, one part, ragged tile": (20, 600, 3, False, False),
    "20 bins, across a part, across a wave": (20, 1100, 70, True, True),
    "3 bins": (3, 600, 3, False, True),
    "64 bins, the LDS limit": (64, 1100, 3, True, False),
}


@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_scores_equal_model_lnprob(oeu_scale, case):
    """BinnedToySeeds.scores against Model_{s,t}.lnprob at the seeds' theta, Model_{s,t} the scale's model given realisation t; -inf where
    the model reports non-unitary.  One realisation has a bin narrowed and thrown to the underflow wall's distance from the seeds'
    compositions there, so that the wall cuts through them.  And select against np.lexsort of those scores."""
    nb, M, T, per_scale, per_toy = SCORE_CASES[case]
    args = oeu_args(nb)
    asimov, _ = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    top = oeu_scale if nb >= 20 else failing_scale(args, binned)
    scales = [top - 0.5, top]
    cols, models, bases, _ = scale_models(args, scales, binned)
    rng = np.random.default_rng(nb + M)
    try:
        with R.BinnedToySeeds(models, cols, bases, nseed=M, seed=6) as seeds:
            sd = [seeds.seeds(s) for s in range(2)]
            assert seeds.nonunitary_seeds.sum() > 0, "the case needs seeds the reference would have raised on"
            for s in range(2):
                assert seeds.nonunitary_seeds[s] == np.sum(sd[s]["status"] == _lib.GF_ST_NON_UNITARY)
                assert sd[s]["fr_bins"].shape == (M, nb, 3)
                ok = sd[s]["status"] == _lib.GF_ST_OK
                assert np.isfinite(sd[s]["fr_bins"][ok]).all() and np.isnan(sd[s]["fr_bins"][~ok]).all()
            meas = R.draw_binned_realisations(binned, T, seed=3)
            if per_scale:
                meas = np.stack([meas, R.draw_binned_realisations(binned, T, seed=4)])
            sig = binned.sigma * (1.0 + 0.5 * rng.random((T, nb))) if per_toy else binned.sigma.copy()
            if per_toy:
                # realisation 1, one bin: narrow, and thrown so far that the wall passes through scale 0's compositions there
                b, c, cross = wall_crossings(sd[0]["fr_bins"][sd[0]["status"] == _lib.GF_ST_OK], 0.01)
                sig[1, b] = 0.01
                (meas[0] if per_scale else meas)[1, b] = c + np.nanmedian(cross) * U
            scores = seeds.scores(meas, sig)
            sel = seeds.select(meas, sig, 4)
        assert scores.shape == (2, T, M)
        sgs = np.broadcast_to(sig, (T, nb))
        differ = nfinite = 0
        for s in range(2):
            for t in range(T):
                m_t = meas[s, t] if per_scale else meas[t]
                models[s].set_binned_measurement(BinnedMeasurement(m_t, sgs[t]))
                lp, st = models[s].lnprob(sd[s]["theta"], want_status=True)
                assert np.array_equal(st, sd[s]["status"])                # the verdicts do not depend on the measurement
                want = np.where((st == _lib.GF_ST_NON_UNITARY) | np.isnan(lp), -np.inf, lp)
                differ += int(np.sum(scores[s, t].view(np.int64) != want.view(np.int64)))
                nfinite += int(np.isfinite(want).sum())
                assert H.same_bits(scores[s, t], want), (case, s, t)
                windex, wscore, wcount = H.lexsort_select(want[None], 4)
                assert np.array_equal(sel["index"][s, t], windex[0]) and H.same_bits(sel["score"][s, t], wscore[0]) and sel["count"][s, t] == wcount[0]
                have = windex[0] >= 0
                assert H.same_bits(sel["cube"][s, t][have], sd[s]["cube"][windex[0][have]])
                if per_toy and s == 0 and t == 1:
                    # the wall cuts through scale 0's seeds: some unitary in-box seeds are -inf under this realisation alone, others finite
                    inbox = (st == _lib.GF_ST_OK) & np.isfinite(sd[s]["lp"])
                    walled = inbox & (want == -np.inf)
                    print("%s: the wall takes %d of %d in-box seeds" % (case, walled.sum(), inbox.sum()))
                    assert walled.sum() > 0 and (inbox & np.isfinite(want)).sum() > 0
        print("%s: %d scores, %d finite, %d non-unitary seeds, %d differ from Model.lnprob" % (case, scores.size, nfinite,
                                                                                                 int(seeds.nonunitary_seeds.sum()), differ))
        assert nfinite > T * M // 4
    finally:
        for m in models:
            m.close()


# ---- 2. the selection ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return H.build()


def check_selection(host, lp, frb, status, meas, sigma, off, K, what):
    want = H.host_select(lp, frb, status, H.table(meas, sigma), off, K, host)
    got = R.toy_select_binned(lp, frb, status, meas, sigma, off, K)
    for g, w, name in zip(got, want, ("index", "score", "count")):
        assert H.same_bits(g, w), (what, name)
    return got


@pytest.mark.parametrize("K", [1, 4, 5, 16])
def test_selection_equals_the_host_build(host, K):
    """gf_toy_select_binned against the host build of gf_toys_binned.hpp on the host test's crafted seed sets (ties between indices, -inf,
    NaN in lp and in single bins, non-unitary rows, single bins at the wall): at lane counts around a wave, at seed counts around K, a
    tile and a part of the seed range, with shared and per-realisation widths."""
    for ntoys, per_toy in ((1, False), (65, True), (130, False)):
        for nseed in (1, K, 31, 33, 600, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37):
            lp, frb, status, meas, sigma, off = H.crafted(nseed, ntoys, 5, seed=1000 * K + 7 * ntoys + nseed, per_toy_sigma=per_toy)
            index, score, count = check_selection(host, lp, frb, status, meas, sigma, off, K, (ntoys, nseed))
            if nseed >= 600:
                assert np.all(count == K), (ntoys, nseed)
    for kind, nseed in (("ties", 2 * CHUNK + 5), ("neginf", CHUNK + 1), ("ties", 33), ("neginf", 32)):
        lp, frb, status, meas, sigma, off = H.crafted(nseed, 65, 7, seed=50 + K, kind=kind)
        index, score, count = check_selection(host, lp, frb, status, meas, sigma, off, K, (kind, nseed))
        if kind == "ties":
            assert np.all(index == np.arange(K))
        else:
            assert np.all(count == 0) and np.all(index == -1)
    # the host test's own case
    lp, frb, status, meas, sigma, off = H.crafted(700, 130, 5, seed=3, per_toy_sigma=True)
    check_selection(host, lp, frb, status, meas, sigma, off, K, "host case")


@pytest.mark.parametrize("K", [1, 5])
def test_handle_selection_equals_the_standalone_selection(oeu_scale, K):
    """The two routes through the selection, at 3 energy bins: BinnedToySeeds.select over two scales, with shared and with per-scale
    measurements, against toy_select_binned per scale on that scale's seeds() arrays and the set's offset.  CHUNK + 1 seeds are two
    parts of the seed range, the second of one seed; 65 realisations are two workgroups of the select kernel, the second with one live
    lane.  The last two realisations have one narrow bin: thrown so that the wall leaves scale 0 three finite seeds, and so far that no
    scale keeps any."""
    args = oeu_args(3)
    asimov, _ = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    M, T, nb = CHUNK + 1, 65, 3
    cols, models, bases, _ = scale_models(args, [oeu_scale - 0.5, oeu_scale], binned)
    try:
        off = float(getattr(models[0], "model", models[0]).desc.offset)
        with R.BinnedToySeeds(models, cols, bases, nseed=M, seed=11) as seeds:
            sd = [seeds.seeds(s) for s in range(2)]
            b, c, cross = wall_crossings(sd[0]["fr_bins"][sd[0]["status"] == _lib.GF_ST_OK], 0.01)
            cross = np.sort(cross[np.isfinite(cross)])
            sig = np.broadcast_to(binned.sigma, (T, nb)).copy()
            sig[-2:, b] = 0.01
            shared = R.draw_binned_realisations(binned, T, seed=21)
            shared[-2, b], shared[-1, b] = c + 0.5 * (cross[-4] + cross[-3]) * U, c + 2.0 * U
            other = R.draw_binned_realisations(binned, T, seed=22)
            other[-1, b] = c + 2.0 * U
            for meas in (shared, np.stack([shared, other])):
                sel = seeds.select(meas, sig, K)
                assert sel["cube"].shape == (2, T, K, len(cols))
                check_handle_against_standalone(sel, sd, lambda s: R.toy_select_binned(sd[s]["lp"], sd[s]["fr_bins"], sd[s]["status"],
                                                                                       meas[s] if meas.ndim == 4 else meas, sig, off, K), K)
                print("K = %d, %s measurements: counts of the narrow realisations %s" % (K, "per-scale" if meas.ndim == 4 else "shared",
                                                                                         sel["count"][:, -2:].tolist()))
                # conditions on the inputs: full lists, a list cut short by the wall, and empty ones
                assert np.any(sel["count"] == K) and sel["count"][0, -2] == min(K, 3) and np.all(sel["count"][:, -1] == 0)
    finally:
        for m in models:
            m.close()


# ---- 3. the anchor ---------------------------------------------------------------------------------------------------------------------
def test_own_measurement_equals_profile_scan(oeu_scale):
    """One realisation that is the model's own binned measurement: the scan is profile_scan(binned=)'s, bit for bit."""
    args = oeu_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    scales = np.array([nested.sens_scales(6, 4)[0], oeu_scale - 0.5, oeu_scale])
    kw = dict(nstarts=4, nseed=512, seed=9, run_ids=np.arange(3), on_nonunitary="-inf", **OPTS)
    ref = P.profile_scan(args, asimov, ps, scales, binned=binned, **kw)
    res = R.binned_realisation_scan(args, asimov, ps, scales, binned, measurements=[binned.fr_bins], **kw)
    assert res["nonunitary_seeds"].sum() > 0, "the case needs seeds the reference would have raised on"
    assert np.all(np.isfinite(ref["max_lnl"])) and np.all(ref["nstarts"] == 4)
    assert H.same_bits(res["max_lnl"][0], ref["max_lnl"])
    assert H.same_bits(res["argmax_theta"][0], ref["argmax_theta"])
    for k in ("niter", "nfev", "nstarts"):
        assert np.array_equal(res[k][0], ref[k]), k
    assert np.array_equal(res["nonunitary"][0].astype(np.int64) + res["nonunitary_seeds"], ref["nonunitary"])
    assert res["ts"].shape == (1, 3) and res["ts"][0, 0] == 0.0
    assert H.same_bits(res["ts"][0], -2.0 * (ref["max_lnl"] - ref["max_lnl"][0]))
    assert res["measurements"].shape == (1, 20, 3) and H.same_bits(res["sigmas"], binned.sigma[None])


# ---- 4. the per-run binned measurement ---------------------------------------------------------------------------------------------------
KEYS = ("max_lnl", "ts", "argmax_theta", "nstarts", "nfev", "niter", "nonunitary", "parked", "failed", "limits", "start_cube", "start_score",
        "start_count")


def same(a, b, rows=slice(None), cols=slice(None)):
    for k in KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        x = x[rows] if x.ndim == 1 else x[rows, cols]
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype == np.float64), k


def check_against_standalone(args, scales, res):
    """Every (t, s) of a scan against a maximiser of its own over Model_{s,t} from the same selected seeds; and max_lnl against that
    model's bulk lnprob of argmax_theta."""
    meas, sgs = res["measurements"], res["sigmas"]
    T, S = res["max_lnl"].shape
    cols, models, bases, _ = scale_models(args, scales, BinnedMeasurement(meas[0], sgs[0]))
    try:
        for s in range(S):
            for t in range(T):
                c = int(res["start_count"][t, s])
                assert res["nstarts"][t, s] == c
                if c == 0:                                                   # no seed with a finite value under this realisation: no run
                    assert res["max_lnl"][t, s] == -np.inf and np.isnan(res["argmax_theta"][t, s][cols]).all()
                    assert res["nfev"][t, s] == 0 and res["niter"][t, s] == 0 and not res["failed"][t, s]
                    continue
                models[s].set_binned_measurement(BinnedMeasurement(meas[t], sgs[t]))
                with P.SimplexMaximizer([models[s]], cols, bases[s], nstarts=0, nseed=0, starts=res["start_cube"][t, s, :c][None],
                                        on_nonunitary="-inf", **OPTS) as mx:
                    one = mx.run()
                for k in ("max_lnl", "argmax_theta"):
                    assert H.same_bits(res[k][t, s], one[k][0]), (k, t, s)
                for k in ("niter", "nfev", "nstarts", "nonunitary", "parked"):
                    assert res[k][t, s] == one[k][0], (k, t, s, res[k][t, s], one[k][0])
                assert np.isfinite(res["max_lnl"][t, s])
                assert H.same_bits(models[s].lnprob(res["argmax_theta"][t, s][None], want_status=False), res["max_lnl"][t, s:s + 1]), (t, s)
    finally:
        for m in models:
            m.close()


def test_polish_equals_standalone_models_and_ignores_batch_and_company(oeu_scale):
    args = oeu_args(smearing=0.05)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    scales = np.array([oeu_scale - 0.5, oeu_scale])
    meas = R.draw_binned_realisations(binned, 3, seed=13)
    sig = binned.sigma * np.array([1.0, 0.8, 1.2])[:, None]
    kw = dict(measurements=meas, sigmas=sig, nstarts=4, nseed=512, seed=5, on_nonunitary="-inf", **OPTS)
    res = R.binned_realisation_scan(args, asimov, ps, scales, binned, **kw)
    print("parked %s, non-unitary %s, seeds %s" % (res["parked"].tolist(), res["nonunitary"].tolist(), res["nonunitary_seeds"].tolist()))
    assert res["nonunitary_seeds"].sum() > 0, "the case needs seeds the reference would have raised on"
    assert res["parked"].sum() > 0                                          # candidates were parked and settled under a run's own measurement
    assert res["max_lnl"].shape == (3, 2) and np.all(res["start_count"] == 4)
    assert len(np.unique(res["max_lnl"][:, 1])) == 3                        # the realisations are not copies of each other
    check_against_standalone(args, scales, res)
    same(res, R.binned_realisation_scan(args, asimov, ps, scales, binned, batch=1, **kw))
    one = R.binned_realisation_scan(args, asimov, ps, scales[1:], binned, run_ids=[1], **kw)
    for k in KEYS:
        if k in ("ts", "limits"):                                           # the statistic is against the scan's own null
            continue
        x, y = np.asarray(res[k])[:, 1:2], np.asarray(one[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype == np.float64), k
    per_scale = R.binned_realisation_scan(args, asimov, ps, scales, binned, **dict(kw, measurements=np.stack([meas, meas])))
    same(res, per_scale)


# ---- 5. the start counts ---------------------------------------------------------------------------------------------------------------
def test_fewer_finite_seeds_than_starts(oeu_scale):
    """200 seeds, 8 starts asked for, and realisations with one bin narrowed and placed so that the underflow wall of that bin's term cuts
    through scale 0's compositions there: the runs of one maximiser keep 8 starts, fewer, and none, and each still equals a maximiser of
    its own from exactly those."""
    args = oeu_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    scales = np.array([oeu_scale - 0.5, oeu_scale])
    sm = 0.008
    cols, models, bases, _ = scale_models(args, scales, binned)
    try:
        with R.BinnedToySeeds(models, cols, bases, nseed=200, seed=3) as seeds:
            assert seeds.nonunitary_seeds.sum() > 0, "the case needs seeds the reference would have raised on"
            sd = seeds.seeds(0)
            live = np.isfinite(seeds.scores(binned.fr_bins[None], binned.sigma)[0, 0])      # scale 0's seeds with a value of their own
            b, c, cross = wall_crossings(sd["fr_bins"][live], sm)
            cross = np.sort(cross[np.isfinite(cross)])[::-1]
            # between the crossings of the 5th and 6th seed five stay finite, between the 2nd and 3rd two, far out none
            cand = np.tile(binned.fr_bins[None], (3, 1, 1))
            cand[:, b] = c + np.array([0.5 * (cross[4] + cross[5]), 0.5 * (cross[1] + cross[2]), cross[0] + 2.0])[:, None] * U
            sig = np.tile(binned.sigma[None], (3, 1))
            sig[:, b] = sm
            n = np.sum(seeds.scores(cand, sig)[0] > -np.inf, axis=1)          # finite seeds of scale 0 under every candidate
    finally:
        for m in models:
            m.close()
    some, few = 0, 1
    assert 4 <= n[some] <= 7 and 1 <= n[few] <= 3 and n[-1] == 0, n.tolist()          # a condition on the inputs
    meas = np.stack([binned.fr_bins, cand[some], cand[few], cand[-1]])
    sigs = np.stack([binned.sigma, sig[some], sig[few], sig[-1]])
    res = R.binned_realisation_scan(args, asimov, ps, scales, binned, measurements=meas, sigmas=sigs, nstarts=8, nseed=200, seed=3,
                                    on_nonunitary="-inf", **OPTS)
    counts = res["start_count"]
    print("starts kept per (realisation, scale): %s" % counts.tolist())
    assert np.array_equal(res["nstarts"], counts)
    assert counts[0, 0] == 8 and counts[1, 0] == n[some] and counts[2, 0] == n[few] and counts[3, 0] == 0
    assert res["max_lnl"][3, 0] == -np.inf and np.isnan(res["argmax_theta"][3, 0][cols]).all() and np.isnan(res["ts"][3, 0])
    check_against_standalone(args, scales, res)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(oeu_scale):
    args = oeu_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = own_measurement(args, asimov)
    scales = np.array([oeu_scale - 0.5, oeu_scale])
    nb = binned.nbins
    fb = np.tile(binned.fr_bins[None], (2, 1, 1))
    # a flux-averaged set
    cols, models, bases, _ = scale_models(args, scales, None)
    starts = np.full((2, 1, len(cols)), 0.5)
    try:
        with pytest.raises(_lib.GolemHipError, match="no binned measurement"):
            R.BinnedToySeeds(models, cols, bases, nseed=64)
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts) as mx:
            with pytest.raises(_lib.GolemHipError, match="no binned measurement"):
                mx.set_binned_measurements(fb, binned.sigma)
        # a set of which one model has another number of energy bins, or another likelihood offset
        models[0].set_binned_measurement(binned)
        sp = nested._scale_paramset(ps, float(scales[1]))
        args3 = oeu_args(3)
        with Model(sens_desc(args3, sp, model_bf(asimov), 0.1)) as other:
            other.set_binned_measurement(own_measurement(args3, asimov))
            with pytest.raises(_lib.GolemHipError, match="energy bins"):
                R.BinnedToySeeds([models[0], other], cols, bases, nseed=64)
        with Model(compile_model(sp, "BSM_GAUSS", bestfit_fr=model_bf(asimov), smearing=0.1, source_ratio=args.source_ratio, texture=args.texture,
                                 dimension=args.dimension, binning=args.binning, offset=-300.0)) as other:
            other.set_binned_measurement(binned)
            with pytest.raises(_lib.GolemHipError, match="offset"):
                R.BinnedToySeeds([models[0], other], cols, bases, nseed=64)
    finally:
        for m in models:
            m.close()
    cols, models, bases, _ = scale_models(args, scales, binned)
    try:
        # nseed > 0: the set's own seeding would score under the models' measurement
        with P.SimplexMaximizer(models, cols, bases, nstarts=2, nseed=64) as mx:
            with pytest.raises(_lib.GolemHipError, match="seed points"):
                mx.set_binned_measurements(fb, binned.sigma)
        with P.SimplexMaximizer(models, cols, bases, nstarts=0, nseed=0, starts=starts, maxiter=5, restarts=0, on_nonunitary="-inf") as mx:
            with pytest.raises(_lib.GolemHipError, match="bins given"):
                mx.set_binned_measurements(fb[:, :nb - 1], binned.sigma[:nb - 1])
            bad = fb.copy()
            bad[1, 3, 2] = np.nan
            with pytest.raises(_lib.GolemHipError, match="finite composition"):
                mx.set_binned_measurements(bad, binned.sigma)
            for w in (0.0, -0.1, np.inf, np.nan):
                sg = np.tile(binned.sigma[None], (2, 1))
                sg[1, 2] = w
                with pytest.raises(_lib.GolemHipError, match="width > 0"):
                    mx.set_binned_measurements(fb, sg)
            sg = np.tile(binned.sigma[None], (2, 1))
            sg[0, 1] = 1e-200                                             # its square underflows: the constants are not finite
            with pytest.raises(_lib.GolemHipError, match="outside the range"):
                mx.set_binned_measurements(fb, sg)
            mx.set_binned_measurements(fb, binned.sigma)                  # accepted, and again before the first run
            mx.set_binned_measurements(fb, 1.5 * binned.sigma)
            mx.run()
            with pytest.raises(_lib.GolemHipError, match="before the first run"):
                mx.set_binned_measurements(fb, binned.sigma)
        with R.BinnedToySeeds(models, cols, bases, nseed=64, seed=1) as seeds:
            assert seeds.nonunitary_seeds.sum() > 0, "the case needs seeds the reference would have raised on"
            for K in (0, 17):
                with pytest.raises(_lib.GolemHipError, match="1 to 16"):
                    seeds.select(fb, binned.sigma, K)
            sg = np.tile(binned.sigma[None], (2, 1))
            sg[1, 0] = 0.0
            with pytest.raises(_lib.GolemHipError, match="width > 0"):
                seeds.select(fb, sg, 4)
            with pytest.raises(ValueError, match="measurements must be"):
                seeds.select(fb[:, :3], binned.sigma, 4)
            assert seeds.select(fb, binned.sigma, 16)["count"].shape == (2, 2)
        lp, frb, status, meas, sigma, off = H.crafted(40, 3, 4, seed=1)
        with pytest.raises(_lib.GolemHipError, match="1 to 16"):
            R.toy_select_binned(lp, frb, status, meas, sigma, off, 17)
        with pytest.raises(ValueError, match="1 to 16"):
            R.binned_realisation_scan(args, asimov, ps, scales, binned, ntoys=2, nstarts=17)
        # the flux-averaged entry points keep refusing a binned set
        with pytest.raises(_lib.GolemHipError, match="binned measurement"):
            R.ToySeeds(models, cols, bases, nseed=64)
        with pytest.raises(ValueError, match="energy-resolved"):
            R.realisation_scan(args, asimov, ps, scales, ntoys=2, binned=binned)
    finally:
        for m in models:
            m.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------------------
def test_sens_cli_binned_realisations_end_to_end(tmp_path):
    base = [sys.executable, "-m", "golemflavor_amd.sens", "--stat-method", "frequentist", "--energy-resolved", "--segments", "4", "--smearing", "0.1",
            "--pl-starts", "4", "--pl-seed-points", "512", "--seed", "3"]
    lines = []
    for sub, more in (("toys", ["--realisations", "3", "--realisation-starts", "4", "--realisation-seed", "2"]), ("plain", [])):
        out = subprocess.run(base + more + ["--datadir", str(tmp_path / sub)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads(out.stdout.strip().splitlines()[-1]))
    line, plain = lines
    toys = line["realisations"]
    assert line["likelihood"] == "energy-resolved" and "realisations" not in plain
    assert os.path.dirname(toys["file"]) == os.path.dirname(line["fr_maxllh"])
    assert os.path.basename(toys["file"]).startswith("fr_realisations") and toys["file"].endswith("_ebins.npz")
    z = np.load(toys["file"])
    scales = nested.sens_scales(6, 4)
    asimov, _ = Cf.sens_paramsets(6, (1., 1., 1.))
    binned = BinnedMeasurement.constant(model_bf(asimov), 0.1, Cf.default_bin_edges())
    assert np.array_equal(z["scales"], scales) and z["measurements"].shape == (3, 20, 3) and np.array_equal(z["smearings"], np.tile(binned.sigma, (3, 1)))
    assert np.array_equal(z["measurements"], R.draw_binned_realisations(binned, 3, seed=2))
    for k in ("max_lnl", "ts", "nstarts", "nfev", "niter", "nonunitary", "failed"):
        assert z[k].shape == (3, 4), k
    assert z["argmax_theta"].shape[:2] == (3, 4) and z["limits"].shape == (3,) and z["nonunitary_seeds"].shape == (4,)
    assert np.all(z["ts"][:, 0] == 0.0) and np.all(np.isfinite(z["max_lnl"])) and np.all(z["nstarts"] == 4)
    assert toys["band_quantiles"] == [2.5, 16., 50., 84., 97.5] and len(toys["band_limits"]) == 5
    assert toys["n"] == 3 and toys["without_limit"] == int(np.isnan(z["limits"]).sum()) and len(toys["ts_q95"]) == 4
    band = R.sensitivity_band(z["limits"])
    assert np.array_equal(np.asarray(toys["band_limits"], dtype=float), band["limits"], equal_nan=True)
    # the Asimov arrays are byte for byte what the command writes without --realisations
    for key in ("fr_maxllh", "fr_stat"):
        assert os.path.basename(line[key]).endswith("_ebins.npy")
        assert open(line[key], "rb").read() == open(plain[key], "rb").read(), key
    assert line["max_lnl"] == plain["max_lnl"]
