"""Every stored chain reweighted to other targets on the device: the log-weights against the host's subtraction, the
weight pipeline against the host build of csrc/gf_nested_post.hpp, the measurement path against the model path, non-unitary rows,
the reductions, and one end-to-end check against a chain sampled at the target."""
import json
import os

import numpy as np
import pytest

import nested_post_harness as H
from common import BIN_EDGES, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import contour
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import intervals as iv
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import scan
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model
from golemflavor_amd.reweight import Measurement, lnw_host

pytestmark = pytest.mark.gpu

NW, SEED, IDS = 64, 8, [5, 0, 9]
U = 2.0 ** -53
BF = [(0.30, 0.36, 0.34), (0.36, 0.33, 0.31), (0.32, 0.30, 0.38)]
SM = 0.05                    # no point of the simplex is in the subnormal band: |fr - bf|^2 <= 2, see in_band_possible


def patched(desc, bestfit_fr=None, smearing=None, lo=None, hi=None):
    d = type(desc).from_buffer_copy(desc)
    if bestfit_fr is not None:
        for k in range(3):
            d.bestfit_fr[k] = float(bestfit_fr[k])
    if smearing is not None:
        d.smearing = float(smearing)
    for c, v in (lo or {}).items():
        d.lo[c] = float(v)
    for c, v in (hi or {}).items():
        d.hi[c] = float(v)
    return d


def gauss_consts(smearing):
    """gf_model_create's constants of multi_gaussian: (mh, k) with logpdf = mh |fr - bf|^2 + k"""
    s = smearing ** 2
    return -0.5 / s, -0.5 * (3.0 * np.log(2.0 * np.pi) + 3.0 * np.log(s))


def in_band_possible(smearing):
    """fr and bf are compositions (components in [0, 1], sum 1), so |fr - bf|^2 <= 2: the smallest logpdf any row can have"""
    mh, k = gauss_consts(smearing)
    return k + 2.0 * mh < -708.3


def stored(s):
    """(rows (nchains, n, ndim), lnprob (nchains, n)) in the device's storage order"""
    c, lp, _ = s._fetch(chain=True, lnprob=True)
    return c.reshape(s.nchains, -1, s.dim), lp.reshape(s.nchains, -1)


def notebook():
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    return Cf.notebook_paramsets(ang)


@pytest.fixture(scope="module")
def sm3():
    """three stacked 6-dim SM_GAUSS chains with different best fits, 64 walkers, 65 stored steps: n = 4160, one step past the leaf"""
    asimov, ps = notebook()
    ms = [Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=SM)) for bf in BF]
    np.random.seed(4)
    s = mcmc_utils.DeviceEnsembleSampler(NW, 6, ms, seed=SEED, stream_ids=IDS)
    p0 = np.stack([mcmc_utils.flat_seed(ps, NW) for _ in range(3)])
    s.run_mcmc(p0, 30, storechain=False)
    s.run_mcmc(None, 65)
    rows, lp = stored(s)
    assert rows.shape == (3, 4160, 6)
    yield s, ms, ps, rows, lp
    s.close()
    for m in ms:
        m.close()


def check_pipeline(r, rows, seed, sids, N, what):
    """ess, mean, cov, index and rows of every (chain, target) against the host build on the device's lnw"""
    nch, T = r.nchains, r.ntargets
    sm = r._summary
    got_rows, got_index = r.rows(N, return_index=True)
    got_rows, got_index = got_rows.reshape(nch, T, N, -1), got_index.reshape(nch, T, N)
    empty = 0
    for c in range(nch):
        lnw = r.lnw(c)
        for t in range(T):
            tag = "%s chain %d target %d N %d" % (what, c, t, N)
            if not np.any(lnw[t] > -np.inf):
                empty += 1
                assert sm["ess"][c, t] == 0.0 and np.isnan(sm["lnz_ratio"][c, t]), tag
                assert np.isnan(sm["mean"][c, t]).all() and np.isnan(sm["cov"][c, t]).all(), tag
                assert np.isnan(got_rows[c, t]).all() and (got_index[c, t] == -1).all(), tag
                continue
            hp = H.host_posterior(lnw[t], rows[c])
            assert H.same_bits(sm["ess"][c, t], hp["ess"]), tag
            assert H.same_bits(sm["mean"][c, t], hp["mean"]) and H.same_bits(sm["cov"][c, t], hp["cov"]), tag
            assert sm["lnz_ratio"][c, t] == hp["m"] + np.log(hp["S"]) - np.log(float(len(lnw[t]))), tag
            idx = H.host_resample(hp["C"], N, H.host_offset(seed, sids[c] * 64 + t))
            assert np.array_equal(got_index[c, t], idx), tag
            assert H.same_bits(got_rows[c, t], rows[c][idx]), tag
    return empty


# ---- 1. the model path, bits -------------------------------------------------------------------------------------------------------
def test_model_path_lnw_bits(sm3):
    s, ms, ps, rows, lp = sm3
    targets, models = [], []
    for c in range(3):
        d = ms[c].desc
        cut = float(np.median(rows[c][:, 4]))
        tg = [Model(patched(d, bestfit_fr=BF[(c + 1) % 3])), Model(patched(d, smearing=0.08)), Model(patched(d, hi={4: cut}))]
        keep = float(np.mean(rows[c][:, 4] <= cut))
        assert 0.05 < keep < 0.95, keep                                # the narrow box keeps a real part of the rows
        targets.append(tg)
        models += tg
    try:
        r = s.reweight(targets)
        sm = r.summary()
        assert sm["ess"].shape == (3, 3) and sm["mean"].shape == (3, 3, 6) and sm["cov"].shape == (3, 3, 6, 6)
        assert np.array_equal(sm["n"], [4160] * 3) and np.array_equal(sm["bad_base"], [0] * 3) and not sm["nonunitary"].any()
        for c in range(3):
            lnw = r.lnw(c)
            assert lnw.shape == (3, 4160)
            for t in range(3):
                lt, st = targets[c][t].lnprob(rows[c])
                want, kind = lnw_host(lt, lp[c], st)
                assert H.same_bits(lnw[t], want), (c, t)
                fin = np.isfinite(lt)
                assert H.same_bits(lnw[t][fin], np.subtract(lt[fin], lp[c][fin])) and np.isneginf(lnw[t][~fin]).all()
                assert sm["outside"][c, t] == int((~fin).sum()) == int((kind == 3).sum()), (c, t)
            assert sm["outside"][c, 0] == 0 and sm["outside"][c, 1] == 0 and 0 < sm["outside"][c, 2] < 4160
        assert check_pipeline(r, rows, SEED, IDS, 65, "model path") == 0
    finally:
        for m in models:
            m.close()


def few_cut(x):
    """(column, upper edge) of a box that keeps between 1 and 9 rows (the stretch move repeats rows: count, do not index)"""
    for c in range(x.shape[1] - 1, -1, -1):
        u, cnt = np.unique(x[:, c], return_counts=True)
        k = int(np.searchsorted(np.cumsum(cnt), 9, side="right")) - 1
        if k >= 0 and k + 1 < len(u):
            return c, float(0.5 * (u[k] + u[k + 1]))
    raise AssertionError("no column splits off fewer than 10 rows")


# ---- 2. the pipeline, bits ------------------------------------------------------------------------------------------------------
def test_pipeline_bits_at_every_size(monkeypatch):
    """Stored steps 1, 64, 65, 129 (n = 64, 4096, 4160, 8256) x N in {1, 64, 65, 4097}: ess, mean, cov, index and rows equal the host
    build.  Targets: another best fit, a box that excludes every row, a box that keeps fewer than 10 rows.  The same targets alone and
    in another order give the same lnw, ess, mean and cov bits and the rows of the host build at the id of their new place (the
    resampling offset is keyed by the target's place in the call, stream_id * 64 + t); one target per batch under a small
    GF_REWEIGHT_SCRATCH_BYTES changes no bit of anything."""
    asimov, ps = notebook()
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=BF[0], smearing=SM))
    np.random.seed(11)
    s = mcmc_utils.DeviceEnsembleSampler(NW, 6, m, seed=SEED, stream_ids=[3])
    s.run_mcmc(mcmc_utils.flat_seed(ps, NW), 30, storechain=False)
    open_models = []
    try:
        for add, total in ((1, 1), (63, 64), (1, 65), (64, 129)):
            s.run_mcmc(None, add)
            assert s.nstored == total
            rows, lp = stored(s)
            fcol, few = few_cut(rows[0])
            tg = [Model(patched(m.desc, bestfit_fr=BF[1])), Model(patched(m.desc, lo={4: 0.0}, hi={4: 1e-300})),
                  Model(patched(m.desc, hi={fcol: few}))]
            open_models += tg
            r = s.reweight(tg, seed=77)
            sm = r.summary()
            assert sm["ess"].shape == (3,) and sm["n"] == NW * total
            assert sm["outside"][1] == NW * total and 0 < NW * total - sm["outside"][2] < 10
            for N in (1, 64, 65, 4097):
                assert check_pipeline(r, rows, 77, [3], N, "steps %d" % total) == 1
            if total < 65:
                continue
            base_lnw, base_rows = r.lnw(0), r.rows(65, return_index=True)
            for order in ([0], [1], [2], [2, 1, 0]):
                q = s.reweight([tg[t] for t in order], seed=77)
                qs = q.summary()
                for k, t in enumerate(order):
                    assert H.same_bits(q.lnw(0)[k], base_lnw[t])
                    for f in ("ess", "lnz_ratio", "mean", "cov", "outside"):
                        assert H.same_bits(np.asarray(qs[f][k], dtype=np.float64), np.asarray(sm[f][t], dtype=np.float64)), (order, f)
                check_pipeline(q, rows, 77, [3], 65, "order %r" % (order,))
            meas = [Measurement(bestfit_fr=BF[1]), Measurement(bestfit_fr=BF[2], smearing=0.08), Measurement(bestfit_fr=(1., 0., 0.), smearing=1e-3),
                    Measurement(bestfit_fr=BF[0], smearing=0.065)]
            rm = s.reweight(meas, seed=77)
            meas_lnw, meas_rows, meas_sum = rm.lnw(0), rm.rows(65, with_fr=True, return_index=True), rm.summary()
            assert meas_sum["outside"][2] == NW * total                          # the third excludes every row
            # the variable is read on every call: it stays set over everything that is compared
            for cap in ("1", str(2 * 24 * NW * total)):                          # one target per batch; two, then the rest
                monkeypatch.setenv("GF_REWEIGHT_SCRATCH_BYTES", cap)
                q = s.reweight(tg, seed=77)
                assert H.same_bits(q.lnw(0), base_lnw), cap
                for f, v in q.summary().items():
                    assert H.same_bits(np.asarray(v, dtype=np.float64), np.asarray(sm[f], dtype=np.float64)), (cap, f)
                q_rows = q.rows(65, return_index=True)
                assert H.same_bits(q_rows[0], base_rows[0]) and np.array_equal(q_rows[1], base_rows[1]), cap
                qm = s.reweight(meas, seed=77)                                   # the measurement path's batches
                assert H.same_bits(qm.lnw(0), meas_lnw), cap
                for f, v in qm.summary().items():
                    assert H.same_bits(np.asarray(v, dtype=np.float64), np.asarray(meas_sum[f], dtype=np.float64)), (cap, f)
                qm_rows = qm.rows(65, with_fr=True, return_index=True)
                assert H.same_bits(qm_rows[0], meas_rows[0]) and np.array_equal(qm_rows[1], meas_rows[1]), cap
                monkeypatch.delenv("GF_REWEIGHT_SCRATCH_BYTES")
    finally:
        s.close()
        m.close()
        for x in open_models:
            x.close()


# ---- 3. the measurement path against the model path --------------------------------------------------------------------------------
# |lnw_model - lnw_measurement| <= K 2^-53 max(|l_t|, |l0|) per row, K = 6: the model path rounds l_t = lp + mg_t and
# l0 = lp + mg_0 once each (the measurement path never forms them), and both paths round their final difference, |lnw| <= |l_t| + |l0|
# <= 2 max: 2 + 2 * 2 = 6.  That holds for identical mg in the two paths: the same operations on the same constants, and the same
# composition -- compare_paths asserts first that the lnprob kernel's composition of every row is the propagate kernel's bit for bit.
K_PATHS = 6.0


def compare_paths(s, descs, specs, rows, lp, what):
    """specs: [chain][target] (bestfit_fr, smearing).  Returns the largest deviation in units of 2^-53 max(|l_t|, |l0|)."""
    nch = s.nchains
    meas = [[Measurement(bestfit_fr=bf, smearing=sm) for bf, sm in specs[c]] for c in range(nch)]
    models = [[Model(patched(descs[c], bestfit_fr=bf, smearing=sm)) for bf, sm in specs[c]] for c in range(nch)]
    worst = 0.0
    try:
        a, b = s.reweight(meas, on_nonunitary="-inf"), s.reweight(models, on_nonunitary="-inf")
        for f in ("nonunitary", "outside", "bad_base"):
            assert np.array_equal(a.summary()[f], b.summary()[f]), f
        for c in range(nch):
            la, lb = a.lnw(c), b.lnw(c)
            for t, (bf, sm) in enumerate(specs[c]):
                assert not in_band_possible(sm) and not in_band_possible(descs[c].smearing)      # no row in the subnormal band
                lt, fr_l, st_l = models[c][t].lnprob(rows[c], want_fr=True, want_status=True)
                fr_p, st_p = models[c][t].propagate(rows[c])
                ok = (st_l == _lib.GF_ST_OK) & (st_p == _lib.GF_ST_OK)
                assert np.array_equal(st_l, st_p) and ok.mean() > 0.99 and H.same_bits(fr_l[ok], fr_p[ok]), (what, c, t)   # what K = 6 rests on
                assert np.array_equal(np.isneginf(la[t]), np.isneginf(lb[t])), (what, c, t)      # the same rows carry no weight
                fin = np.isfinite(la[t])
                assert fin.mean() > 0.99
                scale = np.maximum(np.abs(lt[fin]), np.abs(lp[c][fin]))
                dev = np.abs(la[t][fin] - lb[t][fin]) / (U * scale)
                print("%s chain %d target %d: largest deviation %.3f x 2^-53 max(|l_t|, |l0|), bound %.0f" % (what, c, t, dev.max(), K_PATHS))
                assert np.all(dev <= K_PATHS), (what, c, t, dev.max())
                worst = max(worst, float(dev.max()))
        # with_fr: the compositions are postprocess's of the same rows, gathered by index
        ra, ia = a.rows(65, with_fr=True, return_index=True)
        rb, ib = b.rows(65, with_fr=True, return_index=True)
        T = len(specs[0])
        ra, rb = ra.reshape(nch, T, 65, -1), rb.reshape(nch, T, 65, -1)
        ia, ib = ia.reshape(nch, T, 65), ib.reshape(nch, T, 65)
        own = s.postprocess(want_fr=True, step_major=True)["fr"].reshape(nch, -1, 3)
        for c in range(nch):
            for t in range(T):
                assert (ia[c, t] >= 0).all() and H.same_bits(ra[c, t][:, :3], own[c][ia[c, t]]) and H.same_bits(ra[c, t][:, 3:], rows[c][ia[c, t]])
        under = s.postprocess(want_fr=True, step_major=True, models=[models[c][0] for c in range(nch)])["fr"].reshape(nch, -1, 3)
        for c in range(nch):
            assert H.same_bits(rb[c, 0][:, :3], under[c][ib[c, 0]]) and H.same_bits(rb[c, 0][:, 3:], rows[c][ib[c, 0]])
    finally:
        for p in models:
            for m in p:
                m.close()
    return worst


def test_measurement_path_against_model_path_sm(sm3, oracle):
    s, ms, ps, rows, lp = sm3
    specs = [[(BF[(c + 1) % 3], SM), (BF[c], 0.08), (BF[(c + 2) % 3], 0.065)] for c in range(3)]
    # the band, by the oracle alone: its composition of every row, then logpdf = mg - offset under every target
    for c in range(3):
        om = oracle.make_model(ps, "SM_GAUSS", bestfit_fr=BF[c], smearing=SM)
        _, ofr = oracle.lnprob_batch(om, rows[c], want_fr=True)
        for bf, sm in specs[c] + [(BF[c], SM)]:
            mh, k = gauss_consts(sm)
            logpdf = mh * ((ofr - np.asarray(bf)) ** 2).sum(axis=1) + k
            assert np.mean(logpdf < -708.3) <= 0.01
    worst = compare_paths(s, [m.desc for m in ms], specs, rows, lp, "SM")
    print("SM: largest deviation %.3f" % worst)


def test_measurement_path_against_model_path_bsm():
    pts = scan.sens_grid()[:2]
    jobs = [scan._SensPoint(p, g, nwalkers=32, device=0, smearing=SM) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(32, 12, [j.f for j in jobs], seed=25, stream_ids=[0, 1])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 40)
        rows, lp = stored(s)
        assert rows.shape == (2, 1280, 12)
        specs = [[(BF[0], SM), (BF[1], 0.08)], [(BF[2], 0.065), (BF[0], SM)]]
        worst = compare_paths(s, [j.f.model.desc for j in jobs], specs, rows, lp, "BSM")
        print("BSM: largest deviation %.3f" % worst)
    finally:
        s.close()
        for j in jobs:
            j.close()


# ---- 4. non-unitary rows ---------------------------------------------------------------------------------------------------------
def test_nonunitary_rows():
    """A prior-only 7-column chain with logLam over [-37, -34], the range in which dimension 6, OEU passes and fails with all 20
    default bins; the target is the BSM_GAUSS model."""
    ps7 = Cf.texture_paramset(6)
    prior = Model(patched(compile_model(ps7, "PRIOR_ONLY", flat_llh=1.0), lo={6: -37.0}, hi={6: -34.0}))
    bsm = Model(compile_model(ps7, "BSM_GAUSS", texture=Texture.OEU, dimension=6, binning=BIN_EDGES, source_ratio=(1., 2., 0.),
                              bestfit_fr=(1 / 3, 1 / 3, 1 / 3), smearing=SM))
    rng = np.random.default_rng(12)
    p0 = uniform_theta(ps7, NW, rng, seeds=True)
    p0[:, 6] = rng.uniform(-37.0, -34.0, NW)
    s = mcmc_utils.DeviceEnsembleSampler(NW, 7, prior, seed=5)
    try:
        s.run_mcmc(p0, 65)
        rows, lp = stored(s)
        lt, st = bsm.lnprob(rows[0], want_status=True)
        bad = st == _lib.GF_ST_NON_UNITARY
        assert 0.10 <= bad.mean() <= 0.90, bad.mean()
        with pytest.raises(AssertionError, match="Matrix is not unitary!"):
            s.reweight([bsm])
        r = s.reweight([bsm], on_nonunitary="-inf")
        sm = r.summary()
        assert sm["nonunitary"][0] == int(bad.sum()) and sm["bad_base"] == 0
        lnw = r.lnw(0)[0]
        assert np.isneginf(lnw[bad]).all()
        keep = ~bad & np.isfinite(lt)
        assert np.array_equal(np.isneginf(lnw), ~keep) and H.same_bits(lnw[keep], np.subtract(lt[keep], lp[0][keep]))
        assert sm["outside"][0] == int((~bad & ~np.isfinite(lt)).sum())
        _, idx = r.rows(257, return_index=True)
        assert not bad[idx[0]].any()                                   # a row of zero weight is never taken
        with pytest.raises(_lib.GolemHipError):
            s.reweight([Measurement(bestfit_fr=BF[0], smearing=SM)])   # the chain was not sampled under a measurement
    finally:
        s.close()
        prior.close()
        bsm.close()


# ---- 5. the reductions -----------------------------------------------------------------------------------------------------------
def test_reductions_equal_the_host_row_entry_points(sm3):
    s, ms, ps, rows, lp = sm3
    N, pct = 1000, (68., 90.)
    r = s.reweight([Measurement(bestfit_fr=BF[1], smearing=SM), Measurement(bestfit_fr=(1., 0., 0.), smearing=1e-3)])
    assert np.array_equal(r.summary()["outside"][:, 1], [4160] * 3)    # the second target excludes every row: no posterior
    for with_fr in (False, True):
        x = r.rows(N, with_fr=with_fr)
        width = x.shape[-1]
        ranges = ([(0., 1.)] * 3 if with_fr else []) + [(ms[0].desc.lo[c], ms[0].desc.hi[c]) for c in range(6)]
        got_m = r.marginals(N, with_fr=with_fr, percentiles=(5., 50., 95.))
        got_i = r.intervals(N, percentiles=pct, with_fr=with_fr)
        for c in range(3):
            for t in range(2):
                want = mg.chain_marginals(x[c, t], ranges, model=ms[0], names=got_m[c][t].names, percentiles=(5., 50., 95.))
                a, b = got_m[c][t].as_arrays(), want.as_arrays()
                assert sorted(a) == sorted(b)
                for k in a:
                    assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (with_fr, c, t, k)
                wi = iv.chain_intervals(x[c, t], model=ms[0], percentiles=pct)
                for f in iv.FIELDS:
                    assert np.ascontiguousarray(got_i[f][c, t]).tobytes() == np.ascontiguousarray(wi[f]).tobytes(), (with_fr, c, t, f)
        assert width == (9 if with_fr else 6)
    x = r.rows(N, with_fr=True)
    got = r.regions(N, 25, (68., 90.), oversample=2.)
    for c in range(3):
        for t in range(2):
            want = contour.flavor_region(x[c, t][:, :3], 25, (68., 90.), 0.05, 2., model=ms[0])
            for g, w in zip(got[c][t], want):
                for f in ("thres", "saturated", "level_in", "level_out", "mass"):
                    assert np.array_equal(getattr(g, f), getattr(w, f), equal_nan=True), (c, t, f)
                assert np.array_equal(g.cells, w.cells) and np.array_equal(g.density, w.density)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
def test_reweighted_mean_agrees_with_a_chain_sampled_at_the_target():
    """2-dim tutorial model, a chain sampled at best fit A reweighted to B about one smearing width away, against a chain sampled at
    B.  Standard errors: var / n_eff with n_eff = the chain's ESS (diagnostics) for B, and Kish's ESS scaled by the chain's ESS / n
    for the reweighted A."""
    sm = 0.05
    fa = np.array([1., 2., 0.]) / 3.
    fb = fa + np.array([0.035, -0.035, 0.0])
    out = {}
    for tag, f in (("a", fa), ("b", fb)):
        asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles(f), smearing=sm)
        fn = llh_utils.tutorial_ln_prob(asimov, ps)
        np.random.seed(21)
        s = mcmc_utils.DeviceEnsembleSampler(NW, 2, fn, seed=31 if tag == "a" else 32)
        s.run_mcmc(mcmc_utils.flat_seed(ps, NW), 300, storechain=False)
        s.run_mcmc(None, 2000)
        out[tag] = (s, fn)
    try:
        sa, sb = out["a"][0], out["b"][0]
        n = NW * 2000
        bf_b = np.array([out["b"][1].model.desc.bestfit_fr[k] for k in range(3)])
        r = sa.reweight([Measurement(bestfit_fr=bf_b, smearing=sm)])
        q = r.summary()
        assert q["ess"][0] > 1000, q["ess"]
        ess_a, ess_b = np.asarray(sa.diagnostics().ess), np.asarray(sb.diagnostics().ess)
        xb = sb.flat_steps()
        mean_b, var_b = xb.mean(axis=0), xb.var(axis=0, ddof=1)
        var_rw = np.diag(q["cov"][0])
        se = np.sqrt(var_rw / (q["ess"][0] * ess_a / n) + var_b / ess_b)
        z = (q["mean"][0] - mean_b) / se
        print("reweighted %r, sampled %r, z %r, Kish ESS %.0f, chain ESS %r / %r" % (q["mean"][0], mean_b, z, q["ess"][0], ess_a, ess_b))
        assert np.all(np.abs(z) < 5.0), z
        z0 = (sa.flat_steps().mean(axis=0) - mean_b) / se
        assert np.any(np.abs(z0) > 5.0), z0                            # without the weights the chains differ: the check has power
    finally:
        for s, fn in out.values():
            s.close()
            fn.close()


# ---- the scan ---------------------------------------------------------------------------------------------------------------------
def test_scan_writes_reweight_files_for_a_c5_shaped_run(tmp_path, capsys):
    d = str(tmp_path / "c5")
    scan.main(["--config", "C5", "--points", "3", "--nwalkers", "64", "--burnin", "5", "--nsteps", "30", "--datadir", d,
               "--reweight-injected", "0.30", "0.36", "0.34", "1", "1", "1", "--reweight-smearing", "0.05", "0.02", "--reweight-rows", "500"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["reweight"]["points"] == 3 and line["reweight"]["targets"] == 4 and line["reweight"]["rows"] == 500
    chains = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert len(chains) == 3
    want = chains + ["reweight_%s.npz" % f[:-4] for f in chains] + ["reweight_marginals_%s_t%d.npz" % (f[:-4], t) for f in chains for t in range(4)]
    assert sorted(os.listdir(d)) == sorted(want)
    for f in chains:
        with np.load(os.path.join(d, "reweight_%s.npz" % f[:-4])) as z:
            assert z["ess"].shape == (4,) and z["mean"].shape == (4, 12) and z["cov"].shape == (4, 12, 12) and int(z["n"]) == 64 * 30
            assert np.allclose(z["target_bestfit_fr"], [[0.30, 0.36, 0.34]] * 2 + [[1 / 3] * 3] * 2)
            assert np.array_equal(z["target_smearing"], [0.05, 0.02, 0.05, 0.02]) and np.array_equal(z["target_offset"], [-320.0] * 4)
            # the scan's own measurement ((1, 1, 1) / 3 to the rounding of its angles, smearing 0.02) is the last target: lnw ~ 0 on every
            # kept row, so ESS = the kept rows and lnz_ratio = log(kept / n) to rounding
            kept = int(z["n"]) - int(z["outside"][3]) - int(z["nonunitary"][3]) - int(z["bad_base"])
            assert kept > 0 and np.isclose(z["ess"][3], kept, rtol=1e-9, atol=0) and np.isclose(z["lnz_ratio"][3], np.log(kept / float(z["n"])), atol=1e-9)
