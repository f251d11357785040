"""The posterior of the nested sampler's runs on the GPU (gf_nested_post.hip through golemflavor_amd.nested): the gathered points
and every number bit for bit against the host build of gf_nested_post.hpp fed with dead()'s arrays, independence of the runs, the
reuse of the marginal, element and region reductions, the posterior mean against quadrature, a sens-shaped case, the driver, and
runs without a posterior."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import nested_post_harness as H
import test_gpu_nested as TN
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import contour, elements
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import nested
from golemflavor_amd.enums import Texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SEED, IDS, SMEAR = 3, [5, 6, 7], [0.05, 0.08, 0.12]
KW = dict(nlive=100, batch=12, walks=10, seed=SEED)
NROWS = 1000          # no multiple of 64 or 256


def _tutorial(smearing):
    asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=smearing)
    return llh_utils.tutorial_ln_prob(asimov, ps)


@pytest.fixture(scope="module")
def three():
    """three tutorial runs of different smearing (so that their iteration counts differ), run once; closed at the end"""
    fs = [_tutorial(sm) for sm in SMEAR]
    s = nested.NestedSampler(fs, [0, 1], np.zeros(2), run_ids=IDS, **KW)
    res = s.run()
    yield s, fs, res
    s.close()
    for f in fs:
        f.close()


def _bits(a, b):
    return H.same_bits(a, b)


def test_rows_and_posterior_equal_host_program_on_dead_points(three):
    s, fs, res = three
    assert len(set(res["niter"].tolist())) == 3
    post = s.posterior()
    for N in (NROWS, 65):
        rows, index = s.posterior_rows(N, return_index=True)
        assert rows.shape == (3, N, 2) and index.shape == (3, N)
        for r in range(3):
            d = s.dead(r)
            n = len(d["lnw"])
            assert n % 64 and n % 12 and post["npoints"][r] == n == res["niter"][r] * 12 + 100
            assert _bits(rows[r], d["theta"][index[r]]), (N, r)                    # the gather, the cube map and the row build
            h = H.host_posterior(d["lnw"], d["theta"], [0, 0])
            assert np.array_equal(index[r], H.host_resample(h["C"], N, H.host_offset(SEED, IDS[r]))), (N, r)
            if N == NROWS:
                assert _bits(post["ess"][r], h["ess"]) and _bits(post["mean"][r], h["mean"]) and _bits(post["cov"][r], h["cov"]), r
                assert post["lnz_check"][r] == h["m"] + math.log(h["S"])
                assert abs(post["lnz_check"][r] - res["lnz"][r]) < 1e-9 * max(1.0, abs(res["lnz"][r]))
                assert 1.0 < post["ess"][r] < n


def test_runs_are_independent_and_calls_repeatable(three):
    s, fs, res = three
    rows, index = s.posterior_rows(NROWS, return_index=True)
    post = s.posterior()
    before, dead_before = s.result(), s.dead(1)
    rows2, index2 = s.posterior_rows(NROWS, return_index=True)
    post2 = s.posterior()
    assert _bits(rows, rows2) and np.array_equal(index, index2)
    for k in post:
        assert _bits(post[k].astype(np.float64), post2[k].astype(np.float64)), k
    after, dead_after = s.result(), s.dead(1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    for k in dead_before:
        assert np.array_equal(dead_before[k], dead_after[k]), k
    with nested.NestedSampler([fs[1]], [0, 1], np.zeros(2), run_ids=[IDS[1]], **KW) as alone:
        ra = alone.run()
        assert ra["lnz"][0] == res["lnz"][1] and ra["niter"][0] == res["niter"][1]
        arows, aindex = alone.posterior_rows(NROWS, return_index=True)
        apost = alone.posterior()
    assert _bits(arows[0], rows[1]) and np.array_equal(aindex[0], index[1])
    for k in post:
        assert _bits(np.asarray(apost[k][0], np.float64), np.asarray(post[k][1], np.float64)), k


def _same_marginals(a, b):
    assert np.array_equal(a.counts1, b.counts1) and np.array_equal(a.counts2, b.counts2) and a.nvalid == b.nvalid
    assert np.array_equal(a.order_ranks, b.order_ranks) and np.array_equal(a.order_stats, b.order_stats, equal_nan=True)
    assert np.array_equal(a.percentiles, b.percentiles, equal_nan=True)
    for ra, rb in ((a.regions1, b.regions1), (a.regions2, b.regions2)):
        for rowa, rowb in zip(ra, rb):
            for x, y in zip(rowa, rowb):
                assert x.thres == y.thres and x.saturated == y.saturated and np.array_equal(x.flat_cells, y.flat_cells)
                assert np.array_equal(x.density, y.density)


def test_marginals_and_regions_reuse_the_chain_reductions(three):
    s, fs, res = three
    rows = s.posterior_rows(NROWS)
    d = fs[0].model.desc
    ranges = [(d.lo[c], d.hi[c]) for c in range(2)]
    got = s.marginals(NROWS, bins_1d=40, bins_2d=20)
    assert len(got) == 3
    for r in range(3):
        _same_marginals(got[r], mg.chain_marginals(rows[r], ranges, model=fs[r], names=["theta0", "theta1"], bins_1d=40, bins_2d=20))
        assert got[r].nvalid == NROWS
    frows = s.posterior_rows(NROWS, with_fr=True)
    assert _bits(frows[:, :, 3:], rows)
    regs = s.regions(NROWS, 25, [68., 90.])
    for r in range(3):
        ref = contour.flavor_region(frows[r][:, :3], 25, [68., 90.], model=fs[r])
        for x, y in zip(regs[r], ref):
            assert x.thres == y.thres and np.array_equal(x.flat_cells, y.flat_cells) and x.mass == y.mass and x.thres > 0


def test_posterior_mean_matches_quadrature():
    """nlive = 1000: each column's mean within 5 sqrt(var_quad / ess) of the quadrature mean, ess from the device"""
    f = _tutorial(0.05)
    try:
        with nested.NestedSampler([f], [0, 1], np.zeros(2), nlive=1000, seed=3) as s:
            s.run()
            post = s.posterior()
    finally:
        f.close()
    asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=0.05)
    n1, n2 = 3000, 6000
    a1, c2 = (np.arange(n1) + 0.5) / n1, -1 + 2 * (np.arange(n2) + 0.5) / n2
    bf = fr_utils.angles_to_fr(asimov.values)
    acc = []
    for a in np.array_split(a1, 30):
        A, Cc = np.meshgrid(a, c2, indexing="ij")
        sphi2, spsi2 = np.sqrt(A), (1 - Cc) / 2
        fr = np.stack([np.abs(sphi2 * (1 - spsi2)), np.abs(sphi2 * spsi2), np.abs(1 - sphi2)], axis=-1)
        lg = llh_utils.multi_gaussian(fr, bf, 0.05)
        m = lg.max()
        w = np.exp(lg - m)
        acc.append((m, w.sum(), (w * A).sum(), (w * Cc).sum(), (w * A * A).sum(), (w * Cc * Cc).sum()))
    top = max(x[0] for x in acc)
    tot = np.sum([np.array(x[1:]) * np.exp(x[0] - top) for x in acc], axis=0)
    mean = tot[1:3] / tot[0]
    var = tot[3:5] / tot[0] - mean ** 2
    ess = post["ess"][0]
    print("quadrature mean %r var %r; device mean %r ess %.1f" % (mean, var, post["mean"][0], ess))
    assert ess > 100
    assert np.all(np.abs(post["mean"][0] - mean) < 5 * np.sqrt(var / ess)), (post["mean"][0], mean, var, ess)
    assert np.allclose(np.diag(post["cov"][0]), var, rtol=0.5)


@pytest.fixture(scope="module")
def sens_like():
    """Cf.sens_paramsets(6, (1, 1, 1)), two scales, nlive 100, non-unitary points outside the support"""
    args = TN.sens_args()
    asimov, ps = TN.sens_sets()
    scales = nested.sens_scales(6, 10)[[1, 4]]
    res = nested.evidence_scan(args, asimov, ps, scales, run_ids=[1, 4], nlive=100, batch=12, walks=10, seed=7, on_nonunitary="-inf", return_sampler=True)
    yield res, ps
    res["sampler"].close()
    for m in res["models"]:
        m.close()


def test_sens_shaped_rows_carry_the_propagated_composition(sens_like):
    res, ps = sens_like
    s = res["sampler"]
    rows, index = s.posterior_rows(500, with_fr=True, return_index=True)
    assert rows.shape == (2, 500, 3 + 12)
    for r in range(2):
        assert np.isfinite(res["lnz"][r]) and index[r].min() >= 0
        assert _bits(rows[r][:, 3:], s.dead(r)["theta"][index[r]])
        fr, st = res["models"][r].propagate(rows[r][:, 3:])
        fr[st != 0] = np.nan
        assert _bits(rows[r][:, :3], fr) and np.isfinite(fr).any()


def test_element_space_marginals_equal_the_host_rows_pushed_through(sens_like):
    res, ps = sens_like
    s = res["sampler"]
    rows = s.posterior_rows(500)
    plan, names, ranges = elements.element_plan(ps)
    got = s.marginals(500, space="elements", llh_paramset=ps, bins_1d=30, bins_2d=10)
    for r in range(2):
        erows = elements.element_rows(rows[r], plan, model=res["models"][r])
        _same_marginals(got[r], mg.chain_marginals(erows, ranges, model=res["models"][r], names=names, bins_1d=30, bins_2d=10))
        assert list(got[r].names) == list(names)


def test_sens_driver_writes_posteriors_and_leaves_fr_stat_alone(tmp_path):
    base = [sys.executable, "-m", "golemflavor_amd.sens", "--segments", "2", "--mn-live-points", "100", "--mn-walks", "10", "--smearing", "0.1",
            "--seed", "3"]
    with_p = subprocess.run(base + ["--datadir", str(tmp_path / "a"), "--posterior", "--posterior-rows", "512", "--posterior-elements"], cwd=ROOT,
                            capture_output=True, text=True, timeout=300)
    assert with_p.returncode == 0, with_p.stderr[-3000:]
    without = subprocess.run(base + ["--datadir", str(tmp_path / "b")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert without.returncode == 0, without.stderr[-3000:]
    la, lb = json.loads(with_p.stdout.strip().splitlines()[-1]), json.loads(without.stdout.strip().splitlines()[-1])
    for k in ("fr_stat", "fr_maxllh"):
        assert open(la[k], "rb").read() == open(lb[k], "rb").read(), k
    assert len(la["posterior"]) == 4 and "posterior" not in lb
    for f in la["posterior"]:
        assert os.path.dirname(f) == os.path.dirname(la["fr_stat"]) and os.path.basename(f).startswith("posterior")
        z = np.load(f)
        w = 12 if "posterior_elements" not in f else len(z["names"])
        for k in mg.MarginalResult.ARRAYS + ("names", "r1_thres", "r2_thres", "r1_cells", "r2_cells", "ess", "npoints", "mean", "cov"):
            assert k in z.files, (f, k)
        assert z["counts1"].shape == (w, 100) and z["counts2"].shape == (w * (w - 1) // 2, 50, 50)
        assert z["mean"].shape == (12,) and z["cov"].shape == (12, 12) and z["ess"].shape == () and z["ess"] > 1 and z["npoints"] > 100
        assert int(z["nvalid"]) == 512


def test_runs_without_a_posterior(three):
    s, fs, res = three
    # before run()
    with nested.NestedSampler([fs[0]], [0, 1], np.zeros(2), **KW) as fresh:
        rows, index = fresh.posterior_rows(64, return_index=True)
        post = fresh.posterior()
        assert np.all(index == -1) and np.all(np.isnan(rows)) and post["ess"][0] == 0 and post["npoints"][0] == 0
        assert np.isnan(post["mean"]).all() and np.isnan(post["cov"]).all() and np.isnan(post["lnz_check"][0])
        assert np.all(np.isnan(fresh.posterior_rows(64, with_fr=True)))
        # nrows = 0 is refused and the sampler stays usable
        with pytest.raises(_lib.GolemHipError) as err:
            fresh.posterior_rows(0)
        assert err.value.code == _lib.GF_ERR_INVALID_ARG
        fresh.run()
        assert fresh.posterior()["ess"][0] > 1 and np.isfinite(fresh.posterior_rows(64)).all()


def test_a_failed_run_has_no_posterior_and_its_neighbours_keep_theirs():
    sc = TN._nonunitary_scale(Texture.OEU)
    assert sc is not None
    args = TN.sens_args(texture=Texture.OEU)
    asimov, ps = TN.sens_sets()
    scales = np.array([-100., sc, -100.])
    kw = dict(nlive=100, batch=12, walks=10, seed=7, on_nonunitary="raise")
    cols, models, bases, labels = nested._scan_models(args, asimov, ps, scales, None, 0)
    try:
        with nested.NestedSampler(models, cols, bases, run_ids=[0, 1, 2], **kw) as s:
            res = s.run(check=False)
            assert res["failed"].tolist() == [False, True, False]
            rows, index = s.posterior_rows(200, with_fr=True, return_index=True)
            post = s.posterior()
        with nested.NestedSampler([models[0], models[2]], cols, [bases[0], bases[2]], run_ids=[0, 2], **kw) as t:
            t.run()
            trows, tindex = t.posterior_rows(200, with_fr=True, return_index=True)
            tpost = t.posterior()
    finally:
        for m in models:
            m.close()
    assert np.all(index[1] == -1) and np.all(np.isnan(rows[1])) and post["ess"][1] == 0 and np.isnan(post["mean"][1]).all()
    for a, b in ((0, 0), (2, 1)):
        assert np.array_equal(index[a], tindex[b]) and _bits(rows[a], trows[b]) and index[a].min() >= 0
        assert _bits(post["ess"][a], tpost["ess"][b]) and _bits(post["cov"][a], tpost["cov"][b])
