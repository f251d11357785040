"""The device nested sampler (golemflavor_amd.nested, gf_nested.hip) on the GPU: evidence against closed-form and importance
Monte Carlo references, the device accounting against its host restatement, determinism and independence of the runs, the
unitarity options, and the sens.py driver end to end."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import nested
from golemflavor_amd.enums import PriorsCateg, Texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def sens_args(dimension=6, texture=Texture.OET):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=dimension, texture=texture,
                              binning=Cf.default_bin_edges(), smearing=0.02, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


def sens_sets(dimension=6):
    return Cf.sens_paramsets(dimension, (1., 1., 1.))


def run_scan(scales, run_ids=None, **kw):
    args = sens_args()
    asimov, ps = sens_sets()
    kw.setdefault("seed", 7)
    return nested.evidence_scan(args, asimov, ps, scales, run_ids=run_ids, **kw)


def test_tutorial_evidence_matches_quadrature():
    angles = fr_utils.fr_to_angles((1., 2., 0.))
    asimov, ps = Cf.tutorial_paramsets(angles, smearing=0.05)
    f = llh_utils.tutorial_ln_prob(asimov, ps)
    try:
        with nested.NestedSampler([f], [0, 1], np.zeros(2), nlive=1000, seed=3) as s:
            res = s.run()
    finally:
        f.close()
    # Z over the unit cube = (1 / box area) * integral of exp(multi_gaussian(angles_to_fr(theta))) over the box (flat priors)
    n1, n2 = 3000, 6000
    a1 = (np.arange(n1) + 0.5) / n1
    bf = fr_utils.angles_to_fr(asimov.values)
    chunks = []
    for a in np.array_split(a1, 30):
        A, Cc = np.meshgrid(a, -1 + 2 * (np.arange(n2) + 0.5) / n2, indexing="ij")
        sphi2, spsi2 = np.sqrt(A), (1 - Cc) / 2
        fr = np.stack([np.abs(sphi2 * (1 - spsi2)), np.abs(sphi2 * spsi2), np.abs(1 - sphi2)], axis=-1)
        lg = llh_utils.multi_gaussian(fr, bf, 0.05)
        m = lg.max()
        chunks.append((m, np.exp(lg - m).sum()))
    top = max(m for m, _ in chunks)
    lnz_quad = top + np.log(sum(s * np.exp(m - top) for m, s in chunks)) - np.log(n1 * n2)
    sig = res["lnz_err"][0]
    assert np.isfinite(res["lnz"][0]) and sig > 0
    assert abs(res["lnz"][0] - lnz_quad) < 4 * sig, (res["lnz"][0], lnz_quad, sig)


def _importance_lnz(ps, scale, rng, max_draws=100_000_000, chunk=2_000_000, target=0.02):
    """ln Z over the unit cube of every column but the scale by importance sampling from q = each column's own prior,
    truncated to its box: Z = prod(1 / w_i) mean(exp(lnprob - ln q)).  Returns (ln Z, its standard error)."""
    from scipy.stats import truncnorm
    from golemflavor_amd.model import Model
    sp = nested._scale_paramset(ps, scale)
    args = sens_args()
    asimov, _ = sens_sets()
    names = list(sp.names)
    scol = names.index("logLam")
    cols = [i for i in range(len(names)) if i != scol]
    box = np.array(sp.ranges, dtype=float)
    width = box[cols, 1] - box[cols, 0]
    dists = []
    for i in cols:
        p = sp[i]
        lo, hi = box[i]
        if p.prior in (PriorsCateg.GAUSSIAN, PriorsCateg.LIMITEDGAUSS):
            mu, sd = float(p.nominal_value), float(p.std)
            dists.append(truncnorm((lo - mu) / sd, (hi - mu) / sd, loc=mu, scale=sd))
        else:
            dists.append(None)
    n, s1, s2, shift = 0, 0.0, 0.0, None
    with Model(nested._bsm_desc(args, asimov, sp, 0.02)) as m:
        while n < max_draws:
            th = np.tile(np.array(sp.values, dtype=float), (chunk, 1))
            lnq = np.zeros(chunk)
            for k, i in enumerate(cols):
                if dists[k] is None:
                    th[:, i] = rng.uniform(box[i, 0], box[i, 1], chunk)
                    lnq -= np.log(width[k])
                else:
                    x = dists[k].rvs(size=chunk, random_state=rng)
                    th[:, i] = x
                    lnq += dists[k].logpdf(x)
            lp, st = m.lnprob(th, want_status=True)
            lw = np.where(st == _lib.GF_ST_OK, lp - lnq, -np.inf)
            if shift is None:
                if not np.isfinite(lw).any():
                    if n + chunk >= 10 * chunk:
                        return -np.inf, 0.0
                    n += chunk
                    continue
                shift = np.max(lw[np.isfinite(lw)])
            w = np.exp(lw - shift)
            s1 += w.sum(); s2 += (w * w).sum(); n += chunk
            mean = s1 / n
            se = np.sqrt(max(s2 / n - mean * mean, 0.0) / n) / mean
            if se < target and n >= 10 * chunk:
                break
    return shift + np.log(mean) - np.sum(np.log(width)), se


def test_sens_evidence_matches_importance_monte_carlo():
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    scales = np.array([-100., 0.5 * (lo + hi), float(hi)])
    res = run_scan(scales)
    _, ps = sens_sets()
    rng = np.random.default_rng(11)
    for k, sc in enumerate(scales):
        lnz_mc, se_mc = _importance_lnz(ps, sc, rng)
        if lnz_mc == -np.inf:
            # the Gaussian likelihood underflows (llh.py:32-54) on every draw: Z = 0 in fp64, and the device must say so
            print("scale %g: every importance draw has L = 0; nested ln Z %r" % (sc, res["lnz"][k]))
            assert res["lnz"][k] == -np.inf
            continue
        assert se_mc < 0.05, "importance Monte Carlo too noisy at scale %g: sigma %.3f" % (sc, se_mc)
        sig = np.sqrt(res["lnz_err"][k] ** 2 + se_mc ** 2)
        print("scale %g: ln Z nested %.4f +- %.4f, importance MC %.4f +- %.4f" % (sc, res["lnz"][k], res["lnz_err"][k],
                                                                                  lnz_mc, se_mc))
        assert abs(res["lnz"][k] - lnz_mc) < 4 * sig, (sc, res["lnz"][k], lnz_mc, sig)


@pytest.mark.parametrize("scale", [-43.5, -42.75, -42.5, -42.25])
def test_sens_evidence_in_the_falloff_band(scale):
    """Where part of the cube has L = 0 (about 18, 49, 68 and 92 % of it at these scales) the plateau is removed without
    replacement; charging it the per-batch compression instead overstates ln Z by about -1.06 f - ln(1 - f)."""
    res = run_scan(np.array([scale]))
    _, ps = sens_sets()
    lnz_mc, se_mc = _importance_lnz(ps, scale, np.random.default_rng(12))
    assert np.isfinite(lnz_mc) and se_mc < 0.05, (scale, lnz_mc, se_mc)
    sig = np.sqrt(res["lnz_err"][0] ** 2 + se_mc ** 2)
    print("scale %g: ln Z nested %.4f +- %.4f, importance MC %.4f +- %.4f" % (scale, res["lnz"][0], res["lnz_err"][0], lnz_mc,
                                                                              se_mc))
    assert abs(res["lnz"][0] - lnz_mc) < 4 * sig, (scale, res["lnz"][0], lnz_mc, sig)


def test_device_accounting_matches_host_restatement():
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    res = run_scan(np.array([-100., lo]), nlive=600, return_sampler=True)
    s = res["sampler"]
    try:
        for r in range(2):
            d = s.dead(r)
            nd = d["ndead"]
            host = nested.evidence_from_dead(d["lnl"][:nd], d["nlive_seq"], live_lnl=d["lnl"][nd:])
            assert abs(host["lnz"] - res["lnz"][r]) <= 1e-12 * abs(res["lnz"][r]), (host["lnz"], res["lnz"][r])
            assert nd == res["niter"][r] * s.batch
            assert np.all(np.diff(d["lnl"][:nd].reshape(-1, s.batch), axis=1) >= 0)     # removed in ascending lnL
            assert np.max(d["lnl"]) == res["max_lnl"][r]
    finally:
        s.close()
        for m in res["models"]:
            m.close()


def test_runs_are_deterministic_and_independent():
    sc = nested.sens_scales(6, 10)
    ids = np.array([1, 4, 8])
    kw = dict(nlive=500)
    together = run_scan(sc[ids], run_ids=ids, **kw)
    alone = run_scan(sc[ids[1:2]], run_ids=ids[1:2], **kw)
    again = run_scan(sc[ids], run_ids=ids, **kw)
    for key in ("lnz", "lnz_err", "max_lnl", "niter", "nevals"):
        assert together[key][1] == alone[key][0], key
        assert np.array_equal(together[key], again[key]), key
    # the lanes-per-walker choice does not change a bit
    old = os.environ.get("GF_NESTED_LPW")
    try:
        for lpw in ("1", "16"):
            os.environ["GF_NESTED_LPW"] = lpw
            forced = run_scan(sc[ids[1:2]], run_ids=ids[1:2], **kw)
            assert forced["lnz"][0] == alone["lnz"][0] and forced["nevals"][0] == alone["nevals"][0], lpw
    finally:
        if old is None:
            os.environ.pop("GF_NESTED_LPW", None)
        else:
            os.environ["GF_NESTED_LPW"] = old


def _nonunitary_scale(texture):
    args = sens_args(texture=texture)
    asimov, ps = sens_sets()
    rng = np.random.default_rng(5)
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    for sc in np.linspace(lo, hi, 27):
        sp = nested._scale_paramset(ps, float(sc))
        f = llh_utils.bsm_ln_prob(args, asimov, sp, on_nonunitary="-inf", check_unitarity=True)
        try:
            box = np.array(sp.ranges, dtype=float)
            th = rng.uniform(box[:, 0], box[:, 1], size=(20000, len(sp)))
            th[:, list(sp.names).index("logLam")] = sc
            _, st = f.model.lnprob(th, want_status=True)
        finally:
            f.close()
        if np.any(st == _lib.GF_ST_NON_UNITARY):
            return float(sc)
    return None


def test_nonunitary_options():
    # texture OEU: at the scales where its prior draws start to fail the reference's unitarity assert (about 1 % near -36) most
    # of the cube is still finite (OET has no such scale: its likelihood underflows everywhere first)
    sc = _nonunitary_scale(Texture.OEU)
    assert sc is not None, "no scale of the d = 6 OEU sens posterior has prior draws the reference would raise on"
    args = sens_args(texture=Texture.OEU)
    asimov, ps = sens_sets()
    kw = dict(nlive=400, seed=7)
    res = nested.evidence_scan(args, asimov, ps, np.array([sc]), on_nonunitary="-inf", **kw)
    assert res["nonunitary"][0] > 0 and np.isfinite(res["lnz"][0])
    with pytest.raises(AssertionError, match="scale %.6g" % sc):
        nested.evidence_scan(args, asimov, ps, np.array([sc]), on_nonunitary="raise", **kw)


def test_sens_cli_end_to_end(tmp_path):
    # --smearing 0.1: with the default 0.02 the Gaussian likelihood underflows everywhere at the top scale of d = 6 OET from a
    # (0, 1, 0) source (ln Z = -inf there, test_sens_evidence_matches_importance_monte_carlo); a wider one keeps every row finite
    out = subprocess.run([sys.executable, "-m", "golemflavor_amd.sens", "--segments", "4", "--mn-live-points", "400",
                          "--smearing", "0.1", "--datadir", str(tmp_path), "--seed", "3"], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    stat, mx = np.load(line["fr_stat"]), np.load(line["fr_maxllh"])
    assert stat.shape == (4, 2) and mx.shape == (4, 2)
    assert np.all(np.isfinite(stat)) and np.all(np.isfinite(mx))
    assert np.array_equal(stat[:, 0], nested.sens_scales(6, 4))
    lim = nested.bayes_factor_limit(stat[:, 0], stat[:, 1])
    assert lim is None or np.isfinite(lim)
