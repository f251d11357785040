"""GPU: the tempered ensemble sampler (gf_sampler_create_tempered, csrc/gf_temper.hip) -- lnprior and lnL apart, the
tempered half-step, replica exchange, the device reduction behind the estimators and the stepping-stone evidence.  The yardsticks:
`Model.lnprob` (held to the oracle by tests/test_gpu_parity.py) for the split evaluation; the numpy stretch move of tests/stretch_ref.py
on the sampler's Philox stream, fed T = lp + beta lnl built in numpy from `Model.lnprior_lnlike`, for the half-step; a numpy restatement
of the round (tests/temper_harness.py) for the exchange; the host build of csrc/gf_temper.hpp for the reduction; a direct average over
prior draws for the evidence.  Every comparison but the last is bit for bit."""
import math
import os

import numpy as np
import pytest

import temper_harness as TH
from common import BIN_EDGES, TEX_BY_VALUE, bsm_args, rel_err
from golemflavor_amd import _lib, llh, tempering
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, PriorsCateg, Texture
from golemflavor_amd.model import Model
from stretch_ref import reference_stretch
from test_gpu_binned_sampler import a_measurement, assert_same_run, device_run, same_bits
from test_gpu_table_sampler import forced_lpw

pytestmark = pytest.mark.gpu

REL = 1e-10
NW = 24                  # the smallest legal ensemble of the 12-column posterior
SRC = fr_utils.normalize_fr((0., 1., 0.))


# ---- the posteriors ----------------------------------------------------------------------------------------------------------------------
def sens_sets():
    return Cf.sens_paramsets(6, (1., 1., 1.))


def sens_kw(smearing, texture=Texture.OET):
    asimov, _ = sens_sets()
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    return dict(bestfit_fr=bf, smearing=smearing, source_ratio=SRC, texture=texture, dimension=6, binning=BIN_EDGES)


def sens_lnprob(smearing, texture=Texture.OET):
    """the 12-column sens posterior (source (0, 1, 0)) as an LnProb whose non-unitary proposals score -inf"""
    return llh.LnProb(compile_model(sens_sets()[1], "BSM_GAUSS", **sens_kw(smearing, texture)), on_nonunitary="-inf")


def failing_lnprob():
    """texture OEU across the top of its scale range: the model of test_bsm_sampler_unitarity_through_the_failing_region"""
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    return llh.bsm_ln_prob(bsm_args(6, Texture.OEU, (1 / 3, 2 / 3, 0.)), asimov, ps, smearing=0.3, on_nonunitary="-inf"), ps


def failing_rows(ps, n, rng):
    box = np.array(ps.seeds, dtype=float)
    th = rng.uniform(box[:, 0], box[:, 1], size=(n, len(ps)))
    th[:, 11] = rng.uniform(-40.0, -30.0, n)
    return th


def prior_draws(ps, n, rng):
    """n draws of the prior over the box: uniform columns uniformly, Gaussian ones (truncated or cut by the box alike) by rejection"""
    out = np.empty((n, len(ps)))
    for c, p in enumerate(ps):
        lo, hi = float(p.ranges[0]), float(p.ranges[1])
        if p.prior is PriorsCateg.UNIFORM:
            out[:, c] = rng.uniform(lo, hi, n)
            continue
        x = np.empty(0)
        while x.size < n:
            d = rng.normal(float(p.nominal_value), float(p.std), 2 * n)
            x = np.concatenate([x, d[(d >= lo) & (d <= hi)]])
        out[:, c] = x[:n]
    return out


@pytest.fixture(scope="module")
def posts():
    """the module's posteriors, made once: the sens posterior at smearing 0.02 (a plateau of lnl = -inf over half the prior) and 0.1, a
    second texture, and the failing-region model"""
    f = {"s002": sens_lnprob(0.02), "s01": sens_lnprob(0.1), "out01": sens_lnprob(0.1, Texture.OUT)}
    f["oeu"], oeu_ps = failing_lnprob()
    f["ps"], f["oeu_ps"] = sens_sets()[1], oeu_ps
    yield f
    for k in ("s002", "s01", "out01", "oeu"):
        f[k].close()


def tempered(fns, betas, nw=NW, seed=5, swap_every=0, ngroups=None, stream_ids=None, ndim=12):
    return mcmc_utils.DeviceEnsembleSampler(nw, ndim, fns, seed=seed, betas=betas, swap_every=swap_every, ngroups=ngroups, stream_ids=stream_ids)


# ---- 1. lnprior and lnl apart ---------------------------------------------------------------------------------------------------------------
def check_split(oracle, model, om, th, what):
    th = np.ascontiguousarray(th)
    lp, lnl, st = model.lnprior_lnlike(th)
    ref, ref_st = model.lnprob(th, want_status=True)
    assert np.array_equal(st, ref_st), (what, np.flatnonzero(st != ref_st)[:10])
    ok = st == _lib.GF_ST_OK
    with np.errstate(invalid="ignore"):
        assert same_bits((lp + lnl)[ok], ref[ok]), what
    out = st == _lib.GF_ST_OUT_OF_PRIOR
    assert np.all(lp[out] == -np.inf) and np.all(lnl[out] == -np.inf)
    assert np.all(np.isnan(lnl[st == _lib.GF_ST_NON_UNITARY]))
    want = np.array([oracle.lnprior(om, t) for t in th[~out]])
    assert np.all(np.isfinite(lp[~out])) and rel_err(lp[~out], want) <= REL, what
    return lp, lnl, st


def test_split_evaluation(golden, oracle, posts):
    """About 4 000 rows: the golden 12-column BSM rows, prior draws at smearing 0.02, rows outside the box, the failing region."""
    n = 0
    rows = golden["g9_rows"]
    for key in np.unique(rows[:, :5], axis=0):
        sel = np.all(rows[:, :5] == key, axis=1)
        dim, tex, src = int(key[0]), TEX_BY_VALUE[int(key[1])], key[2:5]
        _, ps = Cf.fr_paramsets(dim, (0.4, 0.0))
        kw = dict(dimension=dim, binning=BIN_EDGES, source_ratio=src, bestfit_fr=golden["g9_injected"], smearing=0.02)
        om = oracle.make_model(ps, "BSM_GAUSS", texture=tex.name, **kw)
        with Model(compile_model(ps, "BSM_GAUSS", texture=tex, **kw)) as m:
            check_split(oracle, m, om, rows[sel][:, 5:], "golden rows %s" % key)
        n += int(sel.sum())
    rng = np.random.default_rng(31)
    ps = posts["ps"]
    th = prior_draws(ps, 2048, rng)
    far = prior_draws(ps, 256, rng)                                      # outside the box: one column each, below or above its range
    for i in range(len(far)):
        c = i % len(ps)
        lo, hi = ps[c].ranges
        far[i, c] = lo - (hi - lo) * 0.01 * (1 + i % 7) if i % 2 else hi + (hi - lo) * 0.01 * (1 + i % 5)
    om = oracle.make_model(ps, "BSM_GAUSS", **{**sens_kw(0.02), "texture": "OET"})
    lp, lnl, st = check_split(oracle, posts["s002"].model, om, np.concatenate([th, far]), "sens posterior, smearing 0.02")
    plateau = int(np.sum((st == _lib.GF_ST_OK) & (lnl == -np.inf)))
    print("sens posterior at smearing 0.02: %d of %d prior draws on the plateau lnl = -inf" % (plateau, len(th)))
    assert plateau > 0.3 * len(th) and np.all(st[len(th):] == _lib.GF_ST_OUT_OF_PRIOR)
    n += len(th) + len(far)
    ops = posts["oeu_ps"]
    om = oracle.make_model(ops, "BSM_GAUSS", texture="OEU", dimension=6, binning=BIN_EDGES, source_ratio=(1 / 3, 2 / 3, 0.),
                           bestfit_fr=fr_utils.angles_to_fr(fr_utils.fr_to_angles((1, 1, 1))), smearing=0.3)
    _, _, st = check_split(oracle, posts["oeu"].model, om, failing_rows(ops, 1024, rng), "the failing region")
    assert np.sum(st == _lib.GF_ST_NON_UNITARY) > 100 and np.sum(st == _lib.GF_ST_OK) > 100
    n += 1024
    print("%d rows" % n)
    assert n >= 3500


# ---- 2. beta = 1 is the untempered sampler ----------------------------------------------------------------------------------------------------
def test_beta_one_is_the_untempered_sampler(posts):
    """betas = [1], two groups with different models, 40 steps at thin 3 -- graph replays and eager steps -- against the multi-model
    sampler on the same seed and stream ids"""
    fns = [posts["s01"], posts["out01"]]
    p0 = np.stack([prior_draws(posts["ps"], NW, np.random.default_rng(s)) for s in (41, 42)])
    ids = (7, 2)
    a = tempered(fns, [1.0], seed=17, ngroups=2, stream_ids=ids)
    b = mcmc_utils.DeviceEnsembleSampler(NW, 12, fns, seed=17, stream_ids=ids)
    try:
        assert a.nchains == 2 and np.array_equal(a.cold_chains, [0, 1]) and a.launch_shape()["shape"] == "grid"
        a.run_mcmc(p0, 40, thin=3)
        b.run_mcmc(p0, 40, thin=3)
        ra, rb = device_run(a), device_run(b)
        assert ra["chain"].shape == (2, 14, NW, 12)
        assert_same_run(ra, rb, "betas = [1] against the multi-model sampler")
        assert a.nonunitary_proposals == b.nonunitary_proposals
    finally:
        a.close()
        b.close()


# ---- 3. the tempered half-step against numpy ----------------------------------------------------------------------------------------------------
def numpy_T(om, q):
    """a reference_stretch `lnprob`: om = (Model, beta); T from the split evaluation, -inf where the reference would have raised"""
    model, beta = om
    lp, lnl, st = model.lnprior_lnlike(np.ascontiguousarray(q))
    return np.where(st == _lib.GF_ST_NON_UNITARY, -np.inf, TH.temper(lp, lnl, beta))


_REFS = {}


def shared(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


BETAS3 = [1.0, 0.25, 0.0]


@pytest.mark.parametrize("lpw", [1, 2, 4, 16])
def test_tempered_half_step_on_the_plateau(oracle, posts, lpw):
    """smearing 0.02: half the prior has lnl = -inf, and the beta = 0 chain lives there as well as anywhere"""
    f = posts["s002"]
    p0 = prior_draws(posts["ps"], 3 * NW, np.random.default_rng(51)).reshape(3, NW, 12)
    with forced_lpw(lpw):
        smp = tempered(f, BETAS3, seed=23)
        try:
            smp.run_mcmc(p0, 20)
            assert smp.launch_shape() == {**smp.launch_shape(), "shape": "grid", "lanes_per_walker": lpw}
            ref = shared("plateau", lambda: reference_stretch(oracle, [(f.model, b) for b in BETAS3], p0, 20, 23, lnprob=numpy_T, full=True))
            got = device_run(smp)
            assert_same_run(got, ref, "betas %s, %d lanes per walker" % (BETAS3, lpw))
            lnl = f.model.lnprior_lnlike(got["chain"][2].reshape(-1, 12))[1]
            assert np.sum(lnl == -np.inf) > 0, "the prior chain stores no sample with lnl = -inf"
            assert np.all(np.isfinite(got["lnp_chain"][2][got["lnp_chain"][2] > -np.inf]))
        finally:
            smp.close()


def test_tempered_half_step_rounds_the_product_and_the_sum(oracle, posts):
    """betas that are no powers of two: beta * lnl is inexact, and T fused into one fma would differ from the two roundings in about
    every third walker (at 0.25 the product is exact and the two agree)"""
    f = posts["s01"]
    betas = [1.0, 0.3, 0.07]
    p0 = prior_draws(posts["ps"], 3 * NW, np.random.default_rng(53)).reshape(3, NW, 12)
    smp = tempered(f, betas, seed=31)
    try:
        smp.run_mcmc(p0, 12)
        ref = reference_stretch(oracle, [(f.model, b) for b in betas], p0, 12, 31, lnprob=numpy_T, full=True)
        assert_same_run(device_run(smp), ref, "betas %s" % betas)
        lp, lnl, _ = f.model.lnprior_lnlike(p0[1])
        with np.errstate(invalid="ignore"):
            fused = np.array([TH.fma(0.3, float(b), float(a)) for a, b in zip(lp, lnl)])
        assert np.sum(fused != TH.temper(lp, lnl, 0.3)) > 0, "the start positions do not tell the fused sum from the rounded one"
    finally:
        smp.close()


@pytest.mark.parametrize("lpw", [1, 2, 4, 16])
def test_tempered_half_step_through_the_failing_region(oracle, posts, lpw):
    """texture OEU where the reference raises: the verdict, parking and settlement apply at every beta, the prior chain included"""
    f = posts["oeu"]
    p0 = failing_rows(posts["oeu_ps"], 3 * NW, np.random.default_rng(52)).reshape(3, NW, 12)
    with forced_lpw(lpw):
        smp = tempered(f, BETAS3, seed=29)
        try:
            smp.run_mcmc(p0, 20)
            ref = shared("failing", lambda: reference_stretch(oracle, [(f.model, b) for b in BETAS3], p0, 20, 29, lnprob=numpy_T, full=True))
            got = device_run(smp)
            assert_same_run(got, ref, "failing region, %d lanes per walker" % lpw)
            print("parked %d, non-unitary %d" % (smp.parked_proposals, smp.nonunitary_proposals))
            assert smp.parked_proposals > 0 and smp.nonunitary_proposals > 0
            # no sample the reference would have died on is in any chain
            st = f.model.lnprior_lnlike(got["chain"][:, :, :, :].reshape(-1, 12))[2]
            moved = np.isfinite(got["lnp_chain"].reshape(-1))
            assert not np.any(st[moved] == _lib.GF_ST_NON_UNITARY)
        finally:
            smp.close()


# ---- 4. replica exchange against a numpy restatement of the round ---------------------------------------------------------------------------
def numpy_tempered(oracle, models, betas, p0, nsteps, seed, swap_every, stream_ids=None, rounds=None):
    """The tempered run in numpy: reference_stretch between the rounds, TH.swap_round for a round.  models: one per group.  rounds: a
    list that receives one dict per round -- its number, and copies of what the round started from (pos, T, lp, lnl, status) and of the
    positions it left."""
    K = len(betas)
    nch = p0.shape[0]
    oms = [(models[ch // K], betas[ch % K]) for ch in range(nch)]
    pos, lnp, it = np.array(p0), None, 0
    chain, lnp_chain = [], []
    nacc = np.zeros(p0.shape[:2], dtype=int)
    counts = np.zeros((nch, 2), dtype=np.int64)
    while it < nsteps:
        seg = nsteps - it if not swap_every else min(nsteps - it, swap_every - it % swap_every)
        r = reference_stretch(oracle, oms, pos, seg, seed, lnprob=numpy_T, full=True, iteration0=it, lnp0=lnp, stream_ids=stream_ids)
        chain.append(r["chain"])
        lnp_chain.append(r["lnp_chain"])
        pos, lnp = r["pos"], r["lnp"]
        nacc += r["nacc"]
        it += seg
        if swap_every and it % swap_every == 0:
            ev = [m.lnprior_lnlike(np.ascontiguousarray(pos[ch])) for ch, (m, _) in enumerate(oms)]
            lp, lnl = np.stack([e[0] for e in ev]), np.stack([e[1] for e in ev])
            if rounds is not None:
                rounds.append({"round": it // swap_every - 1, "pos": pos.copy(), "T": lnp.copy(), "lp": lp, "lnl": lnl,
                               "status": np.stack([e[2] for e in ev])})
            TH.swap_round(oracle, seed, it // swap_every - 1, betas, pos, lnp, lp, lnl, counts, stream_ids)
            if rounds is not None:
                rounds[-1]["pos_after"] = pos.copy()
    return {"chain": np.concatenate(chain, axis=1), "lnp_chain": np.concatenate(lnp_chain, axis=1), "pos": pos, "lnp": lnp, "nacc": nacc,
            "counts": counts}


def state_holds_the_formula(smp, models, betas, got):
    """the state's lnprob is T of the state's positions, bit for bit (a walker at -inf stays there)"""
    K = len(betas)
    for ch in range(got["pos"].shape[0]):
        want = numpy_T((models[ch // K], betas[ch % K]), got["pos"][ch])
        live = got["lnp"][ch] > -np.inf
        assert same_bits(got["lnp"][ch][live], want[live]), ch


@pytest.mark.parametrize("ntemps, swap_every, nsteps", [(4, 3, 20), (3, 3, 20), (4, 1, 6), (3, 1, 6)])
def test_swaps_against_numpy(oracle, posts, ntemps, swap_every, nsteps):
    """two groups with different models; chain, state and swap counters bit for bit; one walker starts outside the support and stays
    there: its pairs are skipped and not counted"""
    fns = [posts["s01"], posts["out01"]]
    models = [f.model for f in fns]
    betas = [1.0, 0.3, 0.05, 0.0] if ntemps == 4 else [1.0, 0.3, 0.0]
    nch = 2 * ntemps
    p0 = prior_draws(posts["ps"], nch * NW, np.random.default_rng(61)).reshape(nch, NW, 12)
    p0[1, 3, 0] = 1e6                                                     # group 0, rung 1, walker 3: no proposal from there is in the box
    ids = tuple(range(10, 10 + 3 * nch, 3))
    smp = tempered(fns, betas, seed=37, swap_every=swap_every, ngroups=2, stream_ids=ids)
    try:
        smp.run_mcmc(p0, nsteps)
        ref = shared(("swaps", ntemps, swap_every), lambda: numpy_tempered(oracle, models, betas, p0, nsteps, 37, swap_every, ids))
        got = device_run(smp)
        assert_same_run(got, ref, "%d rungs, a round every %d steps" % (ntemps, swap_every))
        prop, acc = smp.swap_counts()
        assert np.array_equal(prop.reshape(-1), ref["counts"][:, 0]) and np.array_equal(acc.reshape(-1), ref["counts"][:, 1])
        rounds = nsteps // swap_every
        print("proposed\n%s\naccepted\n%s" % (prop, acc))
        assert acc.sum() > 0 and np.all(prop[:, -1] == 0)
        # the pairs of walker 3 of group 0's rung 1 with rungs 0 and 2 were never proposed (nor is any other pair with a walker at -inf:
        # the counts are the numpy round's, above)
        r_even, r_odd = (rounds + 1) // 2, rounds // 2
        assert prop[0, 0] <= r_even * (NW - 1) and prop[0, 1] <= r_odd * (NW - 1)
        assert prop[1, 0] <= r_even * NW and prop[1, 1] <= r_odd * NW
        assert got["lnp"][1, 3] == -np.inf and got["pos"][1, 3, 0] == 1e6
        state_holds_the_formula(smp, models, betas, got)
        frac = smp.swap_fraction
        assert frac.shape == (2, ntemps - 1) and np.all((frac[np.isfinite(frac)] >= 0) & (frac[np.isfinite(frac)] <= 1))
    finally:
        smp.close()


def test_a_round_permutes_a_groups_rows(posts):
    """swap_every = 1: the stored sample of a step is what the round that follows it starts from, the state what it leaves"""
    fns = [posts["s01"], posts["out01"]]
    betas = [1.0, 0.3, 0.05, 0.0]
    p0 = prior_draws(posts["ps"], 8 * NW, np.random.default_rng(62)).reshape(8, NW, 12)
    smp = tempered(fns, betas, seed=43, swap_every=1, ngroups=2)
    try:
        moved = 0
        for step in range(6):
            smp.run_mcmc(p0 if step == 0 else None, 1)
            got = device_run(smp)
            before, after = got["chain"][:, -1], got["pos"]
            for g in range(2):
                a = before[4 * g:4 * g + 4].reshape(-1, 12)
                b = after[4 * g:4 * g + 4].reshape(-1, 12)
                assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)]), (step, g)
                # walker w of a rung is walker w of a rung still
                assert np.array_equal(np.sort(before[4 * g:4 * g + 4], axis=0), np.sort(after[4 * g:4 * g + 4], axis=0))
            moved += int(np.sum(np.any(before != after, axis=2)))
        assert moved > 0
    finally:
        smp.close()


def test_graph_replays_and_eager_steps_give_the_same_chain(posts):
    """48 steps with a round every 20: graph replays of 16 steps and eager steps between the rounds, against eager steps alone"""
    fns = [posts["s01"], posts["out01"]]
    betas = [1.0, 0.3, 0.0]
    p0 = prior_draws(posts["ps"], 6 * NW, np.random.default_rng(63)).reshape(6, NW, 12)
    runs = []
    old = os.environ.pop("GF_SAMPLER_NO_GRAPH", None)
    try:
        for no_graph in (False, True):
            if no_graph:
                os.environ["GF_SAMPLER_NO_GRAPH"] = "1"
            smp = tempered(fns, betas, seed=47, swap_every=20, ngroups=2)
            try:
                smp.run_mcmc(p0, 48, thin=2)
                runs.append((device_run(smp), smp.swap_counts()))
            finally:
                smp.close()
    finally:
        os.environ.pop("GF_SAMPLER_NO_GRAPH", None)
        if old is not None:
            os.environ["GF_SAMPLER_NO_GRAPH"] = old
    (a, ca), (b, cb) = runs
    assert_same_run(a, b, "graph replays against eager steps")
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and ca[0].sum() > 0


def rounds_run(posts, run):
    """the shape of the test above -- 6 chains, a round every 20 steps: 16 replayed and 4 eager steps before each, an 8-step tail of 48 --
    on a fresh sampler: what `run(smp, p0)` returns, what it left on the device, and the swap counts"""
    p0 = prior_draws(posts["ps"], 6 * NW, np.random.default_rng(63)).reshape(6, NW, 12)
    smp = tempered([posts["s01"], posts["out01"]], [1.0, 0.3, 0.0], seed=47, swap_every=20, ngroups=2)
    try:
        out = run(smp, p0)
        return out, device_run(smp), smp.swap_counts()
    finally:
        smp.close()


def whole_run(posts):
    return shared("rounds: 48 steps at thin 2", lambda: rounds_run(posts, lambda smp, p0: smp.run_mcmc(p0, 48, thin=2))[1:])


def test_read_back_during_a_tempered_run(posts):
    """run_mcmc_to_host over two rounds: what crossed to the host block by block is the stored chain of the same run, bit for bit, and
    the run is the one run_mcmc makes"""
    ref, counts = whole_run(posts)
    (c, lnp), got, cb = rounds_run(posts, lambda smp, p0: smp.run_mcmc_to_host(p0, 48, thin=2, lnprob=True))
    assert c.shape == (6, 24, NW, 12) and lnp.shape == (6, 24, NW)
    assert same_bits(c, ref["chain"]) and same_bits(lnp, ref["lnp_chain"])
    assert_same_run(got, ref, "run_mcmc_to_host against run_mcmc")
    assert np.array_equal(cb[0], counts[0]) and np.array_equal(cb[1], counts[1]) and counts[0].sum() > 0


def test_a_run_continued_across_a_round(posts):
    """30 steps, then 18: rounds are counted from creation, so the second run has its round behind its 10th step, and the two are the
    single run of 48.  Both are below the 32 steps from which a run replays a graph: eager blocks cut at other steps than the single
    run's replays and blocks, the same chain."""
    ref, counts = whole_run(posts)

    def two_runs(smp, p0):
        smp.run_mcmc(p0, 30, thin=2)
        smp.run_mcmc(None, 18, thin=2)

    _, got, cb = rounds_run(posts, two_runs)
    assert_same_run(got, ref, "30 + 18 steps against 48")
    assert np.array_equal(cb[0], counts[0]) and np.array_equal(cb[1], counts[1]) and counts[0].sum() > 0


# ---- 5. the series kernel ----------------------------------------------------------------------------------------------------------------------
def series_against_host(smp, models, betas):
    """(series, lnl) of the stored chain, held to the host build of gf_temper.hpp fed lnprior_lnlike of the stored chain; models: one
    per group"""
    K = len(betas)
    ser, lnl = smp.lnl_series(want_lnl=True)
    chain = device_run(smp)["chain"]
    nch, nsteps, nw, ndim = chain.shape
    assert ser.shape == (nch, nsteps, 5) and lnl.shape == (nch, nsteps, nw)
    b = np.array(betas)
    d_up = np.concatenate([[0.0], b[:-1] - b[1:]])                     # the distance in beta to the rung above, and below
    d_dn = np.concatenate([b[:-1] - b[1:], [0.0]])
    for ch in range(nch):
        want_lnl = models[ch // K].lnprior_lnlike(chain[ch].reshape(-1, ndim))[1].reshape(nsteps, nw)
        fin = np.isfinite(want_lnl)
        assert np.array_equal(fin, np.isfinite(lnl[ch])) and same_bits(lnl[ch][fin], want_lnl[fin])
        want = TH.host_series(want_lnl, d_up[ch % K], d_dn[ch % K])
        assert same_bits(ser[ch], want), (ch, ser[ch], want)
    return ser, lnl


@pytest.mark.parametrize("nw, nsteps", [(24, 1), (24, 7), (100, 1), (100, 7)])
def test_series_against_the_host_build(posts, nw, nsteps):
    """all five outputs against the host build of gf_temper.hpp fed lnprior_lnlike of the stored chain; rung 1 starts outside the
    support and stays there: count 0, sums 0, max -inf"""
    f = posts["s002"]
    betas = [1.0, 0.4, 0.1, 0.0]
    p0 = prior_draws(posts["ps"], 4 * nw, np.random.default_rng(71)).reshape(4, nw, 12)
    p0[1, :, 0] = 1e6
    smp = tempered(f, betas, nw=nw, seed=53, swap_every=2)
    try:
        smp.run_mcmc(p0, nsteps)
        ser, lnl = series_against_host(smp, [f.model], betas)
        assert ser.shape == (4, nsteps, 5) and lnl.shape == (4, nsteps, nw)
        assert np.all(ser[1, :, 0] == 0) and np.all(ser[1, :, 1] == 0) and np.all(ser[1, :, 2] == -np.inf) and np.all(ser[1, :, 3:] == 0)
        assert np.all(ser[0, :, 0] > 0) and np.any(ser[3, :, 0] < nw)          # the prior chain holds samples on the plateau
        assert same_bits(smp.lnlikelihood(), lnl.transpose(0, 2, 1))
    finally:
        smp.close()


# ---- 6. the evidence against a direct average ----------------------------------------------------------------------------------------------------
def test_stepping_stone_evidence_against_a_direct_average(posts):
    """The sens posterior at smearing 0.1.  Reference: ln mean_prior(L) from 2^20 prior draws through Model.lnprior_lnlike, its standard
    error from the draws.  Tempered run: geometric_ladder(8, 1e-3), 256 walkers, a round every 8 steps, 500 burn-in + 1500 stored steps.
    Pass iff |ln_ratio - reference| <= 5 sqrt(err_ss^2 + err_ref^2) and err_ss <= 0.1."""
    f, ps = posts["s01"], posts["ps"]
    rng = np.random.default_rng(2024)
    th = prior_draws(ps, 1 << 20, rng)
    lp, lnl, st = f.model.lnprior_lnlike(th)
    bad = st != _lib.GF_ST_OK
    print("%d of 2^20 prior draws are not OK (L = 0 for them, as for the sampler), %d have a non-finite lnl" % (bad.sum(), np.sum(~np.isfinite(lnl))))
    assert bad.sum() < 1e-3 * len(st)
    m = lnl[~bad].max()
    with np.errstate(invalid="ignore"):
        w = np.where(bad, 0.0, np.exp(lnl - m))
    ref = m + math.log(w.mean())
    err_ref = float(w.std(ddof=1) / math.sqrt(len(w)) / w.mean())
    print("direct average over 2^20 prior draws: ln mean L = %.4f, relative standard error %.4f" % (ref, err_ref))
    assert err_ref <= 0.01
    betas = tempering.geometric_ladder(8, 1e-3)
    smp = tempered(f, betas, nw=256, seed=97, swap_every=8)
    try:
        # the start: prior draws of their own, resampled to every rung (tempering.ladder_start has the reason).  Measured from plain
        # prior draws on every rung, at these lengths: ln_ratio - reference = -0.052, -0.042, -0.028, -0.032 over four seeds at
        # err_ss 0.005 to 0.009 -- the hot chains had not shed what the first exchanges handed them; 2000 + 6000 steps: +0.015
        p0, ess = tempering.ladder_start(f.model, ps, betas, 256, np.random.default_rng(98))
        print("start: effective prior draws per rung %s" % np.round(ess))
        assert ess.min() > 20 * 256
        smp.run_mcmc(p0, 500, storechain=False)
        smp.reset()
        smp.run_mcmc(None, 1500)
        est = tempering.stepping_stone(smp.lnl_series(), betas, nwalkers=256)
        got, err_ss = est["ln_ratio"][0], est["ln_ratio_err"][0]
        print("stepping stone: ln(Z_1 / Z_0) = %.4f +- %.4f (thermodynamic %.4f), difference %.4f; rungs %s +- %s; swap fraction %s"
              % (got, err_ss, est["ln_ratio_ti"][0], got - ref, np.round(est["rungs"][0], 4), np.round(est["rungs_err"][0], 4),
                 np.round(smp.swap_fraction[0], 3)))
        assert abs(got - ref) <= 5 * math.sqrt(err_ss ** 2 + err_ref ** 2)
        assert err_ss <= 0.1
    finally:
        smp.close()


def test_sens_writes_the_tempered_evidence_beside_fr_stat(tmp_path, capsys):
    """python -m golemflavor_amd.sens --evidence-method stepping-stone on three scales and a short ladder: its own file, no fr_stat"""
    import json
    from golemflavor_amd import sens
    argv = ["--evidence-method", "stepping-stone", "--datadir", str(tmp_path), "--segments", "3", "--smearing", "0.1", "--on-nonunitary=-inf",
            "--temperatures", "3", "--beta-min", "0.01", "--swap-every", "4", "--tempered-steps", "48", "--tempered-walkers", "24"]
    assert sens.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    args = sens.parse_args(argv)
    f = sens.evidence_tempered_path(args)
    assert line["fr_evidence_tempered"] == f and line["evidence_method"] == "stepping-stone" and len(line["ln_z"]) == 3
    with np.load(f) as z:
        assert set(z.files) >= {"scales", "ln_z", "ln_z_err", "ln_ratio", "ln_ratio_ti", "swap_fraction", "nonunitary", "nonfinite_fraction", "betas"}
        assert z["ln_z"].shape == (3,) and np.all(np.isfinite(z["ln_z"])) and z["swap_fraction"].shape == (3, 3)
        assert np.array_equal(z["betas"], tempering.geometric_ladder(3, 0.01)) and np.array_equal(z["scales"], line["scales"])
    stat, llh_file = sens.output_paths(args)
    assert not os.path.exists(stat + ".npy") and not os.path.exists(llh_file + ".npy")
    assert sorted(os.listdir(os.path.dirname(f))) == [os.path.basename(f)]


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(golden, posts):
    f, ps = posts["s01"], posts["ps"]

    def refused(code, says, fns, betas, **kw):
        with pytest.raises(_lib.GolemHipError) as e:
            tempered(fns, betas, **kw).close()
        assert e.value.code == code and says in str(e.value), str(e.value)

    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, nps = Cf.notebook_paramsets(ang)
    for mode in ("SM_GAUSS", "PRIOR_ONLY"):
        with Model(compile_model(nps, mode, bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02)) as m:
            with pytest.raises(_lib.GolemHipError) as e:
                mcmc_utils.DeviceEnsembleSampler(24, len(nps), m, betas=[1.0, 0.0]).close()
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED and "flux-averaged BSM likelihood only" in str(e.value)
            with pytest.raises(_lib.GolemHipError) as e:
                m.lnprior_lnlike(np.zeros((1, len(nps))))
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED
    with Model(compile_model(ps, "BSM_GAUSS", **sens_kw(0.1))) as m:
        m.set_binned_measurement(a_measurement(len(BIN_EDGES) - 1, BIN_EDGES))
        refused(_lib.GF_ERR_UNSUPPORTED, "binned measurement", m, [1.0, 0.0])
    table = llh.TabulatedLikelihood.from_function(lambda fr: -np.sum((fr - 1 / 3) ** 2, axis=1), 8)
    with Model(compile_model(ps, "BSM_GAUSS", **sens_kw(0.1))) as m:
        m.set_table_likelihood(table)
        refused(_lib.GF_ERR_UNSUPPORTED, "tabulated likelihood", m, [1.0, 0.0])
    refused(_lib.GF_ERR_INVALID_ARG, "strictly decreasing", f, [1.0, 0.5, 0.5, 0.0])
    refused(_lib.GF_ERR_INVALID_ARG, "strictly decreasing", f, [1.0, 0.2, 0.5])
    refused(_lib.GF_ERR_INVALID_ARG, "betas[0]", f, [0.9, 0.5, 0.0])
    refused(_lib.GF_ERR_INVALID_ARG, "it is >= 0", f, [1.0, 0.5, -0.1])
    refused(_lib.GF_ERR_INVALID_ARG, "at most 64", f, list(np.linspace(1.0, 0.0, 65)))
    refused(_lib.GF_ERR_INVALID_ARG, "one for all groups, or one per group", [f, f], [1.0, 0.0], ngroups=3)
    with pytest.raises(ValueError, match="flux-averaged likelihood only"):
        mcmc_utils.DeviceEnsembleSampler(24, 12, f, betas=[1.0, 0.0], tabulated=True)
    # 64 rungs are a ladder
    tempered(f, list(np.linspace(1.0, 0.0, 64))).close()
    # a model that gains a table under a live tempered sampler: every entry point that evaluates refuses, the chain stays
    with Model(compile_model(ps, "BSM_GAUSS", **sens_kw(0.1))) as m:
        smp = tempered(m, [1.0, 0.2, 0.0], swap_every=2)
        smp.on_nonunitary = "-inf"
        try:
            p0 = prior_draws(ps, 3 * NW, np.random.default_rng(81)).reshape(3, NW, 12)
            smp.run_mcmc(p0, 4)
            kept = device_run(smp)["chain"]
            m.set_table_likelihood(table)
            for call in (lambda: smp.run_mcmc(None, 2), lambda: smp.run_mcmc(p0, 2), lambda: smp.lnl_series()):
                with pytest.raises(_lib.GolemHipError) as e:
                    call()
                assert e.value.code == _lib.GF_ERR_INVALID_ARG and "now carries a tabulated likelihood" in str(e.value)
            assert same_bits(device_run(smp)["chain"], kept) and smp.nstored == 4
        finally:
            smp.close()
    # a sampler that is not tempered has no ladder
    plain = mcmc_utils.DeviceEnsembleSampler(NW, 12, f)
    try:
        with pytest.raises(ValueError, match="not a tempered sampler"):
            plain.swap_fraction
        assert plain._L.gf_sampler_betas(plain._h, None, None, None, None) == _lib.GF_ERR_UNSUPPORTED
    finally:
        plain.close()
