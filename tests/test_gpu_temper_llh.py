"""GPU: the tempered ensemble sampler under the energy-resolved Gaussian likelihood and the tabulated flavour-plane
likelihood: gf_sampler_create_tempered_binned / _table, the binned and table instances of k_lnprior_lnl,
k_stretch_tempered and k_pt_series (csrc/gf_temper.hip).  The yardsticks are the flux-averaged tempered sampler's
(tests/test_gpu_temper.py, tests/test_gpu_temper_shapes.py), imported: `Model.lnprob` for the split evaluation, the numpy stretch move
on the sampler's Philox stream fed T = lp + beta lnl from `Model.lnprior_lnlike`, the numpy restatement of the round, the host build of
csrc/gf_temper.hpp, a direct average over prior draws for the evidence; and beside them `TabulatedLikelihood.lnl` and
tests/binned_ref.py for the two likelihoods themselves.  Every comparison is bit for bit but three: lnprior against the oracle
(check_split's REL), the binned lnl against tests/binned_ref.py (binned_bound, as tests/test_gpu_binned.py), and the evidence.
profiles/tempering_llh/README.txt has the instances each test executes."""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest

from binned_ref import binned_bound, binned_lnl_host
from common import BIN_EDGES
from golemflavor_amd import _lib, llh, tempering
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model
from stretch_ref import reference_stretch
from test_gpu_binned_sampler import a_measurement, assert_same_run, bulk, device_run, same_bits
from test_gpu_table_sampler import forced_lpw, stripes, striped_table, surface
from test_gpu_temper import (NW, check_split, failing_lnprob, failing_rows, numpy_T, numpy_tempered, prior_draws, sens_kw, sens_sets,
                             series_against_host, state_holds_the_formula)
from test_gpu_temper_shapes import BLOCK, OEU_ANGLES, TWO_BLOCKS, blocks_per_chain, check_launch, second_block_moves, swap_counts_are, width_model

pytestmark = pytest.mark.gpu

KINDS = ("table", "binned")
BETAS = [1.0, 0.3, 0.0]
K = len(BIN_EDGES) - 1
OFFSET = -320.0                     # compile_model's default, which every model here has


# ---- the posteriors --------------------------------------------------------------------------------------------------------------------
def holed_table(N, seed):
    """tests/test_gpu_table_sampler.py's surface with its stripes -- a quarter of the triangle -- at -inf"""
    return surface(N, seed, hole=stripes)


def attach(model, kind, seed, N=24, smearing=0.02):
    """the likelihood of `kind` on a flux-averaged model: a holed table of side N, or a measurement per energy bin; returns it"""
    if kind == "table":
        what = holed_table(N, seed)
        model.set_table_likelihood(what)
    else:
        what = a_measurement(K, BIN_EDGES, seed=seed, smearing=smearing)
        model.set_binned_measurement(what)
    return what


def sens_model(texture=Texture.OET, smearing=0.1):
    return Model(compile_model(sens_sets()[1], "BSM_GAUSS", **sens_kw(smearing, texture)))


def tempered(kind, fns, betas, nw=NW, seed=5, swap_every=0, ngroups=None, stream_ids=None, ndim=12):
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, fns, seed=seed, betas=betas, swap_every=swap_every, ngroups=ngroups, stream_ids=stream_ids,
                                           energy_resolved=kind == "binned", tabulated=kind == "table")
    smp.on_nonunitary = "-inf"
    return smp


class forced_split_lpw:
    """GF_TEMPER_LPW for the split evaluations inside (None: unset), read by every call"""

    def __init__(self, lpw):
        self.lpw = lpw

    def __enter__(self):
        self.old = os.environ.pop("GF_TEMPER_LPW", None)
        if self.lpw is not None:
            os.environ["GF_TEMPER_LPW"] = str(self.lpw)

    def __exit__(self, *exc):
        os.environ.pop("GF_TEMPER_LPW", None)
        if self.old is not None:
            os.environ["GF_TEMPER_LPW"] = self.old


@pytest.fixture(scope="module")
def pair():
    """per kind, two 12-column sens models (textures OET and OUT) that differ in their likelihood too: tables of sides 24 and 40, two
    measurements.  Made once, read-only."""
    out, models = {}, []
    for kind in KINDS:
        ms = [sens_model(Texture.OET), sens_model(Texture.OUT)]
        attach(ms[0], kind, 61, N=24)
        attach(ms[1], kind, 62, N=40)
        out[kind] = ms
        models += ms
    out["ps"] = sens_sets()[1]
    yield out
    for m in models:
        m.close()


@pytest.fixture(scope="module")
def failing():
    """per kind, the OEU failing-region model of tests/test_gpu_temper.py with a striped table / a measurement attached"""
    out, fns = {}, []
    for kind in KINDS:
        f, ps = failing_lnprob()
        if kind == "table":
            f.model.set_table_likelihood(striped_table(48))
        else:
            attach(f.model, kind, 63, smearing=0.3)
        out[kind], out["ps"] = f.model, ps
        fns.append(f)
    yield out
    for f in fns:
        f.close()


# ---- 1. lnprior and lnl apart ---------------------------------------------------------------------------------------------------------------
NROWS = 2300                        # nine blocks of 256 rows, the last one partial (at 4 and 16 lanes per row: 36 and 144 blocks)


def outside_rows(ps, n, rng):
    """prior draws moved outside the box in one column each, the columns in turn, below and above the range alternately"""
    far = prior_draws(ps, n, rng)
    for i in range(n):
        c = i % len(ps)
        lo, hi = ps[c].ranges
        far[i, c] = lo - (hi - lo) * 0.01 * (1 + i % 7) if (i // len(ps)) % 2 else hi + (hi - lo) * 0.01 * (1 + i % 5)
    return far


def split_case(which):
    """(flux-averaged Model, paramset, the oracle's model keywords, NROWS rows, closer): prior draws, rows outside the box, and rows
    across the top of the scale range, where the textures used here stop being unitary"""
    rng = np.random.default_rng({"sens": 401, "w7": 407, "w11": 411, "oeu": 413}[which])
    if which == "oeu":
        f, ps = failing_lnprob()
        okw = dict(texture="OEU", dimension=6, binning=BIN_EDGES, source_ratio=(1 / 3, 2 / 3, 0.),
                   bestfit_fr=fr_utils.angles_to_fr(fr_utils.fr_to_angles((1, 1, 1))), smearing=0.3)
        nfar = 252
        rows = [prior_draws(ps, 1024, rng), outside_rows(ps, nfar, rng), failing_rows(ps, NROWS - 1024 - nfar, rng)]
        return f.model, ps, okw, np.concatenate(rows), nfar, f.close
    if which == "sens":
        m, ps = sens_model(), sens_sets()[1]
        okw = {**sens_kw(0.1), "texture": "OET"}
    else:
        m, ps, okw = width_model(int(which[1:]))
    width = len(ps)
    nfar = 21 * width
    top = prior_draws(ps, NROWS - 1200 - nfar, rng)
    lo, hi = ps[width - 1].ranges
    top[:, -1] = rng.uniform(hi - 0.25 * (hi - lo), hi, len(top))
    if which == "w11":
        top[:, 6:10] = OEU_ANGLES
    return m, ps, okw, np.concatenate([prior_draws(ps, 1200, rng), outside_rows(ps, nfar, rng), top]), nfar, m.close


@pytest.mark.parametrize("which", ["sens", "w7", "w11", "oeu"])
@pytest.mark.parametrize("kind", KINDS)
def test_split_evaluation(oracle, kind, which):
    """2 300 rows through the binned / table instance of k_lnprior_lnl at the widths 12, 7 and 11 and through the failing region:
    status, lp + lnl and lp against `Model.lnprob`, the same model before the likelihood was attached and the oracle; lnl against the
    likelihood's own restatement.  The table instance at 1, 4 and 16 lanes per row gives the same bits."""
    m, ps, okw, th, nfar, close = split_case(which)
    try:
        assert len(th) == NROWS and NROWS % BLOCK != 0 and NROWS > BLOCK
        om = oracle.make_model(ps, "BSM_GAUSS", **okw)
        lp0, _, st0 = m.lnprior_lnlike(th)                                  # the flux-averaged model: the same prior, the same verdicts
        fr_bins = m.propagate_bins(th, want_status=False)
        what = attach(m, kind, 71)
        lp, lnl, st = check_split(oracle, m, om, th, "%s, %s" % (kind, which))
        assert np.array_equal(st, st0) and same_bits(lp, lp0)
        ok, bad, out = st == _lib.GF_ST_OK, st == _lib.GF_ST_NON_UNITARY, st == _lib.GF_ST_OUT_OF_PRIOR
        assert np.array_equal(np.isnan(lnl), bad), "lnl is NaN on other rows than the non-unitary ones"
        first_far = 1024 if which == "oeu" else 1200
        assert np.all(out[first_far:first_far + nfar]) and out.sum() == nfar, out.sum()
        print("%s, %s: %d ok, %d non-unitary, %d outside" % (kind, which, ok.sum(), bad.sum(), out.sum()))
        assert ok.sum() > 100
        if which == "oeu":
            assert bad.sum() > 100
        if kind == "table":
            _, fr, _ = m.lnprob(th, want_fr=True, want_status=True)
            assert same_bits(lnl[ok], what.lnl(fr[ok]))
            print("%d OK rows in a hole of the table" % np.sum(lnl[ok] == -np.inf))
            assert np.sum(lnl[ok] == -np.inf) > 0 and np.sum(np.isfinite(lnl[ok])) > 0
            for lpw in (1, 4, 16):
                with forced_split_lpw(lpw):
                    again = m.lnprior_lnlike(th)
                assert same_bits(again[0], lp) and same_bits(again[1], lnl) and np.array_equal(again[2], st), lpw
        else:
            # lnl = the terms' sum + offset: tests/test_gpu_binned.py's bound without the prior's add (K + 4 roundings' worth of the sum
            # of the magnitudes; its docstring has the count)
            want, terms = binned_lnl_host(fr_bins[ok], what, OFFSET, return_terms=True)
            bound = binned_bound(terms, np.zeros(len(want)), OFFSET)
            fin = np.isfinite(want)
            err = np.abs(lnl[ok][fin] - want[fin])
            print("binned lnl: %d finite rows, worst |diff| / bound = %.3f" % (fin.sum(), np.max(err / bound[fin])))
            assert fin.sum() > 100 and np.all(err <= bound[fin]) and np.array_equal(lnl[ok][~fin], want[~fin])
    finally:
        close()


# ---- 2. betas = [1] is the untempered sampler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_beta_one_is_the_untempered_sampler(pair, kind):
    """two groups whose models differ in texture and in table (sides 24 and 40) / measurement, 40 steps at thin 3 -- graph replays and
    eager steps -- against the multi-model table / binned sampler on the same seed and stream ids"""
    models = pair[kind]
    p0 = np.stack([prior_draws(pair["ps"], NW, np.random.default_rng(s)) for s in (41, 42)])
    ids = (7, 2)
    a = tempered(kind, models, [1.0], seed=17, ngroups=2, stream_ids=ids)
    b = mcmc_utils.DeviceEnsembleSampler(NW, 12, models, seed=17, stream_ids=ids, energy_resolved=kind == "binned", tabulated=kind == "table")
    b.on_nonunitary = "-inf"
    try:
        assert a.nchains == 2 and np.array_equal(a.cold_chains, [0, 1]) and a.launch_shape()["shape"] == "grid"
        a.run_mcmc(p0, 40, thin=3)
        b.run_mcmc(p0, 40, thin=3)
        ra, rb = device_run(a), device_run(b)
        assert ra["chain"].shape == (2, 14, NW, 12)
        assert_same_run(ra, rb, "%s, betas = [1] against the multi-model sampler" % kind)
        assert a.nonunitary_proposals == b.nonunitary_proposals
        # ... whose stored lnprob is the bulk lnprob of the stored sample
        for ch in range(2):
            assert same_bits(ra["lnp_chain"][ch].reshape(-1), bulk(models[ch], ra["chain"][ch].reshape(-1, 12)))
    finally:
        a.close()
        b.close()


# ---- 3. the tempered half-step against numpy ----------------------------------------------------------------------------------------------------
_REFS = {}


def shared(key, make):
    """a numpy run, computed by the first test that asks for it and read-only from then on"""
    if key not in _REFS:
        ref = make()
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def half_step_run(oracle, kind, model, p0, nsteps, seed, lpw, key, thin=1, stream_ids=None, ndim=12):
    """3 chains at BETAS of one model against reference_stretch with numpy_T; returns (sampler, what it left, the reference)"""
    with forced_lpw(lpw):
        smp = tempered(kind, model, BETAS, nw=p0.shape[1], seed=seed, stream_ids=stream_ids, ndim=ndim)
        try:
            smp.run_mcmc(p0, nsteps, thin=thin)
            check_launch(smp, lpw)
            ref = shared(key, lambda: reference_stretch(oracle, [(model, b) for b in BETAS], p0, nsteps, seed, lnprob=numpy_T, full=True, thin=thin,
                                                        stream_ids=stream_ids))
            got = device_run(smp)
            assert_same_run(got, ref, "%s, betas %s, %d walkers, %d lanes per walker" % (key, BETAS, p0.shape[1], lpw))
            # no sample the reference would have died on is in any chain
            st = model.lnprior_lnlike(got["chain"].reshape(-1, ndim))[2]
            assert not np.any(st[np.isfinite(got["lnp_chain"].reshape(-1))] == _lib.GF_ST_NON_UNITARY)
            return smp, got, ref
        except BaseException:
            smp.close()
            raise


@pytest.mark.parametrize("lpw", [1, 2, 4, 16])
def test_half_step_under_a_holed_table(oracle, pair, lpw):
    """24 walkers, 20 steps; the beta = 0 chain stores samples inside the table's holes: T = lp there, a legal sample of the prior"""
    m = pair["table"][0]
    p0 = prior_draws(pair["ps"], 3 * NW, np.random.default_rng(51)).reshape(3, NW, 12)
    smp, got, _ = half_step_run(oracle, "table", m, p0, 20, 23, lpw, "holed table")
    try:
        lp, lnl, st = m.lnprior_lnlike(got["chain"][2].reshape(-1, 12))
        in_hole = (st == _lib.GF_ST_OK) & (lnl == -np.inf)
        print("the prior chain stores %d samples in a hole" % in_hole.sum())
        assert in_hole.sum() > 0 and np.all(np.isfinite(got["lnp_chain"][2].reshape(-1)[in_hole]))
        assert same_bits(got["lnp_chain"][2].reshape(-1)[in_hole], lp[in_hole])
        # at every beta > 0 a sample in a hole is one that never moved
        for ch in (0, 1):
            lnl = m.lnprior_lnlike(got["chain"][ch].reshape(-1, 12))[1]
            assert np.all(got["lnp_chain"][ch].reshape(-1)[lnl == -np.inf] == -np.inf)
    finally:
        smp.close()


def test_half_step_under_a_binned_measurement(oracle, pair):
    m = pair["binned"][0]
    p0 = prior_draws(pair["ps"], 3 * NW, np.random.default_rng(51)).reshape(3, NW, 12)
    half_step_run(oracle, "binned", m, p0, 20, 23, 1, "binned")[0].close()


@pytest.mark.parametrize("kind", KINDS)
def test_half_step_through_the_failing_region(oracle, failing, kind):
    """texture OEU where the reference raises: the verdict, parking and settlement apply at every beta under both likelihoods"""
    m = failing[kind]
    p0 = failing_rows(failing["ps"], 3 * NW, np.random.default_rng(52)).reshape(3, NW, 12)
    smp = half_step_run(oracle, kind, m, p0, 20, 29, 1, "failing region, " + kind)[0]
    try:
        print("parked %d, non-unitary %d" % (smp.parked_proposals, smp.nonunitary_proposals))
        assert smp.parked_proposals > 0 and smp.nonunitary_proposals > 0
    finally:
        smp.close()


@pytest.mark.parametrize("kind, lpw, nw", [("table",) + s for s in TWO_BLOCKS] + [("binned", 1, 518)])
def test_two_blocks_per_chain(oracle, pair, kind, lpw, nw):
    """6 steps at thin 2 on streams (11, 3, 40): two blocks per chain, the second one partly filled"""
    assert blocks_per_chain(nw, lpw) >= 2 and 0 < nw // 2 * lpw - BLOCK <= 80
    m = pair[kind][0]
    ids = (11, 3, 40)
    p0 = prior_draws(pair["ps"], 3 * nw, np.random.default_rng(100 + lpw)).reshape(3, nw, 12)
    smp, got, ref = half_step_run(oracle, kind, m, p0, 6, 23, lpw, ("two blocks", kind, lpw), thin=2, stream_ids=ids)
    smp.close()
    assert got["chain"].shape == (3, 3, nw, 12)
    print("moves of the second block's walkers: %d" % second_block_moves(ref, nw, lpw))
    assert second_block_moves(ref, nw, lpw) > 0


@pytest.mark.parametrize("kind, width, lpw", [("table", 7, 4), ("table", 11, 16), ("binned", 7, 1), ("binned", 11, 1)])
def test_half_step_at_widths_7_and_11(oracle, kind, width, lpw):
    """the <7> and <0> instances of both likelihoods at the smallest legal ensemble (14 and 22 walkers), 20 steps, started where
    texture OEU fails (at 11 columns every walker carries OEU's angles): they park rows of their own width"""
    nw = 2 * width
    m, ps, _ = width_model(width)
    with m:
        attach(m, kind, 81)
        rng = np.random.default_rng(330 + width)
        p0 = prior_draws(ps, 3 * nw, rng)
        p0[:, -1] = rng.uniform(-40.0, -30.0, len(p0))
        if width == 11:
            p0[:, 6:10] = OEU_ANGLES
        smp = half_step_run(oracle, kind, m, p0.reshape(3, nw, width), 20, 73, lpw, ("width", kind, width), ndim=width)[0]
        try:
            print("parked %d, non-unitary %d" % (smp.parked_proposals, smp.nonunitary_proposals))
            assert smp.parked_proposals > 0 and smp.nonunitary_proposals > 0
        finally:
            smp.close()


# ---- 4. replica exchange against the numpy restatement of the round -------------------------------------------------------------------------
@pytest.mark.parametrize("ntemps, swap_every, nsteps", [(4, 3, 20), (3, 3, 20), (4, 1, 6), (3, 1, 6)])
@pytest.mark.parametrize("kind", KINDS)
def test_swaps_against_numpy(oracle, pair, kind, ntemps, swap_every, nsteps):
    """two groups with different models; chain, state and swap counters bit for bit; one walker starts outside the support and stays
    there: its pairs are skipped and not counted"""
    models = pair[kind]
    betas = [1.0, 0.3, 0.05, 0.0] if ntemps == 4 else [1.0, 0.3, 0.0]
    nch = 2 * ntemps
    p0 = prior_draws(pair["ps"], nch * NW, np.random.default_rng(61)).reshape(nch, NW, 12)
    p0[1, 3, 0] = 1e6                                                     # group 0, rung 1, walker 3: no proposal from there is in the box
    ids = tuple(range(10, 10 + 3 * nch, 3))
    smp = tempered(kind, models, betas, seed=37, swap_every=swap_every, ngroups=2, stream_ids=ids)
    try:
        smp.run_mcmc(p0, nsteps)
        ref = numpy_tempered(oracle, models, betas, p0, nsteps, 37, swap_every, ids)
        got = device_run(smp)
        assert_same_run(got, ref, "%s, %d rungs, a round every %d steps" % (kind, ntemps, swap_every))
        prop, acc = swap_counts_are(smp, ref)
        assert acc.sum() > 0 and np.all(prop[:, -1] == 0)
        assert got["lnp"][1, 3] == -np.inf and got["pos"][1, 3, 0] == 1e6
        state_holds_the_formula(smp, models, betas, got)
        frac = smp.swap_fraction
        assert frac.shape == (2, ntemps - 1) and np.all((frac[np.isfinite(frac)] >= 0) & (frac[np.isfinite(frac)] <= 1))
    finally:
        smp.close()


# ---- 5. the series kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw, nsteps", [(24, 1), (24, 7), (258, 1), (258, 7)])
@pytest.mark.parametrize("kind", KINDS)
def test_series_against_the_host_build(pair, kind, nw, nsteps):
    """all five outputs against the host build of gf_temper.hpp fed lnprior_lnlike of the stored chain, at one and two passes of the
    kernel's walker loop; rung 1 starts outside the support and stays there: count 0, sums 0, max -inf"""
    m = pair[kind][0]
    betas = [1.0, 0.4, 0.1, 0.0]
    p0 = prior_draws(pair["ps"], 4 * nw, np.random.default_rng(71)).reshape(4, nw, 12)
    p0[1, :, 0] = 1e6
    smp = tempered(kind, m, betas, nw=nw, seed=53, swap_every=2)
    try:
        smp.run_mcmc(p0, nsteps)
        ser, lnl = series_against_host(smp, [m], betas)
        assert ser.shape == (4, nsteps, 5) and lnl.shape == (4, nsteps, nw)
        assert np.all(ser[1, :, 0] == 0) and np.all(ser[1, :, 1] == 0) and np.all(ser[1, :, 2] == -np.inf) and np.all(ser[1, :, 3:] == 0)
        assert np.all(ser[0, :, 0] > 0)
        if kind == "table" and nw == 258:
            assert np.any(ser[3, :, 0] < nw)                              # the prior chain holds samples in the holes
        assert same_bits(smp.lnlikelihood(), lnl.transpose(0, 2, 1))
    finally:
        smp.close()


# ---- 6. the evidence against a direct average ----------------------------------------------------------------------------------------------------
def evidence_likelihood(kind, bf):
    """the two likelihoods at the information of the flux-averaged Gaussian of smearing 0.1 around the injected composition: its table
    (side 64), and a measurement per energy bin at the equal-information widths"""
    if kind == "table":
        return llh.TabulatedLikelihood.from_gaussian(bf, 0.1, 64)
    return llh.BinnedMeasurement(np.tile(np.asarray(bf, dtype=np.float64), (K, 1)), 0.1, binning=BIN_EDGES)


@pytest.mark.parametrize("kind", KINDS)
def test_stepping_stone_evidence_against_a_direct_average(kind):
    """tests/test_gpu_temper.py's evidence test under the two likelihoods.  Reference: ln mean_prior(L) from 2^20 prior draws through
    Model.lnprior_lnlike of the same model, its standard error from the draws.  Tempered run: geometric_ladder(8, 1e-3), 256 walkers, a
    round every 8 steps, 500 burn-in + 1500 stored steps from `ladder_start`.  Pass iff |ln_ratio - reference| <= 5 sqrt(err_ss^2 +
    err_ref^2) and err_ss <= 0.1.  Preconditions on the reference alone: fewer than 1e-3 of the draws not OK, err_ref <= 0.01.
    profiles/tempering_llh/README.txt has the measured figures."""
    ps = sens_sets()[1]
    m = sens_model()
    try:
        kw = sens_kw(0.1)
        if kind == "table":
            m.set_table_likelihood(evidence_likelihood(kind, kw["bestfit_fr"]))
        else:
            m.set_binned_measurement(evidence_likelihood(kind, kw["bestfit_fr"]))
        rng = np.random.default_rng(2024)
        th = prior_draws(ps, 1 << 20, rng)
        lp, lnl, st = m.lnprior_lnlike(th)
        bad = st != _lib.GF_ST_OK
        print("%s: %d of 2^20 prior draws are not OK, %d have a non-finite lnl" % (kind, bad.sum(), np.sum(~np.isfinite(lnl))))
        assert bad.sum() < 1e-3 * len(st)
        top = lnl[~bad].max()
        with np.errstate(invalid="ignore"):
            w = np.where(bad, 0.0, np.exp(lnl - top))
        ref = top + math.log(w.mean())
        err_ref = float(w.std(ddof=1) / math.sqrt(len(w)) / w.mean())
        print("direct average over 2^20 prior draws: ln mean L = %.4f, relative standard error %.4f" % (ref, err_ref))
        assert err_ref <= 0.01
        betas = tempering.geometric_ladder(8, 1e-3)
        smp = tempered(kind, m, betas, nw=256, seed=97, swap_every=8)
        try:
            p0, ess = tempering.ladder_start(m, ps, betas, 256, np.random.default_rng(98))
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
    finally:
        m.close()


# ---- 7. models that change under a live sampler ---------------------------------------------------------------------------------------------------
def test_a_table_replaced_between_two_runs_is_the_one_the_next_run_samples(oracle):
    """12 steps under a table of side 24, then the model's table is replaced by one of side 40 (the table moves) and the positions are
    handed to run_mcmc again: the start, the half-steps, the rounds' re-evaluation and lnl_series() all read the new table -- the run
    equals the numpy run on the model as it is now, the stored T of the beta = 1 chain is the bulk lnprob of the stored sample, and the
    series is the host build's on `lnprior_lnlike` of now."""
    ps = sens_sets()[1]
    betas = [1.0, 0.3, 0.0]
    with sens_model() as m:
        m.set_table_likelihood(holed_table(24, 91))
        p0 = prior_draws(ps, 3 * NW, np.random.default_rng(92)).reshape(3, NW, 12)
        smp = tempered("table", m, betas, seed=59, swap_every=2)
        try:
            smp.run_mcmc(p0, 12)
            first = device_run(smp)
            old = m.lnprior_lnlike(first["pos"][0])[1]
            m.set_table_likelihood(surface(40, 93, hole=stripes))
            assert m.table_nside == 40 and np.sum(m.lnprior_lnlike(first["pos"][0])[1] != old) > NW // 2, "the replacement changes nothing"
            smp.reset()
            smp.run_mcmc(first["pos"], 12)
            # the sampler counts its steps and rounds since creation: the numpy run starts at iteration 12 too
            ref = numpy_tempered_from(oracle, [m], betas, first["pos"], 12, 59, 2, iteration0=12)
            got = device_run(smp)
            assert_same_run(got, ref, "after the replacement")
            swap_counts_are(smp, ref)
            assert ref["counts"][:, 1].sum() > 0
            assert same_bits(got["lnp_chain"][0].reshape(-1), bulk(m, got["chain"][0].reshape(-1, 12)))
            state_holds_the_formula(smp, [m], betas, got)
            series_against_host(smp, [m], betas)
        finally:
            smp.close()


def numpy_tempered_from(oracle, models, betas, p0, nsteps, seed, swap_every, iteration0):
    """numpy_tempered for a run that is not the sampler's first: the steps and the rounds are counted from `iteration0`.  Restated here,
    since tests/test_gpu_temper.py's counts from 0."""
    import temper_harness as TH
    nt = len(betas)
    nch = p0.shape[0]
    oms = [(models[ch // nt], betas[ch % nt]) for ch in range(nch)]
    pos, lnp, it = np.array(p0), None, iteration0
    chain, lnp_chain = [], []
    nacc = np.zeros(p0.shape[:2], dtype=int)
    counts = np.zeros((nch, 2), dtype=np.int64)
    while it < iteration0 + nsteps:
        seg = min(iteration0 + nsteps - it, swap_every - it % swap_every)
        r = reference_stretch(oracle, oms, pos, seg, seed, lnprob=numpy_T, full=True, iteration0=it, lnp0=lnp)
        chain.append(r["chain"])
        lnp_chain.append(r["lnp_chain"])
        pos, lnp = r["pos"], r["lnp"]
        nacc += r["nacc"]
        it += seg
        if it % swap_every == 0:
            ev = [mm.lnprior_lnlike(np.ascontiguousarray(pos[ch])) for ch, (mm, _) in enumerate(oms)]
            TH.swap_round(oracle, seed, it // swap_every - 1, betas, pos, lnp, np.stack([e[0] for e in ev]), np.stack([e[1] for e in ev]), counts)
    return {"chain": np.concatenate(chain, axis=1), "lnp_chain": np.concatenate(lnp_chain, axis=1), "pos": pos, "lnp": lnp, "nacc": nacc,
            "counts": counts}


def test_a_model_whose_kind_changes_under_a_live_sampler_is_refused():
    """A flux-averaged tempered sampler whose model gains a measurement: run_mcmc and lnl_series() are refused, the chain stays.  (A
    model with a table or a measurement cannot change its kind -- the model refuses the other likelihood, asserted here -- so the
    tempered table and binned samplers go on running.)"""
    ps = sens_sets()[1]
    p0 = prior_draws(ps, 3 * NW, np.random.default_rng(81)).reshape(3, NW, 12)
    with sens_model() as m:
        smp = mcmc_utils.DeviceEnsembleSampler(NW, 12, m, seed=5, betas=BETAS, swap_every=2)
        smp.on_nonunitary = "-inf"
        try:
            smp.run_mcmc(p0, 4)
            kept = device_run(smp)["chain"]
            m.set_binned_measurement(a_measurement(K, BIN_EDGES))
            for call in (lambda: smp.run_mcmc(None, 2), lambda: smp.run_mcmc(p0, 2), lambda: smp.lnl_series()):
                with pytest.raises(_lib.GolemHipError) as e:
                    call()
                assert e.value.code == _lib.GF_ERR_INVALID_ARG and "now carries a binned measurement" in str(e.value)
            assert same_bits(device_run(smp)["chain"], kept) and smp.nstored == 4
        finally:
            smp.close()
    for kind in KINDS:
        with sens_model() as m:
            attach(m, kind, 95)
            smp = tempered(kind, m, BETAS, swap_every=2)
            try:
                smp.run_mcmc(p0, 4)
                kept = device_run(smp)["chain"]
                with pytest.raises(_lib.GolemHipError) as e:
                    attach(m, "binned" if kind == "table" else "table", 96)
                assert e.value.code == _lib.GF_ERR_UNSUPPORTED
                smp.run_mcmc(None, 2)
                assert smp.nstored == 6 and same_bits(device_run(smp)["chain"][:, :4], kept) and smp.lnl_series().shape == (3, 6, 5)
            finally:
                smp.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pair):
    L = _lib.lib()
    table, binned = pair["table"][0], pair["binned"][0]
    betas = (C.c_double * 2)(1.0, 0.0)

    def create(name, *models, ngroups=None):
        h = C.c_void_p()
        rc = getattr(L, name)((C.c_void_p * len(models))(*[m._h for m in models]), len(models), ngroups or len(models), 2, betas, NW, 5, 2.0, 0,
                              C.byref(h))
        assert not h.value
        return rc, L.gf_last_hip_error()

    with sens_model() as flux:
        # a flux-averaged model, the other kind, a mixed list: gf_sampler_create_table's / _binned's code and wording
        for name, own, other, none in (("gf_sampler_create_tempered_table", table, binned, b"carries no tabulated likelihood"),
                                       ("gf_sampler_create_tempered_binned", binned, table, b"carries no binned measurement")):
            rc, msg = create(name, flux)
            assert rc == _lib.GF_ERR_INVALID_ARG and b"model 0 " + none in msg, msg
            rc, msg = create(name, own, flux)
            assert rc == _lib.GF_ERR_INVALID_ARG and b"model 1 " + none in msg, msg
            rc, msg = create(name, own, other)
            assert rc != _lib.GF_OK and b"model 1 carries" in msg, msg
        rc, msg = create("gf_sampler_create_tempered_table", binned)
        assert rc == _lib.GF_ERR_INVALID_ARG and b"model 0 carries no tabulated likelihood" in msg
        rc, msg = create("gf_sampler_create_tempered_binned", table)
        assert rc == _lib.GF_ERR_UNSUPPORTED and b"model 0 carries a tabulated likelihood" in msg
        # the ladder's rules are the flux-averaged entry point's
        rc, msg = create("gf_sampler_create_tempered_table", table, table, ngroups=3)
        assert rc == _lib.GF_ERR_INVALID_ARG and b"one for all groups, or one per group" in msg
        # the plain tempered constructor still refuses both
        for m, says in ((binned, b"binned measurement"), (table, b"tabulated likelihood")):
            rc, msg = create("gf_sampler_create_tempered", m)
            assert rc == _lib.GF_ERR_UNSUPPORTED and says in msg and b"flux-averaged BSM likelihood only" in msg
        # the keywords: a posterior that does not carry the likelihood, and both at once
        for kw, m, says in ((dict(tabulated=True), flux, "posterior 0 carries the flux-averaged likelihood only"),
                            (dict(tabulated=True), binned, "posterior 0 carries a binned measurement"),
                            (dict(energy_resolved=True), flux, "posterior 0 carries the flux-averaged likelihood only"),
                            (dict(energy_resolved=True), table, "posterior 0 carries a tabulated likelihood"),
                            (dict(energy_resolved=True, tabulated=True), table, "not both")):
            with pytest.raises(ValueError, match=says):
                mcmc_utils.DeviceEnsembleSampler(NW, 12, m, betas=[1.0, 0.0], **kw)
        with pytest.raises(ValueError, match="posterior 1 carries the flux-averaged likelihood only"):
            mcmc_utils.DeviceEnsembleSampler(NW, 12, [table, flux], betas=[1.0, 0.0], tabulated=True)
        for m in (table, binned):
            with pytest.raises(_lib.GolemHipError) as e:
                mcmc_utils.DeviceEnsembleSampler(NW, 12, m, betas=[1.0, 0.0])
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED


# ---- 9. the scan, end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_evidence_scan_tempered_end_to_end(kind):
    """three scales as the groups of one tempered sampler of the likelihood, a ladder of three rungs and the prior's, 24 walkers, 48 steps"""
    args = argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=Texture.OET, binning=BIN_EDGES, smearing=0.1,
                              seed=3)
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    what = evidence_likelihood(kind, bf)
    res = tempering.evidence_scan_tempered(args, asimov, ps, [-52.0, -47.0, -42.0], ntemps=3, beta_min=0.01, swap_every=4, nwalkers=24, burnin=16,
                                           nsteps=48, on_nonunitary="-inf", **{kind: what})
    print("%s: ln Z %s +- %s, swap fraction\n%s" % (kind, res["ln_z"], res["ln_z_err"], res["swap_fraction"]))
    assert res["ln_z"].shape == (3,) and np.all(np.isfinite(res["ln_z"])) and res["swap_fraction"].shape == (3, 3)
    assert np.array_equal(res["betas"], tempering.geometric_ladder(3, 0.01)) and res["start_ess"].shape == (3, 4)
