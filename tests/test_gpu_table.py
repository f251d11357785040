"""GPU: the tabulated flavour-plane likelihood (csrc/gf_table.hip, the MODE_BSM_TABLE instance of proposal_lnprob) -- the
bulk kernel bit for bit against the prior sum plus the host build of csrc/gf_table.hpp on the composition the same call returned, past one
pass of the grid, the nested sampler and the maximiser against the bulk kernel, a Gaussian table against the Gaussian, the reweight path,
the refusals and the command line.

The rows are test_gpu_bulk_passes.py's base block (4099 seeded rows, an eighth outside the box, one NaN row, one +inf row) on an OEU
model whose scale is uniform over its whole range, so that rows the reference would raise on and arbitrated rows occur."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import table_harness as TH
from common import BIN_EDGES, rel_err
from golemflavor_amd import _lib, llh, nested
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import profile_llh as P
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import GF_LAYOUT_AOS, GF_LAYOUT_SOA, Model
from test_gpu_bulk_passes import PERIOD, base_block, batch_rows, launch_rows
from test_gpu_cube_runs import check_dead_points
from test_gpu_parity import REL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "table_sens.npz")
OFFSET = -320.0
SMEARING = 0.02
BF = (1 / 3, 1 / 3, 1 / 3)
OK, OUT, NONUNI, STNAN = _lib.GF_ST_OK, _lib.GF_ST_OUT_OF_PRIOR, _lib.GF_ST_NON_UNITARY, _lib.GF_ST_NAN


def paramset_of(width):
    return Cf.texture_paramset(6) if width == 7 else Cf.fr_paramsets(6, (0.4444, 0.0))[1]


def open_model(width):
    return Model(compile_model(paramset_of(width), "BSM_GAUSS", texture=Texture.OEU, dimension=6, binning=BIN_EDGES, source_ratio=(0., 1., 0.),
                               bestfit_fr=BF, smearing=SMEARING))


def random_table(N, seed):
    return llh.TabulatedLikelihood(np.random.default_rng(seed).uniform(-50.0, 5.0, llh.TabulatedLikelihood.node_count(N)))


def holed_table(N, seed):
    """-inf wherever fr_e > 0.45 or fr_mu < 0.08: a region, not single nodes"""
    t = random_table(N, seed)
    fr = t.node_fr()
    v = t.values.copy()
    v[(fr[:, 0] > 0.45) | (fr[:, 1] < 0.08)] = -np.inf
    return llh.TabulatedLikelihood(v)


_CASES = {}


def case(width):
    """Once per session and never modified: the base block, the Gaussian model's (lnprob, fr, status) on it, and the prior sum as the
    all-zero table gives it, with and without a status array."""
    if width in _CASES:
        return _CASES[width]
    ps = paramset_of(width)
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    base, rows = base_block(ps, PERIOD, scale=(len(ps) - 1, lo, hi))      # test_gpu_bulk_passes.py's own blocks (oeu7, oeu12)
    with open_model(width) as g:
        glp, gfr, gst = g.lnprob(base, want_fr=True, want_status=True)
    with open_model(width) as z:
        z.set_table_likelihood(np.zeros(3))
        assert z.table_nside == 1
        lp0, fr0, st0 = z.lnprob(base, want_fr=True, want_status=True)
        lp0_bare = z.lnprob(base, want_status=False)
    c = dict(ps=ps, base=base, rows=rows, glp=glp, gfr=gfr, gst=gst, lp0=lp0, fr0=fr0, st0=st0, lp0_bare=lp0_bare)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[width] = c
    return c


# ---- 1. the bulk kernel, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [7, 12])
def test_zero_table_gives_the_prior_sum(oracle, width):
    """lnprob under the all-zero table is lp + 0.0: the prior sum itself.  It is held to the oracle's lnprior with the suite's bar, and the
    composition and the status are the Gaussian model's."""
    c = case(width)
    st = c["st0"]
    assert np.array_equal(st, c["gst"]) and TH.same_values(c["fr0"], c["gfr"])
    assert {int(v) for v in np.unique(st)} >= {OK, OUT, NONUNI}
    ok = st == OK
    assert ok.sum() > 0.4 * PERIOD and 0.1 < np.mean(st == NONUNI) < 0.3
    assert (st == OUT).sum() == PERIOD // 8 + 2                            # the rows outside the box, the NaN row and the +inf row
    om = oracle.make_model(c["ps"], "PRIOR_ONLY")
    want = np.array([oracle.lnprior(om, t) for t in c["base"][ok]])
    assert np.all(np.isfinite(c["lp0"][ok])) and rel_err(c["lp0"][ok], want) <= REL
    assert np.all(c["lp0"][st == OUT] == -np.inf) and np.all(np.isnan(c["lp0"][st == NONUNI]))
    assert np.all(np.isnan(c["fr0"][st == OUT])) and np.all(np.isfinite(c["fr0"][ok]))
    # without the status array the rows the reference would raise on carry their value; the others are unchanged
    inbox = st != OUT
    assert TH.same_bits(c["lp0_bare"][ok], c["lp0"][ok]) and np.all(c["lp0_bare"][~inbox] == -np.inf)
    assert np.mean(np.isfinite(c["lp0_bare"][st == NONUNI])) > 0.9


TABLES = [(1, "random"), (2, "random"), (3, "random"), (64, "random"), (512, "random"), (64, "holed")]


@pytest.mark.parametrize("width", [7, 12])
@pytest.mark.parametrize("N,kind", TABLES, ids=["%d-%s" % t for t in TABLES])
def test_bulk_lnprob_is_the_prior_sum_plus_the_header(width, N, kind):
    """lnprob == lp + host_header(fr) bit for bit, fr the array the same call returned; fr and status are the Gaussian model's; without
    the status array the values are unchanged; rows and columns on device buffers give the same."""
    c = case(width)
    t = random_table(N, 10 * N + width) if kind == "random" else holed_table(N, 7 + width)
    with open_model(width) as m:
        m.set_table_likelihood(t)
        assert m.table_nside == N
        lp, fr, st = m.lnprob(c["base"], want_fr=True, want_status=True)
        bare, fr_bare = m.lnprob(c["base"], want_fr=True, want_status=False)
        dev = {layout: launch_rows(m, c["base"], layout, True) for layout in (GF_LAYOUT_AOS, GF_LAYOUT_SOA)}
    assert np.array_equal(st, c["gst"]) and TH.same_values(fr, c["gfr"])
    ok, inbox = st == OK, st != OUT
    look = np.full(PERIOD, np.nan)
    look[inbox] = TH.host_lookup(t.values, N, fr[inbox])
    assert TH.same_bits(look[inbox], t.lnl(fr[inbox]))                      # ... and the numpy restatement
    want = c["lp0_bare"] + look                                            # one rounding, as the kernel's lp + L
    assert TH.same_bits(lp[ok], want[ok])
    assert np.all(np.isnan(lp[st == NONUNI])) and np.all(lp[st == OUT] == -np.inf) and np.all(np.isnan(lp[st == STNAN]))
    assert not np.any(np.isnan(lp[ok])) and not np.any(lp[ok] == np.inf)
    if kind == "holed":
        assert np.sum(lp[ok] == -np.inf) >= 20 and np.sum(np.isfinite(lp[ok])) >= 20      # -inf with status OK, never NaN
    else:
        assert np.all(np.isfinite(lp[ok]))
    # without the status array: no verdict, every row inside the box has its value
    assert TH.same_values(fr_bare, fr)
    assert TH.same_values(bare[inbox], want[inbox]) and np.all(bare[~inbox] == -np.inf)
    for layout, (dlp, dfr, dst) in dev.items():
        assert TH.same_values(dlp, lp) and TH.same_values(dfr, fr) and np.array_equal(dst, st), layout


@pytest.mark.parametrize("width", [7, 12])
def test_one_launch_past_one_pass_of_the_grid(width):
    """2 * pass_items + 64 * 5 + 29 rows in one launch through lnprob_device, the base block repeated: a base row gives the same bits
    wherever it lands, with and without fr and status, and the guard zones around every output are intact (launch_rows checks them)."""
    c = case(width)
    t = holed_table(64, 3)
    with open_model(width) as m:
        m.set_table_likelihood(t)
        p, n = batch_rows(m)
        assert n >= 2 * p + 64                                             # test_gpu_bulk_passes.py's precondition
        idx = np.arange(n) % PERIOD
        big_rows = np.resize(c["base"], (n, c["base"].shape[1]))
        for outputs in (True, False):
            block = launch_rows(m, c["base"], GF_LAYOUT_AOS, outputs)
            big = launch_rows(m, big_rows, GF_LAYOUT_AOS, outputs)
            for k in range(3):
                assert (big[k] is None) == (block[k] is None)
                if big[k] is not None:
                    assert TH.same_values(big[k], block[k][idx]) if k < 2 else np.array_equal(big[k], block[k][idx]), (outputs, k)
            if outputs:
                ok = block[2] == OK
                look = TH.host_lookup(t.values, 64, block[1][ok])
                assert TH.same_bits(block[0][ok], c["lp0_bare"][ok] + look) and np.array_equal(block[2], c["gst"])


# ---- 2. the nested sampler and the maximiser -----------------------------------------------------------------------------------------
def sens_args(texture=Texture.OEU):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=texture,
                              binning=Cf.default_bin_edges(), smearing=SMEARING, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


SCALES = np.array([-100.0, -45.0, -38.0])


def a_surface(N, seed=5):
    """a smooth surface that is no Gaussian: two bumps of different width, a slope, and a -inf corner (fr_e > 0.9)"""
    def f(fr):
        d1 = np.sum((fr - np.array([0.30, 0.36, 0.34])) ** 2, axis=1)
        d2 = np.sum((fr - np.array([0.55, 0.20, 0.25])) ** 2, axis=1)
        v = np.logaddexp(-d1 / (2 * 0.05 ** 2), -2.0 - d2 / (2 * 0.12 ** 2)) + 3.0 * fr[:, 1]
        return np.where(fr[:, 0] > 0.9, -np.inf, v)
    return llh.TabulatedLikelihood.from_function(f, N)


def close_all(res, key):
    res[key].close()
    for m in res["models"]:
        m.close()


def test_evidence_scan_points_equal_the_bulk_lnprob():
    """Every stored lnL of a table evidence_scan (dead and final live points of three scales, nlive 64) is Model.lnprob of dead()'s theta
    bit for bit, and max_lnl is the largest of them: the walk kernel's table instance against the bulk kernel (check_dead_points of
    test_gpu_cube_runs.py).  The posterior reductions run on the table run unchanged."""
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    res = nested.evidence_scan(args, asimov, ps, SCALES, run_ids=np.arange(3), nlive=64, batch=8, walks=10, seed=7, tol=0.5, table=a_surface(64),
                               return_sampler=True, on_nonunitary="-inf")
    try:
        s = res["sampler"]
        problems = []
        for r, m in enumerate(res["models"]):
            assert m.table_nside == 64
            check_dead_points(s, res, r, m, "table nested", problems)
        print("table nested: lnz %s, niter %s, non-unitary %s" % (res["lnz"], res["niter"], res["nonunitary"]))
        assert not problems, "\n".join(problems)
        assert np.all(np.isfinite(res["lnz"])) and np.all(res["niter"] >= 20)
        post = s.posterior()
        assert np.all(np.isfinite(post["mean"])) and np.all(post["ess"] > 1.0)
        rows = s.posterior_rows(64)
        assert rows.shape == (3, 64, 12) and np.all(np.isfinite(rows))
    finally:
        close_all(res, "sampler")


def full_window_models(tables):
    """test_gpu_cube_runs.py's posterior B with a table per run: 12 columns all scanned, logLam over the whole window of SCALE_BOUNDARIES[6],
    which reaches the region where the reference's unitarity assert fails, so proposals are parked and settled."""
    args = sens_args()
    asimov, ps = Cf.fr_paramsets(6, fr_utils.fr_to_angles(args.injected_ratio))
    names = list(ps.names)
    sc = names.index("logLam")
    cols = [sc] + [i for i in range(len(names)) if i != sc]
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    models = []
    for t in tables:
        models.append(Model(compile_model(ps, "BSM_GAUSS", bestfit_fr=bf, smearing=SMEARING, source_ratio=args.source_ratio, texture=args.texture,
                                          dimension=args.dimension, binning=args.binning)))
        models[-1].set_table_likelihood(t)
    return models, cols, np.tile(np.array(ps.values, dtype=float), (len(tables), 1))


def run_nested(models, cols, bases, run_ids, problems, before_run=None):
    """(result, dead() of every run); every run's points are held to the bulk lnprob, what does not hold goes to `problems`.
    before_run(): called between the sampler's creation and its run (tests/test_gpu_model_changes.py)."""
    with nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=13, tol=0.5, on_nonunitary="-inf", run_ids=run_ids) as s:
        if before_run is not None:
            before_run()
        res = s.run()
        return res, [check_dead_points(s, res, r, m, "table nested window", problems) for r, m in enumerate(models)]


def run_simplex(models, cols, bases, run_ids, starts, before_run=None):
    with P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, starts=starts, maxiter=100, adaptive=True, restarts=1,
                            on_nonunitary="-inf", run_ids=run_ids) as s:
        if before_run is not None:
            before_run()
        res = s.run()
        return res, [s.starts(r) for r in range(len(models))], [s.cube_to_theta(r, s.starts(r)["cube"][:int(res["nstarts"][r])])
                                                               for r in range(len(models))]


def test_runs_with_sides_3_and_64_in_one_set_and_parked_proposals():
    """A nested sampler and a maximiser over two runs whose tables have sides 3 and 64, every column scanned with logLam over its whole
    window: every stored value is the bulk lnprob of the reported theta bit for bit -- proposals the reference would have raised on occur, so
    parked ones were settled -- and each run gives in the set what it gives alone."""
    tables = [a_surface(3), a_surface(64)]
    models, cols, bases = full_window_models(tables)
    try:
        assert [m.table_nside for m in models] == [3, 64]
        problems = []
        res, dead = run_nested(models, cols, bases, [0, 1], problems)
        assert not problems, "\n".join(problems)
        print("table nested window: non-unitary %s, niter %s" % (res["nonunitary"], res["niter"]))
        assert np.all(res["nonunitary"] > 0), res["nonunitary"]
        for r in range(2):
            alone, dead1 = run_nested(models[r:r + 1], cols, bases[r:r + 1], [r], problems)
            assert not problems and TH.same_bits(alone["lnz"], res["lnz"][r:r + 1]) and TH.same_bits(alone["max_lnl"], res["max_lnl"][r:r + 1])
            assert alone["niter"][0] == res["niter"][r] and TH.same_bits(dead1[0]["lnl"], dead[r]["lnl"])
            assert TH.same_bits(dead1[0]["cube"], dead[r]["cube"])
        # the maximiser
        starts = np.random.default_rng(23).uniform(0.3, 0.7, size=(2, 2, len(cols)))
        starts[:, :, 0] = [[0.2, 0.45], [0.3, 0.5]]                        # logLam: inside the window where lnprob is finite
        sres, sstarts, sth = run_simplex(models, cols, bases, [0, 1], starts)
        print("table simplex window: non-unitary %s, parked %s, max_lnl %s" % (sres["nonunitary"], sres["parked"], sres["max_lnl"]))
        for r, m in enumerate(models):
            used = int(sres["nstarts"][r])
            assert used == 3
            th = np.tile(bases[r], (used, 1))
            th[:, cols] = sth[r]
            lp, st = m.lnprob(th, want_status=True)
            good = (st == OK) & (lp > -np.inf)
            fun = sstarts[r]["lnl"][:used]
            assert good.sum() >= 1 and TH.same_bits(fun[good], lp[good]) and np.all(fun[~good] == -np.inf), (r, fun, lp)
            assert TH.same_bits(m.lnprob(sres["argmax_theta"][r:r + 1], want_status=False), sres["max_lnl"][r:r + 1])
            assert TH.same_bits(sres["max_lnl"][r:r + 1], [fun.max()])
            alone, astarts, _ = run_simplex(models[r:r + 1], cols, bases[r:r + 1], [r], starts[r:r + 1])
            assert TH.same_bits(alone["max_lnl"], sres["max_lnl"][r:r + 1]) and TH.same_bits(astarts[0]["lnl"], sstarts[r]["lnl"])
            assert TH.same_bits(astarts[0]["cube"], sstarts[r]["cube"])
        assert sres["parked"].sum() > 0, sres["parked"]
    finally:
        for m in models:
            m.close()


def test_profile_scan_values_equal_the_bulk_lnprob():
    """profile_scan(..., table=) on three scales, 3 starts: -fun of every start is Model.lnprob at cube_to_theta of its cube point, max_lnl
    is Model.lnprob(argmax_theta) and the best start's value, bit for bit."""
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    res = P.profile_scan(args, asimov, ps, SCALES, run_ids=np.arange(3), nstarts=3, nseed=256, seed=3, table=a_surface(64), on_nonunitary="-inf",
                         return_maximizer=True)
    try:
        s = res["maximizer"]
        names = list(ps.names)
        cols = [i for i in range(len(names)) if names[i] != "logLam"]
        print("table profile: max_lnl %s, non-unitary %s, parked %s" % (res["max_lnl"], res["nonunitary"], res["parked"]))
        assert np.all(np.isfinite(res["max_lnl"]))
        for r, m in enumerate(res["models"]):
            assert m.table_nside == 64
            used = int(res["nstarts"][r])
            dev = s.starts(r)
            th = np.tile(s.bases[r], (used, 1))
            th[:, cols] = s.cube_to_theta(r, dev["cube"][:used])
            lp, st = m.lnprob(th, want_status=True)
            good = (st == OK) & (lp > -np.inf)
            fun = dev["lnl"][:used]
            assert used == 3 and good.sum() >= 1
            assert TH.same_bits(fun[good], lp[good]) and np.all(fun[~good] == -np.inf), (r, fun, lp)
            assert TH.same_bits(m.lnprob(res["argmax_theta"][r:r + 1], want_status=False), res["max_lnl"][r:r + 1])
            assert TH.same_bits(res["max_lnl"][r:r + 1], [fun.max()])
    finally:
        close_all(res, "maximizer")


def test_bsm_ln_prob_with_a_table():
    """llh.bsm_ln_prob(..., table=) is the callable of a model with that table; binned and table together are refused."""
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    t = a_surface(64)
    rng = np.random.default_rng(4)
    box = np.array(ps.seeds, dtype=float)
    th = rng.uniform(box[:, 0], box[:, 1], size=(300, len(ps)))
    th[:, list(ps.names).index("logLam")] = rng.uniform(-56.0, -42.0, 300)
    f = llh.bsm_ln_prob(args, asimov, ps, table=t, on_nonunitary="-inf")
    g = llh.bsm_ln_prob(args, asimov, ps, on_nonunitary="-inf")
    try:
        assert f.model.table_nside == 64 and g.model.table_nside == 0
        lp, fr, st = f.model.lnprob(th, want_fr=True, want_status=True)
        g.model.set_table_likelihood(np.zeros(3))
        prior = g.model.lnprob(th, want_status=False)
        ok = st == OK
        assert ok.sum() >= 200 and TH.same_bits(f(th)[ok], lp[ok]) and TH.same_bits(lp[ok], prior[ok] + t.lnl(fr[ok]))
        assert isinstance(f(th[np.flatnonzero(ok)[0]]), float)
    finally:
        f.close()
        g.close()
    with pytest.raises(ValueError):
        llh.bsm_ln_prob(args, asimov, ps, table=t, binned=llh.BinnedMeasurement(np.full((20, 3), 1 / 3), np.full(20, 0.05)))


# ---- 3. against the Gaussian -----------------------------------------------------------------------------------------------------------
GAUSS_N = 512
GAUSS_BOUND = 3.0 / (SMEARING * GAUSS_N) ** 2          # 0.0286: the linear interpolation error for a Hessian of norm 3 / s^2 over a cell of diameter sqrt(2) / N
assert GAUSS_BOUND < 0.05


@pytest.mark.parametrize("width", [7, 12])
def test_gaussian_table_against_the_gaussian_per_row(width):
    """from_gaussian(the model's measurement and width, N = 512, the model's offset) against the Gaussian model's lnprob row by row:
    within 3 / (s N)^2.  Rows whose Gaussian ln L lies below -700 are left to the -inf rule: there the reference's multi_gaussian leaves the
    quadratic form (the subnormal band from -708.4, -inf from -745.1), and a cell of diameter sqrt(2) / N spans up to 5.2 in ln L."""
    c = case(width)
    t = llh.TabulatedLikelihood.from_gaussian(BF, SMEARING, GAUSS_N, offset=OFFSET)
    with open_model(width) as m:
        m.set_table_likelihood(t)
        lp, st = m.lnprob(c["base"], want_status=True)
    assert np.array_equal(st, c["gst"])
    ok = st == OK
    gl = np.asarray(llh.multi_gaussian(c["gfr"][ok], BF, SMEARING, offset=0.0))
    rows = gl >= -700.0
    err = np.abs(lp[ok][rows] - c["glp"][ok][rows])
    print("Gaussian table, %d columns: %d rows, worst |diff| %.3e, bound %.3e" % (width, rows.sum(), err.max(), GAUSS_BOUND))
    assert rows.sum() >= 300 and np.all(np.isfinite(lp[ok][rows])) and np.all(err <= GAUSS_BOUND)
    wall = gl == -np.inf
    assert np.all(lp[ok][wall] == -np.inf)


def test_gaussian_table_evidence_against_the_gaussian_evidence():
    """The table scan's lnz within 4 lnz_err + 3 / (s N)^2 of the Gaussian scan's at the same seeds, three scales."""
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    kw = dict(run_ids=np.arange(3), nlive=128, batch=16, walks=10, seed=7, tol=0.5, on_nonunitary="-inf")
    g = nested.evidence_scan(args, asimov, ps, SCALES, **kw)
    t = nested.evidence_scan(args, asimov, ps, SCALES, table=llh.TabulatedLikelihood.from_gaussian(bf, SMEARING, GAUSS_N, offset=OFFSET), **kw)
    diff = np.abs(t["lnz"] - g["lnz"])
    print("lnz Gaussian %s +- %s, table %s +- %s, |diff| %s" % (g["lnz"], g["lnz_err"], t["lnz"], t["lnz_err"], diff))
    assert np.all(np.isfinite(g["lnz"])) and np.all(np.isfinite(t["lnz"]))
    assert np.all(diff <= 4.0 * g["lnz_err"] + GAUSS_BOUND), (diff, g["lnz_err"])


# ---- 4. the reweight path --------------------------------------------------------------------------------------------------------------
def test_reweight_a_gaussian_chain_to_the_table_model():
    """reweight([table_model]) on a short Gaussian chain: lnw = table.lnprob(rows) - stored lnprob on the host, bit for bit."""
    rng = np.random.default_rng(12)
    ps = paramset_of(7)
    with open_model(7) as m, open_model(7) as target:
        target.set_table_likelihood(a_surface(64))
        box = np.array(ps.ranges, dtype=float)
        p0 = rng.uniform(box[:, 0], box[:, 1], size=(32, 7))
        p0[:, -1] = rng.uniform(-50.0, -42.0, 32)
        s = mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=5)
        s.on_nonunitary = "-inf"
        try:
            s.run_mcmc(p0, 40)
            ch, lp0, _ = s._fetch(chain=True, lnprob=True)
            rows, lp0 = ch.reshape(-1, 7), lp0.reshape(-1)
            r = s.reweight([target], on_nonunitary="-inf")
            lnw = r.lnw(0)[0]
            lt, st = target.lnprob(rows, want_status=True)
            keep = np.isfinite(lp0) & (st == OK) & np.isfinite(lt)
            assert keep.sum() >= 1000
            assert TH.same_bits(lnw[keep], lt[keep] - lp0[keep]) and np.all(lnw[~keep] == -np.inf)
        finally:
            s.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def raw_set(m, nside, values):
    v = np.ascontiguousarray(values, dtype=np.float64)
    return _lib.lib().gf_model_set_table_likelihood(m._h, int(nside), v.ctypes.data_as(_lib._dp))


def test_refusals_leave_the_models_usable():
    L = _lib.lib()
    c = case(7)
    th = c["base"][:400]
    good = random_table(8, 1)
    # a table on an SM model and on a prior-only model
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, nps = Cf.notebook_paramsets(ang)
    for mode in ("SM_GAUSS", "PRIOR_ONLY"):
        with Model(compile_model(nps, mode, bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02)) as sm:
            assert raw_set(sm, 8, good.values) == _lib.GF_ERR_UNSUPPORTED and sm.table_nside == 0
            with pytest.raises(_lib.GolemHipError) as e:
                sm.set_table_likelihood(good)
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED
    with open_model(7) as m, open_model(7) as other, open_model(7) as binned:
        before = m.lnprob(th, want_status=False)
        # bad tables
        bad = good.values.copy()
        for k, v in ((3, np.nan), (5, np.inf)):
            b = bad.copy()
            b[k] = v
            assert raw_set(m, 8, b) == _lib.GF_ERR_INVALID_ARG and (b"NaN" in L.gf_last_hip_error() or b"+inf" in L.gf_last_hip_error())
        assert raw_set(m, 8, np.full(45, -np.inf)) == _lib.GF_ERR_INVALID_ARG and b"-inf" in L.gf_last_hip_error()
        assert raw_set(m, 0, good.values) == _lib.GF_ERR_INVALID_ARG and raw_set(m, _lib.GF_TABLE_MAX_NSIDE + 1, good.values) == _lib.GF_ERR_INVALID_ARG
        assert L.gf_model_set_table_likelihood(m._h, 8, None) == _lib.GF_ERR_INVALID_ARG
        assert m.table_nside == 0 and L.gf_model_table_nside(None) == 0
        assert TH.same_bits(m.lnprob(th, want_status=False), before)
        # binned-on-table and table-on-binned
        meas = llh.BinnedMeasurement(np.full((20, 3), 1 / 3), np.full(20, 0.05))
        binned.set_binned_measurement(meas)
        assert raw_set(binned, 8, good.values) == _lib.GF_ERR_UNSUPPORTED and b"binned" in L.gf_last_hip_error() and binned.table_nside == 0
        m.set_table_likelihood(good)
        tabled = m.lnprob(th, want_status=False)
        assert m.table_nside == 8 and not TH.same_values(tabled, before)
        with pytest.raises(_lib.GolemHipError) as e:
            m.set_binned_measurement(meas)
        assert e.value.code == _lib.GF_ERR_UNSUPPORTED and not m.is_binned
        # a run set carries tables or it does not
        ps = paramset_of(7)
        cols = np.arange(6, dtype=np.int32)
        base = np.tile(np.array(ps.values, dtype=np.float64), (2, 1))
        hs = (C.c_void_p * 2)(m._h, other._h)
        for create, tail in ((L.gf_nested_create, (64, 8, 5, 1, 0)), (L.gf_simplex_create, (4, 64, 1, 0))):
            h = C.c_void_p()
            rc = create(hs, 2, 6, cols.ctypes.data_as(_lib._ip), base.ctypes.data_as(_lib._dp), *tail, C.byref(h))
            assert rc == _lib.GF_ERR_INVALID_ARG and not h.value and b"tabulated" in L.gf_last_hip_error()
        # the ensemble sampler never samples the Gaussian posterior of a table model
        for fn, arg, n in ((L.gf_sampler_create, m._h, 1), (L.gf_sampler_create_multi, (C.c_void_p * 2)(other._h, m._h), 2),
                           (L.gf_sampler_create_binned, (C.c_void_p * 1)(m._h), 1)):
            h = C.c_void_p()
            rc = fn(arg, n, 1, 32, 5, 2.0, C.byref(h)) if fn is L.gf_sampler_create_binned else fn(arg, n, 32, 5, 2.0, C.byref(h))
            assert rc == _lib.GF_ERR_UNSUPPORTED and not h.value and b"tabulated" in L.gf_last_hip_error(), fn
        with pytest.raises(_lib.GolemHipError) as e:
            mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=1)
        assert e.value.code == _lib.GF_ERR_UNSUPPORTED
        # what sets or reweights to a Gaussian measurement refuses a table set
        other.set_table_likelihood(random_table(3, 2))
        for create in (L.gf_toys_create, L.gf_toys_create_binned):
            h = C.c_void_p()
            rc = create(hs, 2, 6, cols.ctypes.data_as(_lib._ip), base.ctypes.data_as(_lib._dp), 64, 1, C.byref(h))
            assert rc == _lib.GF_ERR_UNSUPPORTED and not h.value and b"tabulated" in L.gf_last_hip_error(), create
        bf2, sm2 = np.full((2, 3), 1 / 3), np.full(2, 0.05)
        for nseed in (0, 64):
            h = C.c_void_p()
            assert L.gf_simplex_create(hs, 2, 6, cols.ctypes.data_as(_lib._ip), base.ctypes.data_as(_lib._dp), min(2, nseed), nseed, 1, 1,
                                       C.byref(h)) == _lib.GF_OK
            try:
                assert L.gf_toys_set_measurements(h, bf2.ctypes.data_as(_lib._dp), sm2.ctypes.data_as(_lib._dp)) == _lib.GF_ERR_UNSUPPORTED
                assert b"tabulated" in L.gf_last_hip_error()
                fb, sg = np.full((2, 20, 3), 1 / 3), np.full((2, 20), 0.05)
                assert L.gf_toys_set_binned_measurements(h, 20, fb.ctypes.data_as(_lib._dp), sg.ctypes.data_as(_lib._dp)) == _lib.GF_ERR_UNSUPPORTED
                assert b"tabulated" in L.gf_last_hip_error()
            finally:
                L.gf_simplex_destroy(h)
        with nested.NestedSampler([m, other], cols, base, nlive=64, batch=8, walks=5, seed=1, tol=0.5, on_nonunitary="-inf") as s:
            s.run()
            out = [np.zeros((2, 2)) for _ in range(4)]
            kept = np.zeros((2, 2), np.int64)
            rc = L.gf_nested_toys_evidence(s._h, bf2.ctypes.data_as(_lib._dp), sm2.ctypes.data_as(_lib._dp), 2, 0,
                                           *[o.ctypes.data_as(_lib._dp) for o in out], kept.ctypes.data_as(C.POINTER(C.c_int64)))
            assert rc == _lib.GF_ERR_UNSUPPORTED and b"tabulated" in L.gf_last_hip_error()
        # the models are what they were, and a table can be replaced: a smaller one in place, a larger one too
        assert TH.same_bits(m.lnprob(th, want_status=False), tabled)
        for N in (3, 64, 8):
            t = random_table(N, 40 + N)
            m.set_table_likelihood(t)
            lp, fr, st = m.lnprob(th, want_fr=True, want_status=True)
            ok = st == OK
            assert m.table_nside == N and TH.same_bits(lp[ok], c["lp0_bare"][:400][ok] + TH.host_lookup(t.values, N, fr[ok]))


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------
SENS = [sys.executable, "-m", "golemflavor_amd.sens", "--segments", "3", "--smearing", "0.1", "--seed", "3"]
SENS_METHOD = {"bayesian": ["--mn-live-points", "100", "--mn-walks", "10"],
               "frequentist": ["--stat-method", "frequentist", "--pl-starts", "4", "--pl-seed-points", "512"]}


@pytest.mark.parametrize("method", ["bayesian", "frequentist"])
def test_sens_command_line(tmp_path, method):
    """--likelihood-table writes _ltab files whose values are the table scan's; without the option the files are byte for byte the ones the
    command wrote before the option existed (tests/golden/table_sens.npz: the files' bytes, written by the build of the commit before the option
    with these arguments)."""
    f = tmp_path / "table.npy"
    a_surface(32).save(str(f))
    base = SENS + SENS_METHOD[method]
    out = subprocess.run(base + ["--datadir", str(tmp_path / "t"), "--likelihood-table", str(f)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["likelihood"] == "table" and line["table_nside"] == 32
    for k in ("fr_stat", "fr_maxllh"):
        assert os.path.basename(line[k]).endswith("_ltab.npy") and os.path.isfile(line[k]), line[k]
        arr = np.load(line[k])
        assert arr.shape == (3, 2) and np.array_equal(arr[:, 0], nested.sens_scales(6, 3)) and np.all(np.isfinite(arr))
    assert np.array_equal(np.load(line["fr_maxllh"])[:, 1], np.asarray(line["max_lnl"]))
    plain = subprocess.run(base + ["--datadir", str(tmp_path / "p")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-3000:]
    pl = json.loads(plain.stdout.strip().splitlines()[-1])
    assert "likelihood" not in pl and not np.array_equal(np.load(pl["fr_maxllh"]), np.load(line["fr_maxllh"]))
    for k in ("fr_stat", "fr_maxllh"):
        name = os.path.basename(pl[k])
        assert "_ltab" not in name
        with open(pl[k], "rb") as got, np.load(GOLDEN, allow_pickle=False) as want:
            assert got.read() == want["%s/%s" % (method, name)].tobytes(), (method, name)
