"""GPU: live handles and a model whose likelihood is set again after they exist ("Models that change under a live
handle"; csrc/gf_modelset.hip, cube_runs_begin in csrc/gf_cube_runs.hip, sampler_kind_refusal in csrc/gf_sampler_host.hip).

A. a set's kind -- tabulated, binned or neither -- is fixed at creation: a model that gains a likelihood afterwards is refused by every
   entry point that evaluates, and what the handle holds stays readable and unchanged;
B. the first run of a nested sampler or a maximiser takes the tables (and, their address being stable, the measurements) of now;
C. a run that has begun does not change likelihood: it is refused once one of its models has had its likelihood set again;
and the ensemble samplers go on sampling what their models carry at the start of each run.

Every comparison is bit for bit: the yardstick is `Model.lnprob` of the models as they are now, and a handle created after the change."""
import ctypes as C

import numpy as np
import pytest

import table_harness as TH
from common import BIN_EDGES
from golemflavor_amd import _lib, llh, nested
from golemflavor_amd import configs as Cf
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import profile_llh as P
from golemflavor_amd.enums import Texture
from stretch_ref import reference_stretch
from test_gpu_binned import sens_args as binned_sens_args, sens_measurement
from test_gpu_binned_sampler import a_measurement, assert_same_run, binned_model, bulk, device_run, scale_rows
from test_gpu_binned_sampler import run_against_reference as binned_run_against_reference
from test_gpu_table import OK, a_surface, full_window_models, open_model, paramset_of, random_table, raw_set, run_nested, run_simplex

pytestmark = pytest.mark.gpu

INVALID = _lib.GF_ERR_INVALID_ARG
I64 = C.POINTER(C.c_int64)


def halved(t):
    """another table of the same side: every node halved (-inf stays), so that the surface keeps its shape"""
    return llh.TabulatedLikelihood(0.5 * t.values)


# (the table run 1's model carries when the handle is created, the one it carries when the handle first runs)
TABLE_CASES = {"64-to-64-in-place": (lambda: a_surface(64), lambda: halved(a_surface(64))),
               "64-to-3-in-place": (lambda: a_surface(64), lambda: a_surface(3)),
               "3-to-64-moves": (lambda: a_surface(3), lambda: a_surface(64))}


def differ_on(old, new, m, theta):
    """the share of the rows of theta the bulk kernel accepts at whose composition the two tables give different bits"""
    lp, fr, st = m.lnprob(theta, want_fr=True, want_status=True)
    ok = st == OK
    assert ok.sum() >= 1
    return float(np.mean(old.lnl(fr[ok]).view(np.int64) != new.lnl(fr[ok]).view(np.int64)))


_ALONE = {}


def run0_alone(models, cols, bases, problems):
    """run 0 (a_surface(64), run id 0) by itself: the same for every case, computed once and read-only"""
    if "nested" not in _ALONE:
        res, dead = run_nested(models[:1], cols, bases[:1], [0], problems)
        for v in list(res.values()) + [dead[0]["lnl"], dead[0]["cube"]]:
            v.setflags(write=False)
        _ALONE["nested"] = (res, dead[0])
    return _ALONE["nested"]


# ---- 1. nested: the table is replaced between the handle's creation and its first run ----------------------------------------------------
@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_nested_first_run_takes_the_tables_of_now(case):
    """Posterior B with a table per run, two runs; run 1's table is replaced after gf_nested_create and before the first gf_nested_run.
    Every dead and final live lnL of both runs is Model.lnprob of now (check_dead_points, inside run_nested); the run is the run of a
    handle created after the replacement; run 0, whose model is untouched, is what it gives alone; proposals were parked."""
    old, new = (f() for f in TABLE_CASES[case])
    models, cols, bases = full_window_models([a_surface(64), old])
    try:
        problems = []
        res, dead = run_nested(models, cols, bases, [0, 1], problems, before_run=lambda: models[1].set_table_likelihood(new))
        assert models[1].table_nside == new.nside
        print("%s: niter %s, non-unitary %s, lnz %s" % (case, res["niter"], res["nonunitary"], res["lnz"]))
        assert not problems, "\n".join(problems)
        assert np.all(res["nonunitary"] > 0), res["nonunitary"]
        share = differ_on(old, new, models[1], dead[1]["theta"])
        print("%s: the two tables differ on %.0f %% of run 1's points" % (case, 100 * share))
        assert share > 0.5, "the replacement changes too little: nothing was compared"
        fresh, fdead = run_nested(models, cols, bases, [0, 1], problems)
        assert not problems, "\n".join(problems)
        for k in ("lnz", "max_lnl"):
            assert TH.same_bits(res[k], fresh[k]), (k, res[k], fresh[k])
        assert np.array_equal(res["niter"], fresh["niter"])
        for r in range(2):
            assert TH.same_bits(dead[r]["lnl"], fdead[r]["lnl"]) and TH.same_bits(dead[r]["cube"], fdead[r]["cube"]), r
        alone, adead = run0_alone(models, cols, bases, problems)
        assert not problems, "\n".join(problems)
        assert TH.same_bits(alone["lnz"], res["lnz"][:1]) and TH.same_bits(alone["max_lnl"], res["max_lnl"][:1]) and alone["niter"][0] == res["niter"][0]
        assert TH.same_bits(adead["lnl"], dead[0]["lnl"]) and TH.same_bits(adead["cube"], dead[0]["cube"])
    finally:
        for m in models:
            m.close()


# ---- 2. the maximiser, the same three cases ----------------------------------------------------------------------------------------------
def window_starts(ncols):
    """test_gpu_table.py's two given starts per run"""
    starts = np.random.default_rng(23).uniform(0.3, 0.7, size=(2, 2, ncols))
    starts[:, :, 0] = [[0.2, 0.45], [0.3, 0.5]]                            # logLam: inside the window where lnprob is finite
    return starts


@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_maximiser_first_run_takes_the_tables_of_now(case):
    """`fun` of every used start is Model.lnprob of now at cube_to_theta of its cube point, max_lnl is Model.lnprob(argmax_theta), and
    starts and results are those of a handle created after the replacement."""
    old, new = (f() for f in TABLE_CASES[case])
    models, cols, bases = full_window_models([a_surface(64), old])
    try:
        starts = window_starts(len(cols))
        res, sstarts, sth = run_simplex(models, cols, bases, [0, 1], starts, before_run=lambda: models[1].set_table_likelihood(new))
        assert models[1].table_nside == new.nside
        print("%s: max_lnl %s, non-unitary %s, parked %s" % (case, res["max_lnl"], res["nonunitary"], res["parked"]))
        for r, m in enumerate(models):
            used = int(res["nstarts"][r])
            assert used == 3
            th = np.tile(bases[r], (used, 1))
            th[:, cols] = sth[r]
            lp, st = m.lnprob(th, want_status=True)
            good = (st == OK) & (lp > -np.inf)
            fun = sstarts[r]["lnl"][:used]
            assert good.sum() >= 1 and TH.same_bits(fun[good], lp[good]) and np.all(fun[~good] == -np.inf), (r, fun, lp)
            assert TH.same_bits(m.lnprob(res["argmax_theta"][r:r + 1], want_status=False), res["max_lnl"][r:r + 1])
            assert TH.same_bits(res["max_lnl"][r:r + 1], [fun.max()])
            if r == 1:
                share = differ_on(old, new, m, th)
                assert share > 0.5, "the replacement changes too little: nothing was compared"
        fresh, fstarts, _ = run_simplex(models, cols, bases, [0, 1], starts)
        for k in ("max_lnl", "argmax_cube"):
            assert TH.same_bits(res[k], fresh[k]), (k, res[k], fresh[k])
        for k in ("nstarts", "niter", "nfev", "nonunitary", "parked"):
            assert np.array_equal(res[k], fresh[k]), (k, res[k], fresh[k])
        for r in range(2):
            assert TH.same_bits(sstarts[r]["lnl"], fstarts[r]["lnl"]) and TH.same_bits(sstarts[r]["cube"], fstarts[r]["cube"]), r
    finally:
        for m in models:
            m.close()


# ---- 3. binned cube runs: a measurement's address is the model's for good ------------------------------------------------------------------
BINNED_SCALES = np.array([-100.0, -45.0])


def binned_models(meas):
    """test_gpu_binned.py's two sens scales with `meas` on both models: (cols, models, bases)"""
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    cols, models, bases, _ = nested._scan_models(binned_sens_args(), asimov, ps, BINNED_SCALES, 0.02, 0, binned=meas)
    return cols, models, np.array(bases)


def two_measurements():
    asimov, _ = Cf.sens_paramsets(6, (1., 1., 1.))
    return sens_measurement(asimov), a_measurement(20, Cf.default_bin_edges(), seed=8, smearing=0.05)


def binned_nested(models, cols, bases, change=None):
    with nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=7, tol=0.5, on_nonunitary="-inf", run_ids=[0, 1]) as s:
        if change is not None:
            change()
        res = s.run()
        return res, [s.dead(r) for r in range(len(models))]


def binned_simplex(models, cols, bases, change=None):
    with P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, starts=np.full((2, len(cols)), 0.5), maxiter=100,
                            on_nonunitary="-inf", run_ids=[0, 1]) as s:
        if change is not None:
            change()
        res = s.run()
        return res, [s.starts(r) for r in range(len(models))]


def test_binned_cube_runs_take_the_measurement_of_now():
    """A nested sampler and a maximiser over two binned models; run 1's measurement is replaced between creation and the first run.
    Stored values are Model.lnprob of now, and both equal a handle created after the replacement."""
    first, second = two_measurements()
    cols, models, bases = binned_models(first)
    cols2, twins, _ = binned_models(first)                                 # keep the first measurement: what a stale run would have evaluated
    try:
        res, dead = binned_nested(models, cols, bases, change=lambda: models[1].set_binned_measurement(second))
        print("binned nested: niter %s, lnz %s" % (res["niter"], res["lnz"]))
        for r, m in enumerate(models):
            lp, st = m.lnprob(dead[r]["theta"], want_status=True)
            ok = st == OK
            assert ok.sum() >= len(lp) - 64 and len(lp) >= 64 + 8 * 20
            assert TH.same_bits(dead[r]["lnl"][ok], lp[ok]) and np.all(dead[r]["lnl"][~ok] == -np.inf), r
            assert TH.same_bits(res["max_lnl"][r:r + 1], [lp[ok].max()])
            if r == 1:
                stale = twins[1].lnprob(dead[r]["theta"][ok], want_status=False)
                share = np.mean(stale.view(np.int64) != lp[ok].view(np.int64))
                print("the two measurements differ on %.0f %% of run 1's points" % (100 * share))
                assert share > 0.5, "the replacement changes too little: nothing was compared"
        fresh, fdead = binned_nested(models, cols, bases)
        assert TH.same_bits(res["lnz"], fresh["lnz"]) and TH.same_bits(res["max_lnl"], fresh["max_lnl"]) and np.array_equal(res["niter"], fresh["niter"])
        for r in range(2):
            assert TH.same_bits(dead[r]["lnl"], fdead[r]["lnl"]) and TH.same_bits(dead[r]["cube"], fdead[r]["cube"]), r
        # the maximiser: back to the first measurement at creation, the second at the first run
        models[1].set_binned_measurement(first)
        sres, sstarts = binned_simplex(models, cols, bases, change=lambda: models[1].set_binned_measurement(second))
        for r, m in enumerate(models):
            assert int(sres["nstarts"][r]) == 3
            assert TH.same_bits(m.lnprob(sres["argmax_theta"][r:r + 1], want_status=False), sres["max_lnl"][r:r + 1]), r
            assert TH.same_bits(sres["max_lnl"][r:r + 1], [sstarts[r]["lnl"][:3].max()])
        assert not TH.same_bits(twins[1].lnprob(sres["argmax_theta"][1:2], want_status=False), sres["max_lnl"][1:2])
        sfresh, fstarts = binned_simplex(models, cols, bases)
        for k in ("max_lnl", "argmax_cube"):
            assert TH.same_bits(sres[k], sfresh[k]), (k, sres[k], sfresh[k])
        for k in ("nstarts", "niter", "nfev", "nonunitary", "parked"):
            assert np.array_equal(sres[k], sfresh[k]), (k, sres[k], sfresh[k])
        for r in range(2):
            assert TH.same_bits(sstarts[r]["lnl"], fstarts[r]["lnl"]) and TH.same_bits(sstarts[r]["cube"], fstarts[r]["cube"]), r
    finally:
        for m in list(models) + list(twins):
            m.close()


# ---- 4. a run that has begun does not change likelihood --------------------------------------------------------------------------------------
def last_error():
    return _lib.lib().gf_last_hip_error().decode()


def nested_snapshot(s):
    res = s.result()
    return res, [s.dead(r) for r in range(s.nruns)]


def same_nested_snapshot(a, b):
    (ra, da), (rb, db) = a, b
    for k in ("lnz", "lnz_err", "info", "max_lnl"):
        assert TH.same_bits(ra[k], rb[k]), k
    for k in ("niter", "nevals", "nonunitary", "failed"):
        assert np.array_equal(ra[k], rb[k]), k
    for x, y in zip(da, db):
        for k in ("lnl", "lnw", "cube"):
            assert TH.same_bits(x[k], y[k]), k


def simplex_snapshot(s):
    return s.result(), [s.starts(r) for r in range(s.nruns)]


def same_simplex_snapshot(a, b):
    (ra, sa), (rb, sb) = a, b
    for k in ("max_lnl", "argmax_cube"):
        assert TH.same_values(ra[k], rb[k]), k
    for k in ("nstarts", "niter", "nfev", "nevals", "nonunitary", "parked", "failed"):
        assert np.array_equal(ra[k], rb[k]), k
    for x, y in zip(sa, sb):
        assert TH.same_values(x["lnl"], y["lnl"]) and TH.same_values(x["cube"], y["cube"])
        assert np.array_equal(x["nit"], y["nit"]) and np.array_equal(x["nfev"], y["nfev"])


def begun_nested(models, cols, bases):
    """a nested sampler eight iterations into its runs, none of which has finished"""
    L = _lib.lib()
    s = nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=13, tol=0.5, on_nonunitary="-inf", run_ids=[0, 1])
    try:
        assert L.gf_nested_run(s._h, 8) == _lib.GF_ERR_UNSUPPORTED and "max_iter" in last_error()
        assert np.array_equal(s.result()["niter"], [8, 8])
    except BaseException:
        s.close()
        raise
    return s


def begun_simplex(models, cols, bases):
    """a maximiser three rounds into its runs"""
    L = _lib.lib()
    s = P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, starts=window_starts(len(cols)), maxiter=100,
                           on_nonunitary="-inf", run_ids=[0, 1])
    try:
        assert L.gf_simplex_run(s._h, 3) == _lib.GF_OK
        assert np.all(s.result()["nstarts"] == 3)
    except BaseException:
        s.close()
        raise
    return s


@pytest.mark.parametrize("new_side", [64, 3], ids=["same-side-in-place", "smaller-in-place"])
def test_a_begun_table_run_refuses_a_replaced_table(new_side):
    """gf_nested_run(max_iter = 8) and gf_simplex_run(max_rounds = 3), then run 1's table of side 64 is replaced: the next run call is
    GF_ERR_INVALID_ARG naming the call and model 1, and result, dead points and starts are what they were.  A table set on a model outside
    the set refuses nothing."""
    L = _lib.lib()
    models, cols, bases = full_window_models([a_surface(64), a_surface(64)])
    outsider = open_model(12)
    try:
        for begun, run, snapshot, same, more in ((begun_nested, L.gf_nested_run, nested_snapshot, same_nested_snapshot, 12),
                                                 (begun_simplex, L.gf_simplex_run, simplex_snapshot, same_simplex_snapshot, 3)):
            models[1].set_table_likelihood(a_surface(64))
            s = begun(models, cols, bases)
            try:
                what = "gf_%s_run" % s._abi
                outsider.set_table_likelihood(random_table(new_side, 81))
                count = _lib.likelihood_sets(models[1]._h)
                assert raw_set(models[1], 8, np.full(45, np.nan)) == INVALID  # a refused table is no replacement
                assert _lib.likelihood_sets(models[1]._h) == count
                rc = run(s._h, more)                                       # goes on: four more iterations / three more rounds
                assert rc == (_lib.GF_ERR_UNSUPPORTED if s._abi == "nested" else _lib.GF_OK), (what, rc, last_error())
                kept = snapshot(s)
                if s._abi == "nested":
                    assert np.array_equal(kept[0]["niter"], [12, 12])
                models[1].set_table_likelihood(random_table(new_side, 82))
                assert models[1].table_nside == new_side and _lib.likelihood_sets(models[1]._h) == count + 1
                for _ in range(2):
                    assert run(s._h, 100000) == INVALID
                    msg = last_error()
                    assert msg.startswith(what + ":") and "model 1" in msg and "replaced" in msg, msg
                    same(snapshot(s), kept)
                with pytest.raises(_lib.GolemHipError) as e:
                    s.run()
                assert e.value.code == INVALID and "model 1" in str(e.value)
            finally:
                s.close()
    finally:
        for m in models + [outsider]:
            m.close()


def test_a_begun_binned_run_refuses_a_replaced_measurement():
    L = _lib.lib()
    first, second = two_measurements()
    cols, models, bases = binned_models(first)
    try:
        for kind in ("nested", "simplex"):
            models[0].set_binned_measurement(first)
            if kind == "nested":
                s = nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=7, tol=0.5, on_nonunitary="-inf", run_ids=[0, 1])
                run, snapshot, same = L.gf_nested_run, nested_snapshot, same_nested_snapshot
            else:
                s = P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, starts=np.full((2, len(cols)), 0.5), maxiter=100,
                                       on_nonunitary="-inf", run_ids=[0, 1])
                run, snapshot, same = L.gf_simplex_run, simplex_snapshot, same_simplex_snapshot
            try:
                rc = run(s._h, 8 if kind == "nested" else 3)
                assert rc == (_lib.GF_ERR_UNSUPPORTED if kind == "nested" else _lib.GF_OK), (kind, rc, last_error())
                kept = snapshot(s)
                models[0].set_binned_measurement(second)
                assert run(s._h, 100000) == INVALID
                msg = last_error()
                assert msg.startswith("gf_%s_run:" % kind) and "model 0" in msg and "replaced" in msg, msg
                same(snapshot(s), kept)
            finally:
                s.close()
    finally:
        for m in models:
            m.close()


# ---- 5. a model gains a likelihood after the handle exists -------------------------------------------------------------------------------------
def gain(model, word):
    if word == "tabulated":
        model.set_table_likelihood(random_table(8, 91))
    else:
        model.set_binned_measurement(a_measurement(20, BIN_EDGES))


def refused(call, who, index, word):
    """call() fails with GF_ERR_INVALID_ARG through the Python wrapper, and the message names the call, the model and what it carries"""
    other = "binned" if word == "tabulated" else "tabulated"
    with pytest.raises(_lib.GolemHipError) as e:
        call()
    msg = str(e.value)
    assert e.value.code == INVALID and who + ":" in msg and "model %d now carries a %s" % (index, word) in msg and other not in msg, msg


def sampler_holds(smp):
    d = dict(chain=smp.chain, lnprobability=smp.lnprobability, pos=smp.state[0], lnp=smp.state[1], acceptance_fraction=smp.acceptance_fraction,
             fr=smp.postprocess()["fr"])
    return d, smp.iterations


def start_rows(width, n, seed):
    ps = paramset_of(width)
    rng = np.random.default_rng(seed)
    box = np.array(ps.ranges, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(n, width))
    p0[:, -1] = rng.uniform(-50.0, -42.0, n)
    return p0


@pytest.mark.parametrize("word", ["tabulated", "binned"])
@pytest.mark.parametrize("multi", [False, True], ids=["gf_sampler_create", "gf_sampler_create_multi"])
def test_a_sampler_refuses_a_model_that_gained_a_likelihood(multi, word):
    """20 steps of a Gaussian BSM sampler, then its model (chain 1's of two) is given a table or a binned measurement: set_state, run and
    run_to_host are refused, and chain, lnprob, state, iterations and acceptance are what they were; postprocess only propagates."""
    models = [open_model(7) for _ in range(2 if multi else 1)]
    changed = len(models) - 1
    try:
        p0 = np.stack([start_rows(7, 32, 40 + k) for k in range(len(models))])
        smp = mcmc_utils.DeviceEnsembleSampler(32, 7, models if multi else models[0], nchains=len(models), seed=5)
        smp.on_nonunitary = "-inf"
        try:
            smp.run_mcmc(p0 if multi else p0[0], 20)
            kept, iterations = sampler_holds(smp)
            assert iterations == 20 and np.all(np.isfinite(kept["lnp"]))
            gain(models[changed], word)
            refused(lambda: smp.run_mcmc(p0 if multi else p0[0], 5), "gf_sampler_set_state", changed, word)
            refused(lambda: smp.run_mcmc(None, 5), "gf_sampler_run", changed, word)
            refused(lambda: smp.run_mcmc_to_host(None, 5), "gf_sampler_run_to_host", changed, word)
            L = _lib.lib()
            assert L.gf_sampler_run(smp._h, 5, 1, 1) == INVALID and L.gf_sampler_set_state(smp._h, p0.ctypes.data_as(_lib._dp)) == INVALID
            now, iterations = sampler_holds(smp)
            assert iterations == 20
            for k in kept:
                assert TH.same_bits(now[k], kept[k]), k
            # ... and what the stored lnprob holds is not the model's lnprob any more: the reason for the refusal
            rows = smp._fetch(chain=True)[0][changed].reshape(-1, 7)
            assert not TH.same_values(bulk(models[changed], rows), smp._fetch(lnprob=True)[1][changed].reshape(-1))
        finally:
            smp.close()
    finally:
        for m in models:
            m.close()


@pytest.mark.parametrize("word", ["tabulated", "binned"])
def test_cube_runs_and_seed_sets_refuse_a_model_that_gained_a_likelihood(word):
    """A nested sampler and a maximiser, fresh and begun, and a gf_toys seed set over two Gaussian BSM models, the second of which gains a
    table or a binned measurement: every run and seed call is refused, results so far stay what they were, destroying works."""
    L = _lib.lib()
    models = [open_model(7), open_model(7)]
    ps = paramset_of(7)
    cols = np.arange(6, dtype=np.int32)
    bases = np.tile(np.array(ps.values, dtype=np.float64), (2, 1))
    kw = dict(on_nonunitary="-inf", run_ids=[0, 1])
    try:
        fresh_n = nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=13, tol=0.5, **kw)
        begun_n = nested.NestedSampler(models, cols, bases, nlive=64, batch=8, walks=10, seed=13, tol=0.5, **kw)
        fresh_s = P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, maxiter=100, **kw)
        begun_s = P.SimplexMaximizer(models, cols, bases, nstarts=1, nseed=256, seed=5, maxiter=100, **kw)
        toys = C.c_void_p()
        try:
            assert L.gf_toys_create((C.c_void_p * 2)(models[0]._h, models[1]._h), 2, 6, cols.ctypes.data_as(_lib._ip), bases.ctypes.data_as(_lib._dp), 64, 1,
                                    C.byref(toys)) == _lib.GF_OK
            assert L.gf_nested_run(begun_n._h, 8) == _lib.GF_ERR_UNSUPPORTED and L.gf_simplex_run(begun_s._h, 3) == _lib.GF_OK
            kept_n, kept_s = nested_snapshot(begun_n), simplex_snapshot(begun_s)
            gain(models[1], word)
            for s in (fresh_n, begun_n):
                refused(s.run, "gf_nested_run", 1, word)
            for s in (fresh_s, begun_s):
                refused(s.run, "gf_simplex_run", 1, word)
            nu = np.zeros(2, np.uint32)
            refused(lambda: _lib.check(L.gf_toys_seed(toys, nu.ctypes.data_as(C.POINTER(C.c_uint32))), "gf_toys_seed"), "gf_toys_seed", 1, word)
            same_nested_snapshot(nested_snapshot(begun_n), kept_n)
            same_simplex_snapshot(simplex_snapshot(begun_s), kept_s)
            assert np.array_equal(fresh_n.result()["niter"], [0, 0])          # nothing was launched or written
        finally:
            if toys.value:
                L.gf_toys_destroy(toys)
            for s in (fresh_n, begun_n, fresh_s, begun_s):
                s.close()
    finally:
        for m in models:
            m.close()


# ---- 6. the binned sampler: a measurement replaced between two runs ------------------------------------------------------------------------------
def test_a_measurement_replaced_between_two_runs_is_the_one_the_next_run_samples(oracle):
    """36 steps under one measurement, the model's measurement is replaced, 34 more: the second run is the numpy stretch move on the bulk
    lnprob of the new measurement from the first run's final state, the walkers holding the lnprob the device holds -- the old
    measurement's, not recomputed."""
    m, ps = binned_model(7, 6, Texture.OET)
    with m:
        p0 = scale_rows(ps, 32, np.random.default_rng(61), 6)[None]
        smp, ref = binned_run_against_reference(oracle, [m], False, p0, 36, seed=17, what="before the replacement")
        try:
            m.set_binned_measurement(a_measurement(20, BIN_EDGES, seed=6))
            smp.reset()
            smp.run_mcmc(None, 34)
            new = reference_stretch(oracle, m, ref["pos"], 34, 17, lnprob=bulk, full=True, iteration0=36, lnp0=ref["lnp"])
            stale = bulk(m, ref["pos"][0]) != ref["lnp"][0]
            assert stale.sum() > 16, "the replacement changes nothing: nothing was compared"
            assert_same_run(device_run(smp), new, "after the measurement was replaced")
        finally:
            smp.close()
