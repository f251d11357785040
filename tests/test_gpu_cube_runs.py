"""The nested sampler and the profile maximiser against the bulk kernel, bit for bit, at the theta the package reports.

Both work in the unit cube of their scanned columns and report theta = (hi - lo) u + lo formed on the host, the product and the sum each
rounded (NestedSampler.dead, SimplexMaximizer.cube_to_theta).  Their kernels must form the same theta (cube_to_theta, gf_cube_runs.hpp):
a map that fuses the two operations is one ulp off in a scanned coordinate on up to 40 per cent of the draws of a box that does not start
at 0, and a stored lnL then belongs to a neighbouring theta.  The sens and notebook boxes ([0, 1], [0, 2 pi], [-1, 1]) cannot tell the two
maps apart, so the posteriors here have offset boxes and priors that depend on those columns:

    P   PRIOR_ONLY, five nuisance columns, boxes [-5, 5], [0.1, 10], [0.26, 0.35], [-50, -30], [0, 1]
    S   SM_GAUSS, the notebook's six columns plus two nuisance columns, boxes [-5, 5] and [0.1, 10]
    B   flux-averaged BSM_GAUSS, texture OEU, dimension 6, the 12 columns of Cf.fr_paramsets, all scanned -- logLam too, over the whole
        window of SCALE_BOUNDARIES[6], which reaches the region where the reference's unitarity assert fails -- at 1, 4 and 16 lanes

Every test first shows that its own cube points can tell the maps apart (`told_apart`): the fused map is computed on the host with exact
rationals, at least 25 per cent of the points must have a scanned coordinate on which the two maps differ, and the bulk lnprob at the two
thetas must differ on a stated share of them.  That is a condition on the inputs; nothing of it comes from the kernels under test."""
import argparse
import os

import numpy as np
import pytest

from stretch_ref import fma
from golemflavor_amd import _lib, nested
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import profile_llh as P
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, PriorsCateg, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import Param, ParamSet

pytestmark = pytest.mark.gpu

NLIVE, BATCH, WALKS, TOL = 64, 8, 10, 0.5
MIN_POINTS = NLIVE + 8 * 20
MIN_COORD_SHARE = 0.25         # of the checked points: a scanned coordinate on which the fused and the unfused map differ
SEED_ITER = 0xFFFFFFFE         # gf_simplex.hip SX_SEED_ITER: the iteration word of the seeding draws


# ---- the posteriors --------------------------------------------------------------------------------------------------------------------
def nuisance(name, value, ranges, std=None, prior=None):
    return Param(name=name, value=value, ranges=ranges, std=std, prior=prior, tag=ParamTag.NUISANCE)


def p_paramset(sharp):
    """P.  `sharp` scales the widths: the runs of one sampler are not copies of each other."""
    g, lg = PriorsCateg.GAUSSIAN, PriorsCateg.LIMITEDGAUSS
    return ParamSet([nuisance("n_sym", 1.3, [-5., 5.], 0.2 * sharp, g),
                     nuisance("n_norm", 3.7, [0.1, 10.], 0.5 * sharp, lg),
                     nuisance("n_s12", 0.31, [0.26, 0.35], 0.008 * sharp, lg),
                     nuisance("n_scale", -41.3, [-50., -30.], 1.5 * sharp, g),
                     nuisance("n_flat", 0.4, [0., 1.])])


P_BASES = np.array([[1.21, 3.9, 0.3134, -40.7, 0.83],           # off the box centres (0, 5.05, 0.305, -40, 0.5)
                    [1.42, 3.3, 0.3071, -42.1, 0.17],
                    [1.1, 4.4, 0.3023, -41.9, 0.61]])


def s_paramset():
    """S: the notebook posterior with two nuisance columns behind it.  The [-5, 5] column's prior sits where |theta| < 2: there the sum
    of the map is exact and the fused map keeps bits the rounded product has lost, elsewhere in that box the two maps agree.  The models
    take offset 0 in place of the reference's -320, which would drown the priors' last bits."""
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    g = PriorsCateg.GAUSSIAN
    ps = ps.extend([nuisance("n_sym", 0.7, [-5., 5.], 0.05, g), nuisance("n_norm", 6.3, [0.1, 10.], 0.1, g)])
    return ps, fr_utils.angles_to_fr(asimov.values)


S_BASES = np.array([[0.301, 0.9571, 0.52, 3.7, 0.93, 0.07, 0.73, 6.37],
                    [0.312, 0.9559, 0.57, 4.4, 0.97, -0.04, 0.66, 6.22],
                    [0.295, 0.9566, 0.49, 2.9, 0.95, 0.02, 0.71, 6.31]])
S_SMEARING = (0.1, 0.2, 0.1)


def open_models(which):
    """The three runs' models (closed by the caller) and bases."""
    if which == "P":
        return [Model(compile_model(p_paramset(sh), "PRIOR_ONLY")) for sh in (1.0, 1.5, 1.0)], P_BASES
    ps, bf = s_paramset()
    return [Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=sm, offset=0.0)) for sm in S_SMEARING], S_BASES


# nscan = 1 (the [-5, 5] column: the only box that carries a one-column run past MIN_COORD_SHARE), a strict subset out of declaration
# order, every column
COLS = {"P": {"one": [0], "subset": [3, 0, 2], "all": [0, 1, 2, 3, 4]},
        "S": {"one": [6], "subset": [7, 2, 6], "all": [0, 1, 2, 3, 4, 5, 6, 7]}}
# the least share of the checked points whose bulk lnprob differs between the two thetas: half of the lowest share the bulk kernel gave
# over the test's runs (the tests' docstrings carry the measured shares)
MIN_LNPROB_SHARE = {("nested", "P", "one"): 0.23, ("nested", "P", "subset"): 0.27, ("nested", "P", "all"): 0.32,
                    ("nested", "S", "one"): 0.29, ("nested", "S", "subset"): 0.34, ("nested", "S", "all"): 0.30,
                    ("simplex", "P", "one"): 0.22, ("simplex", "P", "subset"): 0.25, ("simplex", "P", "all"): 0.30,
                    ("simplex", "S", "one"): 0.28, ("simplex", "S", "subset"): 0.36, ("simplex", "S", "all"): 0.21}


def b_args():
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=Texture.OEU,
                              binning=Cf.default_bin_edges(), injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


def open_b_models():
    """B: two runs, smearing 0.02 and 0.1; every column is scanned, logLam first.  Offset 0 as for S: under the reference's -320 every
    lnprob is a few hundred, and half of the last-bit differences the offset columns cause are rounded away."""
    args = b_args()
    asimov, ps = Cf.fr_paramsets(6, fr_utils.fr_to_angles(args.injected_ratio))
    ps["convNorm"].std = 0.02                      # 0.4 in the reference: lnprob would hardly see that column's last bit
    names = list(ps.names)
    sc = names.index("logLam")
    assert tuple(ps[sc].ranges) == tuple(Cf.SCALE_BOUNDARIES[6])
    cols = [sc] + [i for i in range(len(names)) if i != sc]
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    models = [Model(compile_model(ps, "BSM_GAUSS", bestfit_fr=bf, smearing=sm, source_ratio=args.source_ratio, texture=args.texture,
                                  dimension=args.dimension, binning=args.binning, offset=0.0)) for sm in (0.02, 0.1)]
    return models, cols, np.tile(np.array(ps.values, dtype=float), (2, 1))


class lanes:
    """GF_NESTED_LPW / GF_SIMPLEX_LPW set for the block and restored."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def close_all(models):
    for m in models:
        m.close()


# ---- what the tests share --------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def ulps(a, b):
    """the largest distance in units of the last place between finite values of the same sign"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(a[fin].view(np.int64) - b[fin].view(np.int64)).max()) if fin.any() else 0


def box(model, cols):
    return np.asarray(model.desc.lo)[cols], np.asarray(model.desc.hi)[cols]


def host_theta(model, cols, base, cube):
    """theta as the package reports it: the product and the sum each rounded"""
    lo, hi = box(model, cols)
    th = np.tile(np.asarray(base, dtype=float), (len(cube), 1))
    th[:, cols] = (hi - lo) * np.asarray(cube) + lo
    return th


def told_apart(model, cols, base, cube, what, min_lnprob_share=None):
    """The condition on the inputs: `cube` [n, nscan] are the points a test checks.  The fused map fma(hi - lo, u, lo) in exact rationals
    against the host's two roundings: at least MIN_COORD_SHARE of the points have a coordinate on which they differ, and the bulk lnprob
    of the two thetas differs on at least `min_lnprob_share` of the points.  Returns (share of points, share of lnprob values)."""
    cube = np.asarray(cube, dtype=float).reshape(-1, len(cols))
    lo, hi = box(model, cols)
    span = hi - lo
    unfused = span * cube + lo
    fused = np.array([[fma(float(span[k]), float(u[k]), float(lo[k])) for k in range(len(cols))] for u in cube])
    coord = np.any(unfused != fused, axis=1)
    th_u, th_f = host_theta(model, cols, base, cube), np.tile(np.asarray(base, dtype=float), (len(cube), 1))
    assert np.array_equal(th_u[:, cols], unfused)
    th_f[:, cols] = fused
    lp_u, st_u = model.lnprob(th_u, want_status=True)
    lp_f, st_f = model.lnprob(th_f, want_status=True)
    fin = (st_u == _lib.GF_ST_OK) & (st_f == _lib.GF_ST_OK) & np.isfinite(lp_u) & np.isfinite(lp_f)
    differ = fin & (lp_u != lp_f)
    share_c, share_l = float(coord.mean()), float(differ.sum()) / len(cube)
    print("%s: %d cube points, %d (%.3f) with a coordinate the fused map rounds otherwise, bulk lnprob of the two thetas differs on %d "
          "(%.3f), by up to %d ulps" % (what, len(cube), coord.sum(), share_c, differ.sum(), share_l, ulps(lp_u[differ], lp_f[differ])))
    assert share_c >= MIN_COORD_SHARE, (what, share_c)
    assert not np.any(differ & ~coord)
    if min_lnprob_share is not None:
        assert share_l >= min_lnprob_share, (what, share_l, min_lnprob_share)
    return share_c, share_l


def check_dead_points(s, res, r, model, what, problems):
    """Run r's dead and final live points against the bulk kernel at the theta dead() reports; what does not hold is added to `problems`,
    so that a failing test names every run.  Returns dead()'s dict."""
    d = s.dead(r)
    lp, st = model.lnprob(d["theta"], want_status=True)
    assert same_bits(d["theta"], host_theta(model, s.cols, s.bases[r], d["cube"]))
    ok = st == _lib.GF_ST_OK
    assert len(lp) >= MIN_POINTS and ok.sum() >= MIN_POINTS, (what, len(lp), ok.sum())
    diff = d["lnl"][ok].view(np.int64) != lp[ok].view(np.int64)
    print("%s run %d: %d points, %d status OK, %d differ from the bulk lnprob, largest %d ulps"
          % (what, r, len(lp), ok.sum(), diff.sum(), ulps(d["lnl"][ok], lp[ok])))
    if not np.all(d["lnl"][~ok] == -np.inf):
        problems.append("%s run %d: a point the bulk kernel refuses has a stored lnL" % (what, r))
    if not same_bits(d["lnl"][ok], lp[ok]):
        problems.append("%s run %d: %d of %d stored lnL are not the bulk lnprob of dead()'s theta, by up to %d ulps"
                        % (what, r, diff.sum(), ok.sum(), ulps(d["lnl"][ok], lp[ok])))
    if not same_bits(res["max_lnl"][r:r + 1], [lp[ok].max()]):
        problems.append("%s run %d: max_lnl %r, the largest bulk lnprob %r" % (what, r, res["max_lnl"][r], lp[ok].max()))
    return d


def run_nested(models, cols, bases, seed):
    s = nested.NestedSampler(models, cols, bases, nlive=NLIVE, batch=BATCH, walks=WALKS, seed=seed, tol=TOL, on_nonunitary="-inf")
    try:
        return s, s.run()
    except BaseException:
        s.close()
        raise


class BulkF:
    """f(u) = -lnprob(theta(u)) by the bulk kernel at the host's theta, for nelder_mead_speculative; keeps the points it was given"""

    def __init__(self, model, cols, base):
        self.model, self.cols, self.base, self.seen = model, cols, base, []

    def __call__(self, U):
        U = np.asarray(U, dtype=float)
        self.seen.append(U.copy())
        lp, st = self.model.lnprob(host_theta(self.model, self.cols, self.base, U), want_status=True)
        bad = st == _lib.GF_ST_NON_UNITARY
        return np.where(bad | ~(lp > -np.inf), np.inf, -lp), bad


def host_seeds(oracle, model, cols, base, seed, run_id, nseed, nstarts):
    """The maximiser's seeding restated: `nseed` uniform cube points of Philox counter (run id, SEED_ITER, point, pair of coordinates),
    their bulk lnprob at the host's theta, a non-unitary or NaN point -inf; the `nstarts` best finite ones, lnL descending then index
    ascending.  Returns (their cube points, the non-unitary count)."""
    n = len(cols)
    key = (seed & 0xFFFFFFFF, ((seed >> 32) ^ (run_id >> 32)) & 0xFFFFFFFF)
    u = np.empty((nseed, n))
    for i in range(nseed):
        for p in range((n + 1) // 2):
            q = oracle.philox4x32_10((run_id & 0xFFFFFFFF, SEED_ITER, i, p), key)
            u[i, 2 * p] = ((q[0] >> 5) * 67108864.0 + (q[1] >> 6)) / 9007199254740992.0
            if 2 * p + 1 < n:
                u[i, 2 * p + 1] = ((q[2] >> 5) * 67108864.0 + (q[3] >> 6)) / 9007199254740992.0
    lp, st = model.lnprob(host_theta(model, cols, base, u), want_status=True)
    bad = st == _lib.GF_ST_NON_UNITARY
    lp = np.where(bad | np.isnan(lp), -np.inf, lp)
    order = np.lexsort((np.arange(nseed), -lp))[:nstarts]
    return u[order[lp[order] > -np.inf]], int(bad.sum())


def check_maximiser(oracle, models, cols, bases, user_starts, what, maxiter, seed=5, nseed=256, nstarts=2, min_lnprob_share=None):
    """One maximiser over `models`: `nstarts` seeded starts and the caller's per run, adaptive, one restart.  Every start's final value
    and the run's maximum against the bulk kernel at the host's theta, and every start -- the seeded ones from the host's own restatement
    of the seeding -- against nelder_mead_speculative fed by the bulk kernel.  Returns run()'s result.

    `maxiter` is to end the starts well before they converge: at an interior maximum the gradient is zero and lnprob does not see the last
    bit of theta, so a converged start has the same value under either map."""
    cols = list(cols)
    problems = []
    with P.SimplexMaximizer(models, cols, bases, nstarts=nstarts, nseed=nseed, seed=seed, starts=user_starts, maxiter=maxiter,
                            adaptive=True, restarts=1, on_nonunitary="-inf") as s:
        res = s.run()
        for r, m in enumerate(models):
            dev = s.starts(r)
            used = int(res["nstarts"][r])
            assert used == nstarts + user_starts.shape[1], (what, r, used)
            th = np.tile(s.bases[r], (used, 1))
            th[:, cols] = s.cube_to_theta(r, dev["cube"][:used])
            lp, st = m.lnprob(th, want_status=True)
            ok = (st == _lib.GF_ST_OK) & (lp > -np.inf)
            fun = dev["lnl"][:used]
            print("%s run %d: %d starts, %d finite, %d differ from the bulk lnprob, largest %d ulps"
                  % (what, r, used, ok.sum(), np.sum(fun[ok] != lp[ok]), ulps(fun[ok], lp[ok])))
            assert ok.sum() >= nstarts, (what, r)
            if not (same_bits(fun[ok], lp[ok]) and np.all(fun[~ok] == -np.inf)):
                problems.append("%s run %d: -fun of %d of %d starts is not the bulk lnprob of cube_to_theta(cube), by up to %d ulps"
                                % (what, r, np.sum(fun[ok] != lp[ok]), used, ulps(fun[ok], lp[ok])))
            if not same_bits(m.lnprob(res["argmax_theta"][r:r + 1])[0], res["max_lnl"][r:r + 1]):
                problems.append("%s run %d: max_lnl is not the bulk lnprob of argmax_theta" % (what, r))
            if not same_bits(res["max_lnl"][r:r + 1], [fun.max()]):
                problems.append("%s run %d: max_lnl is not the best start's value" % (what, r))
            f = BulkF(m, cols, s.bases[r])
            seeds, counted = host_seeds(oracle, m, cols, s.bases[r], seed, r, nseed, nstarts)
            assert len(seeds) == nstarts
            off = 0
            for j, x0 in enumerate(list(seeds) + list(user_starts[r])):
                h = P.nelder_mead_speculative(f, x0, adaptive=True, maxiter=maxiter, restarts=1, on_nonunitary="-inf")
                off += not (np.array_equal(dev["cube"][j], h["x"]) and same_bits([-dev["lnl"][j]], [h["fun"]]) and
                            dev["nit"][j] == h["nit"] and dev["nfev"][j] == h["nfev"])
                counted += h["nonunitary"]
            if off:
                problems.append("%s run %d: %d of %d trajectories are not the host restatement's on the bulk kernel" % (what, r, off, used))
            if res["nonunitary"][r] != counted:
                problems.append("%s run %d: %d non-unitary points counted, the host counts %d" % (what, r, res["nonunitary"][r], counted))
            told_apart(m, cols, s.bases[r], np.concatenate(f.seen)[:1500], "%s run %d" % (what, r), min_lnprob_share)
    assert not problems, "\n".join(problems)
    return res


# ---- the nested sampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one", "subset", "all"])
@pytest.mark.parametrize("which", ["P", "S"])
def test_nested_points_equal_the_bulk_lnprob(which, shape):
    """Three runs of P or S over one column, a strict subset given out of declaration order, and every column: the stored lnL of every dead
    and final live point is Model.lnprob of dead()'s theta bit for bit, and max_lnl is the largest of them.  The S run over every column
    also holds posterior_rows to dead()'s theta.

    Share of the checked points (288 to 1336 a run) whose bulk lnprob tells the two maps apart, as the bulk kernel gave it for the three
    runs (MIN_LNPROB_SHARE holds half of the lowest); in brackets the share with a coordinate on which the maps differ:
        P one     0.535 0.479 0.509  (0.63 0.61 0.61)      S one     0.606 0.612 0.588  (0.68 0.66 0.63)
        P subset  0.627 0.550 0.579  (0.73 0.66 0.69)      S subset  0.718 0.686 0.754  (0.81 0.79 0.83)
        P all     0.687 0.656 0.648  (0.82 0.80 0.80)      S all     0.624 0.620 0.610  (0.80 0.79 0.81)
    With the fused map in the kernels these are the shares of stored lnL that were not the bulk lnprob of dead()'s theta (154 of 288
    to 834 of 1336 points a run, by up to 6144 ulps)."""
    models, bases = open_models(which)
    cols = COLS[which][shape]
    try:
        s, res = run_nested(models, cols, bases, seed=11)
        try:
            problems = []
            for r, m in enumerate(models):
                what = "nested %s %s" % (which, shape)
                d = check_dead_points(s, res, r, m, what, problems)
                told_apart(m, cols, s.bases[r], d["cube"], "%s run %d" % (what, r), MIN_LNPROB_SHARE["nested", which, shape])
            assert not problems, "\n".join(problems)
            if which == "S" and shape == "all":
                rows, index = s.posterior_rows(200, return_index=True)
                d = s.dead(1)
                assert np.all(index[1] >= 0) and len(np.unique(index[1])) >= 20
                assert same_bits(rows[1], d["theta"][index[1]])
        finally:
            s.close()
    finally:
        close_all(models)


@pytest.mark.parametrize("lpw", ["1", "4", "16"])
def test_nested_points_equal_the_bulk_lnprob_flux_averaged(lpw):
    """B at 1, 4 and 16 lanes per point: as above, and both runs meet proposals the reference would have raised on, so parked proposals
    were settled.  The bulk lnprob tells the two maps apart on 0.220 and 0.182 of the two runs' 2576 and 1200 points (0.59 and 0.63 have
    a coordinate on which the maps differ); the floor asserted is 0.05.  With the fused map in the kernels 459 of 2213 and 245 of 1238
    stored lnL were not the bulk lnprob of dead()'s theta, by up to 2640 ulps, at every lane count."""
    with lanes("GF_NESTED_LPW", lpw):
        models, cols, bases = open_b_models()
        try:
            s, res = run_nested(models, cols, bases, seed=13)
            try:
                problems = []
                for r, m in enumerate(models):
                    d = check_dead_points(s, res, r, m, "nested B lpw %s" % lpw, problems)
                    told_apart(m, cols, s.bases[r], d["cube"], "nested B lpw %s run %d" % (lpw, r), 0.05)
                assert not problems, "\n".join(problems)
                assert np.all(res["nonunitary"] > 0), res["nonunitary"]
            finally:
                s.close()
        finally:
            close_all(models)


# ---- the maximiser ---------------------------------------------------------------------------------------------------------------------
def user_starts(which, nruns, cols, seed, k=6):
    """k cube points per run where every offset box of P, S and B sees the map ([-5, 5]: |theta| < 2).  S: the notebook's columns start
    within 0.03 of the planted maximum (the prior centres, the source (1, 0, 0)); far from it lnprob is some 1e4 and its last bit too
    coarse for most of what the nuisance columns' last bits change."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.3, 0.7, size=(nruns, k, len(cols)))
    if which == "S":
        ps, _ = s_paramset()
        box = np.array(ps.ranges, dtype=float)
        star = np.array(ps.values, dtype=float)
        star[4:6] = fr_utils.fr_to_angles((1., 0., 0.))
        ustar = (star - box[:, 0]) / (box[:, 1] - box[:, 0])
        for i, c in enumerate(cols):
            if c < 6:
                u[:, :, i] = np.clip(ustar[c], 0.05, 0.95) + rng.uniform(-0.03, 0.03, size=(nruns, k))
    return u


MAXITER = {"one": 3, "subset": 6, "all": 12}         # the starts end by it, far from converged


@pytest.mark.parametrize("shape", ["one", "subset", "all"])
@pytest.mark.parametrize("which", ["P", "S"])
def test_maximiser_values_and_trajectories_equal_the_bulk_lnprob(oracle, which, shape):
    """Three runs of P or S, two seeded and six given starts each: -fun of every start is Model.lnprob at cube_to_theta of its cube point,
    max_lnl is Model.lnprob(argmax_theta), and every trajectory (cube, fun, nit, nfev) is nelder_mead_speculative's on the bulk kernel --
    the seeded starts from the seeding restated on the host, so a seed's value counts through its rank.

    Share of the points the trajectories evaluate (160 to 848 a run) whose bulk lnprob tells the two maps apart, as the bulk kernel gave
    it for the three runs (MIN_LNPROB_SHARE holds half of the lowest); in brackets the share with a coordinate on which the maps differ:
        P one     0.500 0.463 0.444  (0.58 0.70 0.61)      S one     0.562 0.581 0.562  (0.59 0.64 0.59)
        P subset  0.573 0.633 0.513  (0.69 0.75 0.65)      S subset  0.742 0.758 0.729  (0.82 0.85 0.82)
        P all     0.745 0.603 0.686  (0.84 0.79 0.84)      S all     0.654 0.658 0.421  (0.82 0.83 0.75)
    With the fused map in the kernels up to 7 of a run's 8 starts had a -fun that was not the bulk lnprob of their theta, by up to 992
    ulps, and had left the host restatement's trajectory; every one of the six cases failed."""
    models, bases = open_models(which)
    cols = COLS[which][shape]
    try:
        check_maximiser(oracle, models, cols, bases, user_starts(which, 3, cols, 21), "simplex %s %s" % (which, shape), MAXITER[shape],
                        min_lnprob_share=MIN_LNPROB_SHARE["simplex", which, shape])
    finally:
        close_all(models)


@pytest.mark.parametrize("lpw", ["1", "4", "16"])
def test_maximiser_values_and_trajectories_equal_the_bulk_lnprob_flux_averaged(oracle, lpw):
    """B at 1, 4 and 16 lanes per point, one seeded and two given starts a run, 100 iterations of 12 columns: as above; the seeding meets
    points the reference would have raised on, candidates are parked and settled, and the non-unitary count is the seeding's plus those of
    the points scipy evaluates.  The bulk lnprob tells the two maps apart on 0.167 and 0.326 of the 1500 trajectory points checked per
    run; the floor asserted is 0.05."""
    with lanes("GF_SIMPLEX_LPW", lpw):
        models, cols, bases = open_b_models()
        try:
            starts = user_starts("B", 2, cols, 23, k=2)
            starts[:, :, 0] = [[0.2, 0.45], [0.3, 0.5]]                 # logLam: inside the window where lnprob is finite
            res = check_maximiser(oracle, models, cols, bases, starts, "simplex B lpw %s" % lpw, 100, nstarts=1, min_lnprob_share=0.05)
            print("simplex B lpw %s: non-unitary %s, parked %s" % (lpw, res["nonunitary"], res["parked"]))
            assert np.all(res["nonunitary"] > 0) and res["parked"].sum() > 0, (res["nonunitary"], res["parked"])
        finally:
            close_all(models)
