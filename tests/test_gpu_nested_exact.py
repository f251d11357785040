"""The device nested sampler (gf_nested.hip) against independent references, on the GPU:

  * ln Z of PRIOR_ONLY posteriors against the closed form (a product of 1-D quadratures of the oracle's lnprior);
  * every dead and final live point: cube in [0, 1], lnL = the oracle's lnprob at theta, the dead sequence non-decreasing, the
    final live set above the last dead point, lnw = the host formula, nevals = nlive + the counted evaluations;
  * a step replay: k_ns_select / k_ns_walk / k_ns_commit restated in numpy (Philox4x32-10 on the device's counters, the oracle's
    lnprob), run from the device's own state every 4 iterations and compared with what the device did next -- at the edges of
    k_ns_select (nlive 4096, nlive not a power of two, batch 1, batch nlive - 1, one and 16 dimensions, several runs, a run past
    128 iterations), on every walk instance and lanes-per-walker choice, on the zero-likelihood plateau of the sens posterior and
    on a posterior whose proposals are parked and settled by the emulated-x87 team (k_stretch_settle<NESTED>)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import nested
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, PriorsCateg, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import Param, ParamSet

pytestmark = pytest.mark.gpu

REL = 1e-10                  # lnprob against the oracle (test_gpu_parity: the bar of every mode)
CUBE_TOL = 1e-12
MARGIN = 1e-9                # a host decision this close to L* or to the cube wall may differ from the device's
NS_INIT_ITER = 0xFFFFFFFF
NS_START_STEP = 0xFFFFFFFF
M32 = np.uint64(0xFFFFFFFF)


# ---- models: the device's and the oracle's from one description ------------------------------------------------------------
def prior_paramset(ndim):
    """ndim columns with LIMITEDGAUSS, UNIFORM and GAUSSIAN priors in turn, on boxes of different widths and offsets."""
    kinds = [PriorsCateg.LIMITEDGAUSS, PriorsCateg.UNIFORM, PriorsCateg.GAUSSIAN]
    ps = []
    for i in range(ndim):
        lo, w = -1.0 + 0.37 * i, 1.0 + 0.25 * (i % 4)
        ps.append(Param(name="x%d" % i, value=lo + w * (0.35 + 0.03 * (i % 5)), ranges=[lo, lo + w], std=w * (0.12 + 0.02 * (i % 3)),
                        prior=kinds[i % 3], tag=ParamTag.NUISANCE))
    return ParamSet(ps)


def sens_spec(scale, texture=Texture.OET, dimension=6):
    """The d = 6 sens posterior (source (0, 1, 0), smearing 0.02) with the scale fixed: (paramset, compile kwargs)."""
    asimov, ps = Cf.sens_paramsets(dimension, (1., 1., 1.))
    sp = nested._scale_paramset(ps, float(scale))
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    kw = dict(bestfit_fr=bf, smearing=0.02, source_ratio=fr_utils.normalize_fr((0., 1., 0.)), texture=texture,
              dimension=dimension, binning=Cf.default_bin_edges())
    return sp, kw


class Problem:
    """nruns posteriors of one mode, the scanned columns and their bases, as device models and oracle models."""

    def __init__(self, oracle, specs, mode, cols):
        self.mode = mode
        self.cols = np.asarray(cols, dtype=np.int32)
        self.models, self.oms, self.bases, self.lo, self.hi = [], [], [], [], []
        for ps, kw in specs:
            okw = dict(kw)
            if "texture" in okw:
                okw["texture"] = okw["texture"].name
            self.models.append(Model(compile_model(ps, mode, **kw)))
            self.oms.append(oracle.make_model(ps, mode, **okw))
            self.bases.append(np.array(ps.values, dtype=np.float64))
            r = np.array(ps.ranges, dtype=np.float64)
            self.lo.append(r[:, 0])
            self.hi.append(r[:, 1])

    def theta(self, r, u):
        th = np.tile(self.bases[r], (len(u), 1))
        lo, hi = self.lo[r][self.cols], self.hi[r][self.cols]
        th[:, self.cols] = (hi - lo) * u + lo
        return th

    def lnprob(self, oracle, r, u):
        """The oracle's lnprob at theta(u) and its status; what the sampler makes of them (non-unitary and NaN: -inf)."""
        lp, st = oracle.lnprob_batch(self.oms[r], self.theta(r, u), want_status=True)
        return lp, st

    def close(self):
        for m in self.models:
            m.close()


def prior_problem(oracle, ndim, nscan, nruns=1):
    return Problem(oracle, [(prior_paramset(ndim), dict(flat_llh=0.0)) for _ in range(nruns)], "PRIOR_ONLY", list(range(nscan)))


# ---- closed form -------------------------------------------------------------------------------------------------------------
def closed_form_lnz(oracle, prob, r, n=200001):
    """Z = int over the scanned cube of exp(lnprior(theta(u))) du.  lnprior is a sum over columns, so Z is the product over the
    scanned columns of 1-D midpoint quadratures of the oracle's lnprior along that column, the others held at a reference
    point, times exp(lnprior(reference)) over the 1-D factors' overlap."""
    om = prob.oms[r]
    ref = prob.bases[r].copy()
    lp0 = oracle.lnprob_batch(om, ref[None, :])[0]
    total = lp0
    u = (np.arange(n) + 0.5) / n
    for k, c in enumerate(prob.cols):
        th = np.tile(ref, (n, 1))
        th[:, c] = (prob.hi[r][c] - prob.lo[r][c]) * u + prob.lo[r][c]
        lp = oracle.lnprob_batch(om, th)
        m = lp.max()
        total += m + math.log(np.mean(np.exp(lp - m))) - lp0
    return total


def check_points(oracle, prob, s, res, r):
    """Every dead and final live point of run r."""
    d = s.dead(r)
    nd, K, B = d["ndead"], s.nlive, s.batch
    assert nd == res["niter"][r] * B
    cube, lnl, lnw = d["cube"], d["lnl"], d["lnw"]
    assert np.all((cube >= 0.0) & (cube <= 1.0))
    lp, st = prob.lnprob(oracle, r, cube)
    ref = np.where((st == _lib.GF_ST_NON_UNITARY) | np.isnan(lp), -np.inf, lp)
    assert np.array_equal(np.isinf(lnl), np.isinf(ref)), r
    fin = np.isfinite(ref)
    assert np.all(np.abs(lnl[fin] - ref[fin]) <= REL * np.maximum(np.abs(ref[fin]), 1.0)), r
    dead = lnl[:nd]
    assert np.all(dead[1:] >= dead[:-1]), r                                 # over the whole run, not only in a batch
    if nd:
        assert np.all(lnl[nd:] >= dead[-1]), r
    seq = nested.nlive_sequence(dead, K, B)
    dx = 1.0 / seq.astype(np.float64)
    lnx = np.concatenate([[0.0], -np.cumsum(dx)])
    want = dead + lnx[:-1] + np.log(-np.expm1(-dx))
    fw = np.isfinite(want)
    assert np.array_equal(np.isinf(lnw[:nd]), ~fw), r
    assert np.all(np.abs(lnw[:nd][fw] - want[fw]) <= 1e-12 * np.maximum(np.abs(want[fw]), 1.0)), r
    wl = lnx[-1] - math.log(K) + lnl[nd:]
    fl = np.isfinite(wl)
    assert np.all(np.abs(lnw[nd:][fl] - wl[fl]) <= 1e-12 * np.maximum(np.abs(wl[fl]), 1.0)), r
    return d


@pytest.mark.parametrize("ndim,nscan", [(1, 1), (2, 2), (12, 11), (16, 16)])
def test_prior_only_evidence_matches_closed_form(oracle, ndim, nscan):
    prob = prior_problem(oracle, ndim, nscan, nruns=2)
    try:
        # 25 walk steps (the default) decorrelate a replacement from its start in a few dimensions; 11 and 16 need more
        walks = 25 if nscan <= 2 else 100
        with nested.NestedSampler(prob.models, prob.cols, np.stack(prob.bases), nlive=800, walks=walks, seed=5) as s:
            res = s.run()
            for r in range(2):
                exact = closed_form_lnz(oracle, prob, r)
                sig = res["lnz_err"][r]
                print("D=%d run %d: ln Z %.4f +- %.4f, closed form %.4f (%d iterations)" % (nscan, r, res["lnz"][r], sig, exact,
                                                                                       res["niter"][r]))
                assert sig > 0 and abs(res["lnz"][r] - exact) < 4 * sig, (r, res["lnz"][r], exact, sig)
                check_points(oracle, prob, s, res, r)
                host = nested.evidence_from_dead(s.dead(r)["lnl"][:res["niter"][r] * s.batch],
                                                 nested.nlive_sequence(s.dead(r)["lnl"][:res["niter"][r] * s.batch], s.nlive, s.batch),
                                                 live_lnl=s.dead(r)["lnl"][res["niter"][r] * s.batch:])
                assert abs(host["lnz"] - res["lnz"][r]) <= 1e-12 * abs(res["lnz"][r]) + 1e-12
                assert abs(host["lnz_err"] - res["lnz_err"][r]) <= 1e-12 * res["lnz_err"][r]
    finally:
        prob.close()


# ---- the step replay -----------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (gf_propose.hpp philox_block)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        m0 = np.uint64(0xD2511F53) * c0
        m1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (m1 >> np.uint64(32)) ^ c1 ^ k0, m1 & M32, (m0 >> np.uint64(32)) ^ c3 ^ k1, m0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def uniform2(seed, rid, it, slot, step):
    """gf_nested.hip ns_uniform2: two 53-bit uniforms of counter (run id, iteration, slot, step), key (seed, seed_hi ^ id_hi)."""
    q = philox(np.uint64(rid & 0xFFFFFFFF), np.uint64(it & 0xFFFFFFFF), slot, step, np.uint64(seed & 0xFFFFFFFF),
               np.uint64(((seed >> 32) ^ (rid >> 32)) & 0xFFFFFFFF))
    f = lambda hi, lo: ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) \
        / 9007199254740992.0
    return f(q[0], q[1]), f(q[2], q[3])


def test_numpy_philox_matches_the_oracle(oracle):
    rng = np.random.default_rng(0)
    for _ in range(50):
        c = [int(x) for x in rng.integers(0, 2 ** 32, 4)]
        k = [int(x) for x in rng.integers(0, 2 ** 32, 2)]
        got = philox(*[np.uint64(x) for x in c + k])
        assert tuple(int(x) for x in got) == oracle.philox4x32_10(c, k)


def chol(cov):
    """k_ns_select's Cholesky factor: a degenerate direction keeps sqrt(1e-24)."""
    D = cov.shape[0]
    L = np.zeros((D, D))
    for p in range(D):
        for q in range(p + 1):
            s = cov[p, q] - np.dot(L[p, :q], L[q, :q])
            L[p, q] = math.sqrt(s if s > 1e-24 else 1e-24) if p == q else s / L[q, q]
    return L


class Replay:
    """The host restatement of one run's iterations.  State: the live set (cube, lnL), ln Z, ln X, the plateau count, the step
    scale, the iteration and the evaluation count."""

    def __init__(self, oracle, prob, r, rid, seed, K, B, walks, tol):
        self.O, self.prob, self.r, self.rid, self.seed = oracle, prob, r, rid, seed
        self.K, self.B, self.walks, self.tol = K, B, walks, tol
        self.D = len(prob.cols)
        self.close_calls = []                     # (iteration, kind, margin)
        self.band = 0                             # evaluated proposals whose unitarity residual lies in (1e-9, 1e-5)
        self.nonunit = 0
        self.resynced = False                     # a close decision made the replay take the device's state mid-run

    def lnl(self, u):
        lp, st = self.prob.lnprob(self.O, self.r, u)
        bad = (st == _lib.GF_ST_NON_UNITARY)
        self.nonunit += int(bad.sum())
        if self.prob.mode == "BSM_GAUSS" and len(u):
            res = self.O.unitarity_residual_batch(self.prob.oms[self.r], self.prob.theta(self.r, u))
            self.band += int(np.sum((res > 1e-9) & (res < 1e-5)))
        return np.where(bad | np.isnan(lp), -np.inf, lp), bad

    def init(self):
        K, D = self.K, self.D
        u = np.empty((K, D))
        i = np.arange(K, dtype=np.uint64)
        for p in range((D + 1) // 2):
            v0, v1 = uniform2(self.seed, self.rid, NS_INIT_ITER, i, np.uint64(p))
            u[:, 2 * p] = v0
            if 2 * p + 1 < D:
                u[:, 2 * p + 1] = v1
        self.live_u = u
        self.live_l, _ = self.lnl(u)
        self.lnz, self.lnx, self.nplat, self.scale, self.it, self.nevals, self.done = -math.inf, 0.0, 0, 1.0, 0, K, False

    def load(self, s, res, scale, lnx):
        """The device's state of run r (between iterations)."""
        d = s.dead(self.r)
        nd = d["ndead"]
        self.live_u, self.live_l = d["cube"][nd:].copy(), d["lnl"][nd:].copy()
        self.lnz, self.lnx, self.scale = float(res["lnz"][self.r]), float(lnx[self.r]), float(scale[self.r])
        self.it, self.nevals = int(res["niter"][self.r]), int(res["nevals"][self.r])
        self.nplat = int(np.sum(d["lnl"][:nd] == -np.inf))
        self.done = False

    def near(self, kind, margin):
        if margin < MARGIN:
            self.close_calls.append((self.it, kind, margin))
            if len(self.close_calls) <= 5:                 # logged; a collapsed live set (batch nlive - 1) has hundreds
                print("close decision: run %d iteration %d, %s margin %.3g" % (self.r, self.it, kind, margin))

    def step(self):
        """One iteration, or the stop; returns (dead lnL [B], dead cube [B, D]) or None at the stop."""
        K, B, D = self.K, self.B, self.D
        key = np.where(np.isnan(self.live_l), -np.inf, self.live_l)
        order = np.lexsort((np.arange(K), key))
        lmax = key[order[-1]]
        if self.lnz > -math.inf and lmax > -math.inf:
            self.near("tolerance", abs(np.logaddexp(self.lnz, lmax + self.lnx) - self.lnz - self.tol))
        if lmax == -math.inf or (self.lnz > -math.inf and np.logaddexp(self.lnz, lmax + self.lnx) - self.lnz < self.tol):
            self.done = True
            return None
        rem = order[:B]
        for j, i in enumerate(rem):
            plat = key[i] == -math.inf
            dx = 1.0 / (K - self.nplat if plat else K - j)
            self.lnz = nested._logaddexp(self.lnz, key[i] + self.lnx + math.log(-math.expm1(-dx)))
            self.lnx -= dx
            self.nplat += int(plat)
        dead = (key[rem].copy(), self.live_u[rem].copy())
        lstar = key[order[B - 1]]
        surv = order[B:]
        x = self.live_u[surv]
        mean = x.mean(axis=0)
        cov = (x - mean).T @ (x - mean) / (len(surv) - 1) if len(surv) > 1 else np.zeros((D, D))
        L = chol(cov)
        first = B + int(np.searchsorted(key[surv], lstar, side="right"))
        if first == K:
            first = B
        j = np.arange(B, dtype=np.uint64)
        v0, _ = uniform2(self.seed, self.rid, self.it, j, np.uint64(NS_START_STEP))
        m = np.minimum(first + (v0 * (K - first)).astype(np.int64), K - 1)
        wu, wl = self.live_u[order[m]].copy(), key[order[m]].copy()
        acc = ev = 0
        live = np.ones(B, dtype=bool)             # walkers whose replay is still trusted
        for st in range(self.walks):
            z = np.empty((B, D))
            for p in range((D + 1) // 2):
                a, b = uniform2(self.seed, self.rid, self.it, j, np.uint64((p << 24) | st))
                rad = np.sqrt(-2.0 * np.log(1.0 - a))
                z[:, 2 * p] = rad * np.cos(2.0 * np.pi * b)
                if 2 * p + 1 < D:
                    z[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * b)
            u = wu + self.scale * (z @ L.T)
            inside = np.all((u >= 0.0) & (u <= 1.0), axis=1)
            wall = np.min(np.minimum(np.abs(u), np.abs(u - 1.0)), axis=1)
            for k in np.nonzero(live & (wall < MARGIN))[0]:
                self.near("cube wall", wall[k])
            idx = np.nonzero(inside)[0]
            lq, bad = self.lnl(u[idx])
            ev += len(idx)
            marg = np.abs(lq - lstar) / max(1.0, abs(lstar)) if lstar > -math.inf else np.full(len(idx), np.inf)
            for k in np.nonzero(live[idx] & ~bad & (marg < MARGIN))[0]:
                self.near("L*", marg[k])
            ok = ~bad & (lq > lstar)
            wu[idx[ok]] = u[idx[ok]]
            wl[idx[ok]] = lq[ok]
            acc += int(ok.sum())
        self.live_u[rem] = wu
        self.live_l[rem] = wl
        s = self.scale * math.exp(2.0 * (acc / (B * self.walks) - 0.5))
        self.scale = min(max(s, 1e-6), 10.0)
        self.nevals += ev
        self.it += 1
        return dead


def _run_to(L, s, it):
    rc = L.gf_nested_run(s._h, int(it))
    assert rc in (_lib.GF_OK, _lib.GF_ERR_UNSUPPORTED), rc
    return rc


def _state(s):
    L = _lib.lib()
    fn = L.gf_internal_nested_state
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    sc, lx = np.zeros(s.nruns), np.zeros(s.nruns)
    _lib.check(fn(s._h, sc.ctypes.data_as(C.POINTER(C.c_double)), lx.ctypes.data_as(C.POINTER(C.c_double))),
               "gf_internal_nested_state")
    return sc, lx


def replay_and_compare(oracle, prob, K, B, walks, blocks, seed=3, run_ids=None, on_nonunitary="raise", lpw=None, tol=0.01,
                       min_iter=0):
    """Run the device sampler 4 iterations at a time; before each block load every run's device state into its replay, replay
    the block and compare.  Returns the replays."""
    R = len(prob.models)
    ids = np.arange(R, dtype=np.uint64) * 7 + 1 if run_ids is None else np.asarray(run_ids, dtype=np.uint64)
    old = os.environ.get("GF_NESTED_LPW")
    if lpw is not None:
        os.environ["GF_NESTED_LPW"] = str(lpw)
    s = nested.NestedSampler(prob.models, prob.cols, np.stack(prob.bases), nlive=K, batch=B, walks=walks, seed=seed, tol=tol,
                             on_nonunitary=on_nonunitary, run_ids=ids)
    L = _lib.lib()
    reps = [Replay(oracle, prob, r, int(ids[r]), seed, K, B, walks, tol) for r in range(R)]
    compared = 0
    try:
        for rp in reps:
            rp.init()
        for blk in range(blocks):
            rc = _run_to(L, s, 4 * (blk + 1))
            res = s.result()
            scale, lnx = _state(s)
            for r, rp in enumerate(reps):
                if rp.done:
                    continue
                n0 = len(rp.close_calls)
                it0 = rp.it
                deads = []
                while rp.it < res["niter"][r]:
                    deads.append(rp.step())
                    assert deads[-1] is not None, (r, rp.it)
                if res["niter"][r] < 4 * (blk + 1):         # the device stopped this run: so must the replay
                    assert rp.step() is None or len(rp.close_calls) > n0, (r, rp.it)
                    rp.done = True
                d = s.dead(r)
                nd = d["ndead"]
                # a decision the host cannot call: the removals up to its iteration still match, nothing after it
                last = min(c[0] for c in rp.close_calls[n0:]) if len(rp.close_calls) > n0 else None
                for t, (dl, du) in enumerate(deads):
                    if last is not None and it0 + t > last:
                        break
                    rows = slice((it0 + t) * B, (it0 + t + 1) * B)
                    assert np.array_equal(np.isinf(d["lnl"][rows]), np.isinf(dl)), (r, it0 + t)
                    f = np.isfinite(dl)
                    assert np.all(np.abs(d["lnl"][rows][f] - dl[f]) <= REL * np.maximum(np.abs(dl[f]), 1.0)), (r, it0 + t)
                    assert np.abs(d["cube"][rows] - du).max() <= CUBE_TOL, (r, it0 + t)
                    compared += 1
                if last is not None:
                    rp.load(s, res, scale, lnx)
                    rp.resynced = True
                    continue
                lu, ll = d["cube"][nd:], d["lnl"][nd:]
                assert np.abs(lu - rp.live_u).max() <= CUBE_TOL, (r, rp.it)       # slot by slot: the freed slots exactly
                assert np.array_equal(np.isinf(ll), np.isinf(rp.live_l)), (r, rp.it)
                f = np.isfinite(ll)
                assert np.all(np.abs(ll[f] - rp.live_l[f]) <= REL * np.maximum(np.abs(ll[f]), 1.0)), (r, rp.it)
                assert res["nevals"][r] == rp.nevals, (r, res["nevals"][r], rp.nevals)
                assert abs(scale[r] - rp.scale) <= 1e-12 * rp.scale and abs(lnx[r] - rp.lnx) <= 1e-12 * max(1.0, abs(rp.lnx))
                if rp.lnz > -math.inf and not rp.done:
                    assert abs(res["lnz"][r] - rp.lnz) <= 1e-10 * max(1.0, abs(rp.lnz)), (r, res["lnz"][r], rp.lnz)
                rp.load(s, res, scale, lnx)                  # the next block starts from the device's state, to the bit
            if rc == _lib.GF_OK:
                break
        res = s.result()
        assert compared > 0
        assert min(res["niter"]) >= min_iter, res["niter"]
        for r, rp in enumerate(reps):
            check_points(oracle, prob, s, res, r)
        return reps, s, res
    finally:
        s.close()
        if lpw is not None:
            if old is None:
                os.environ.pop("GF_NESTED_LPW", None)
            else:
                os.environ["GF_NESTED_LPW"] = old


@pytest.mark.parametrize("K,B,D,R,blocks", [
    (4096, 512, 2, 1, 3),          # nlive at k_ns_select's LDS limit
    (37, 36, 2, 1, 3),             # batch nlive - 1: one survivor, a degenerate Cholesky factor; nlive not a power of two
    (100, 1, 3, 2, 8),             # batch 1, two runs
    (300, 37, 1, 3, 6),            # one dimension, three runs
    (500, 60, 16, 2, 4),           # GF_MAX_DIM dimensions
    (200, 3, 2, 2, 40),            # past 128 iterations: the dead buffers grow twice with two runs
], ids=["K4096", "B_K-1", "B1", "D1", "D16", "past128"])
def test_replay_prior_only(oracle, K, B, D, R, blocks):
    prob = prior_problem(oracle, D, D, nruns=R)
    try:
        reps, s, res = replay_and_compare(oracle, prob, K, B, 25, blocks, min_iter=129 if blocks == 40 else 0)
        print("iterations", res["niter"].tolist(), "close decisions", sum(len(r.close_calls) for r in reps))
    finally:
        prob.close()


def test_replay_sm_gauss(oracle):
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    bf = fr_utils.angles_to_fr(asimov.values)
    prob = Problem(oracle, [(ps, dict(bestfit_fr=bf, smearing=0.02))], "SM_GAUSS", [0, 1, 2, 3])
    try:
        replay_and_compare(oracle, prob, 200, 25, 25, 4)
    finally:
        prob.close()


@pytest.mark.parametrize("lpw", [1, 4, 16])
def test_replay_sens_plateau(oracle, lpw):
    """The 11-dim sens posterior at -42.5, where about two thirds of the cube has L = 0: the plateau accounting and the start
    points above L* step by step, on every lanes-per-walker instance of the BSM walk."""
    sp, kw = sens_spec(-42.5)
    cols = [i for i in range(len(sp)) if sp[i].tag != ParamTag.SCALE]
    prob = Problem(oracle, [(sp, kw)], "BSM_GAUSS", cols)
    try:
        reps, s, res = replay_and_compare(oracle, prob, 300, 40, 25, 3, lpw=lpw)
        d = reps[0]
        assert d.nplat > 0                                   # the replay went over the plateau
    finally:
        prob.close()


def test_replay_settle_path(oracle):
    """d = 6 texture OEU at scale -36: nearly every proposal's unitarity verdict falls in the band the in-kernel tiers cannot
    settle, so k_ns_walk parks it and k_stretch_settle<NESTED> decides; about 1 % are non-unitary.  The replay takes the
    oracle's verdicts: every acceptance, rejection and non-unitary count must match."""
    sp, kw = sens_spec(-36.0, texture=Texture.OEU)
    cols = [i for i in range(len(sp)) if sp[i].tag != ParamTag.SCALE]
    prob = Problem(oracle, [(sp, kw)], "BSM_GAUSS", cols)
    try:
        reps, s, res = replay_and_compare(oracle, prob, 200, 25, 10, 2, on_nonunitary="-inf")
        rp = reps[0]
        print("proposals in the undecided band: %d, non-unitary: %d (device %d)" % (rp.band, rp.nonunit, res["nonunitary"][0]))
        assert rp.band > 100
        assert rp.nonunit > 0 and res["nonunitary"][0] > 0
        if not rp.resynced:
            assert res["nonunitary"][0] == rp.nonunit
    finally:
        prob.close()
