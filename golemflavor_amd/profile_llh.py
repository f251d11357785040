"""The profile likelihood on the device: the maximum of ln_prob over every column but the new-physics scale, at every scale of
scripts/sens.py in one device call (gf_simplex.hip, include/golemflavor_hip.h gf_simplex_*).  It is the `fr_maxllh` the
reference's frequentist statistic is built from: golemflavor/plot.py:605-608 (plot_statistic) plots -2 (max lnL(scale) -
max lnL(null)), scripts/plot_sens.py:193-200 feeds it the per-scale array.  The reference imports scipy.optimize.minimize for
this (scripts/sens.py:21) and never calls it (sens.py:137-139 raises NotImplementedError).

Each start minimises f(u) = -ln_prob(theta(u)) over the unit cube of the scanned columns (the nested sampler's map) by scipy's
bounded Nelder-Mead, step for step; the starts are the best points of a uniform seeding draw plus the caller's.

    SimplexMaximizer            the device maximiser over several posteriors (one run each)
    nelder_mead_speculative     the device algorithm restated on the host (the tests' reference for the commit logic)
    profile_scan                sens.py's loop over scales in one device call
    profile_likelihood_limit    the scale where -2 (max lnL - null) crosses a threshold
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from .nested import _CubeRuns, _opt, _scan_models

__all__ = ["SimplexMaximizer", "nelder_mead_speculative", "nm_coefficients", "profile_scan", "profile_likelihood_limit",
           "DEFAULT_STARTS", "DEFAULT_SEED_POINTS", "DEFAULT_XATOL", "DEFAULT_FATOL", "DEFAULT_RESTARTS", "AGREE_TOL"]

DEFAULT_STARTS = 64
DEFAULT_SEED_POINTS = 8192
DEFAULT_XATOL = 1e-4          # scipy's defaults
DEFAULT_FATOL = 1e-4
DEFAULT_RESTARTS = 1
AGREE_TOL = 1e-3              # a start "agrees" when its final lnL is within this of the run's best


def nm_coefficients(n, adaptive):
    """scipy's (rho, chi, psi, sigma) (_minimize_neldermead), with its own expressions."""
    if adaptive:
        dim = float(n)
        return 1, 1 + 2 / dim, 0.75 - 1 / (2 * dim), 1 - 1 / dim
    return 1, 2, 0.5, 0.5


def _initial_simplex(x0):
    x0 = np.clip(np.asarray(x0, dtype=np.float64), 0.0, 1.0)
    N = len(x0)
    sim = np.empty((N + 1, N), dtype=x0.dtype)
    sim[0] = x0
    for k in range(N):
        y = np.array(x0, copy=True)
        y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
        sim[k + 1] = y
    sim = np.where(sim > 1.0, 2 * 1.0 - sim, sim)
    return np.clip(sim, 0.0, 1.0)


def _eval(f_batch, pts):
    out = f_batch(np.ascontiguousarray(pts))
    if isinstance(out, tuple):
        f, bad = out
        return np.asarray(f, dtype=np.float64), np.asarray(bad, dtype=bool)
    f = np.asarray(out, dtype=np.float64)
    return f, np.zeros(len(f), dtype=bool)


def nelder_mead_speculative(f_batch, x0, xatol=DEFAULT_XATOL, fatol=DEFAULT_FATOL, maxiter=None, adaptive=False, restarts=0,
                            on_nonunitary="-inf"):
    """scipy.optimize.minimize(f, x0, method='Nelder-Mead', bounds=[(0, 1)] * n, options=dict(xatol, fatol, maxiter,
    adaptive)) as the device runs it: every iteration forms xr, xe, xc and xcc and evaluates them in ONE call of `f_batch`
    ([m, n] points -> [m] values, or (values, non-unitary flags)), then commits them with scipy's sequential decision table;
    a shrink is a second call with the n shrunk vertices.  The vertices are sorted stably.  `restarts`: minimize again from
    x = res.x until the gain is <= fatol.  A non-unitary flag counts only for a point scipy would have evaluated; with
    on_nonunitary='raise' the first such point ends the run (failed=True).
    Returns dict(x, fun, nit, nfev, devals (points f_batch was given), nonunitary, nonunitary_speculative (flagged points
    scipy would not have evaluated: neither counted nor failing), failed, ties (a sort met equal values), calls: [(x, fun, nit,
    nfev)] per minimize call)."""
    x0 = np.asarray(x0, dtype=np.float64)
    N = len(x0)
    rho, chi, psi, sigma = nm_coefficients(N, adaptive)
    maxiter = N * 200 if maxiter is None else int(maxiter)
    out = dict(nit=0, nfev=0, devals=0, nonunitary=0, nonunitary_speculative=0, failed=False, ties=False, calls=[])
    flagged = [0]

    def evaluate(pts):
        f, bad = _eval(f_batch, pts)
        flagged[0] += int(bad.sum())
        return f, bad
    state = dict(failed=False)

    def use(bad):
        if bad:
            if on_nonunitary == "raise":
                state["failed"] = True
                return False
            out["nonunitary"] += 1
        return True

    def srt(sim, fsim):
        if len(np.unique(fsim)) < len(fsim):
            out["ties"] = True
        ind = np.argsort(fsim, kind="stable")
        return np.take(sim, ind, 0), np.take(fsim, ind, 0)

    def minimize(x0):
        sim = _initial_simplex(x0)
        f, bad = evaluate(sim)
        out["devals"] += N + 1
        fsim = np.full((N + 1,), np.inf)
        for k in range(N + 1):
            if not use(bad[k]):
                return None
            fsim[k] = f[k]
        nfev = N + 1
        sim, fsim = srt(sim, fsim)
        iterations = 1
        while iterations < maxiter:
            with np.errstate(invalid="ignore"):             # inf - inf: NaN, never converged (as in scipy)
                done = np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol
            if done:
                break
            xbar = np.add.reduce(sim[:-1], 0) / N
            cand = np.stack([(1 + rho) * xbar - rho * sim[-1],
                             (1 + rho * chi) * xbar - rho * chi * sim[-1],
                             (1 + psi * rho) * xbar - psi * rho * sim[-1],
                             (1 - psi) * xbar + psi * sim[-1]])
            cand = np.clip(cand, 0.0, 1.0)
            fc, bc = evaluate(cand)
            out["devals"] += 4
            nfev += 1
            if not use(bc[0]):
                return None
            fxr = fc[0]
            take = None
            if fxr < fsim[0]:
                nfev += 1
                if not use(bc[1]):
                    return None
                take = 1 if fc[1] < fxr else 0
            elif fxr < fsim[-2]:
                take = 0
            elif fxr < fsim[-1]:
                nfev += 1
                if not use(bc[2]):
                    return None
                take = 2 if fc[2] <= fxr else None
            else:
                nfev += 1
                if not use(bc[3]):
                    return None
                take = 3 if fc[3] < fsim[-1] else None
            if take is not None:
                sim[-1] = cand[take]
                fsim[-1] = fc[take]
            else:
                for j in range(1, N + 1):
                    sim[j] = np.clip(sim[0] + sigma * (sim[j] - sim[0]), 0.0, 1.0)
                fs, bs = evaluate(sim[1:])
                out["devals"] += N
                for j in range(1, N + 1):
                    if not use(bs[j - 1]):
                        return None
                    fsim[j] = fs[j - 1]
                nfev += N
            iterations += 1
            sim, fsim = srt(sim, fsim)
        return sim[0].copy(), float(np.min(fsim)), iterations, nfev

    x = x0
    fprev = None
    for call in range(int(restarts) + 1):
        res = minimize(x)
        if res is None:
            out["failed"] = True
            break
        x, fun, nit, nfev = res
        out["calls"].append(res)
        out["nit"] += nit
        out["nfev"] += nfev
        gain = None if fprev is None else fprev - fun
        fprev = fun
        if gain is not None and gain <= fatol:
            break
    if not out["failed"]:
        out["nonunitary_speculative"] = flagged[0] - out["nonunitary"]
    if out["calls"]:
        out["x"], out["fun"] = out["calls"][-1][0], out["calls"][-1][1]
    else:
        out["x"], out["fun"] = np.clip(x0, 0.0, 1.0), np.inf
    return out


class SimplexMaximizer(_CubeRuns):
    """`nruns` independent maximisations of ln_prob (nested._CubeRuns: models, cols, bases, run_ids, labels).  Starts: the
    `nstarts` best finite points of `nseed` uniform cube points per run, then `starts` ([nruns][k][nscan] or [k][nscan] cube
    points; optional).  Options as scipy's Nelder-Mead (xatol, fatol, maxiter = 200 n by default, adaptive) plus `restarts`.
    `measurements` = (bestfit_fr [nruns][3], smearing [nruns] or one value): run r maximises under that Gaussian measurement in place
    of its model's (needs nseed = 0, the flux-averaged likelihood).  `start_counts` [nruns] (with nstarts = 0): run r keeps
    the first start_counts[r] of `starts` only.  `binned_measurements` = (fr_bins [nruns][nb][3], sigma [nruns][nb] or [nb]): run r
    maximises under that binned measurement in place of its model's (needs nseed = 0 and models with a binned measurement)."""
    _abi, _what = "simplex", "profile run"

    def __init__(self, models, cols, bases, nstarts=DEFAULT_STARTS, nseed=DEFAULT_SEED_POINTS, seed=0, starts=None,
                 on_nonunitary="raise", xatol=DEFAULT_XATOL, fatol=DEFAULT_FATOL, maxiter=None, adaptive=False,
                 restarts=DEFAULT_RESTARTS, run_ids=None, labels=None, measurements=None, start_counts=None,
                 binned_measurements=None):
        hs = self._open(models, cols, bases, on_nonunitary, labels)
        self.nstarts, self.nseed, self.seed = int(nstarts), int(nseed), int(seed)
        self.maxiter = int(maxiter) if maxiter is not None else 200 * self.nscan
        self.restarts = int(restarts)
        h = C.c_void_p()
        _lib.check(self._L.gf_simplex_create(hs, self.nruns, self.nscan, self.cols.ctypes.data_as(_lib._ip),
                                             self.bases.ctypes.data_as(_lib._dp), self.nstarts, self.nseed,
                                             self.seed & 0xFFFFFFFFFFFFFFFF, 0 if on_nonunitary == "raise" else 1, C.byref(h)),
                   "gf_simplex_create")
        self._h = h
        _lib.check(self._L.gf_simplex_set_options(self._h, float(xatol), float(fatol), self.maxiter, int(bool(adaptive)),
                                                  self.restarts), "gf_simplex_set_options")
        self.nuser = 0
        if starts is not None:
            st = np.asarray(starts, dtype=np.float64)
            if st.ndim == 2:
                st = np.tile(st[None], (self.nruns, 1, 1))
            st = np.ascontiguousarray(st.reshape(self.nruns, -1, self.nscan))
            self.nuser = st.shape[1]
            _lib.check(self._L.gf_simplex_set_starts(self._h, self.nuser, st.ctypes.data_as(_lib._dp)), "gf_simplex_set_starts")
        self._set_run_ids(run_ids)
        if measurements is not None:
            self.set_measurements(*measurements)
        if binned_measurements is not None:
            self.set_binned_measurements(*binned_measurements)
        if start_counts is not None:
            cnt = np.ascontiguousarray(np.broadcast_to(np.asarray(start_counts, dtype=np.int32), (self.nruns,)))
            _lib.check(self._L.gf_toys_set_start_counts(self._h, cnt.ctypes.data_as(_lib._ip)), "gf_toys_set_start_counts")

    def set_measurements(self, bestfit_fr, smearing):
        """A Gaussian measurement of its own for every run, before the first run(): bestfit_fr [nruns][3], smearing [nruns] or one
        value.  Run r then evaluates what a Model compiled with (bestfit_fr[r], smearing[r]) evaluates."""
        bf = np.ascontiguousarray(np.broadcast_to(np.asarray(bestfit_fr, dtype=np.float64), (self.nruns, 3)))
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (self.nruns,)))
        _lib.check(self._L.gf_toys_set_measurements(self._h, bf.ctypes.data_as(_lib._dp), sm.ctypes.data_as(_lib._dp)),
                   "gf_toys_set_measurements")

    def set_binned_measurements(self, fr_bins, sigma):
        """A binned measurement of its own for every run, before the first run(): fr_bins [nruns][nb][3], sigma [nruns][nb] or [nb].
        Run r then evaluates what a Model with set_binned_measurement(BinnedMeasurement(fr_bins[r], sigma[r])) evaluates."""
        f = np.ascontiguousarray(fr_bins, dtype=np.float64)
        if f.ndim != 3 or f.shape[0] != self.nruns or f.shape[2] != 3:
            raise ValueError("fr_bins must be [nruns][nb][3]")
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), f.shape[:2]))
        _lib.check(self._L.gf_toys_set_binned_measurements(self._h, int(f.shape[1]), f.ctypes.data_as(_lib._dp), sg.ctypes.data_as(_lib._dp)),
                   "gf_toys_set_binned_measurements")

    def max_rounds(self):
        """Evaluation rounds after which every start has finished: per minimize call one round for the initial simplex and at
        most two per iteration (the candidates, a shrink)."""
        return (self.restarts + 1) * (2 * self.maxiter + 1) + 1

    def run(self, check=True):
        """Every start to its end; returns result(), raising AssertionError for a run that evaluated a point the reference
        would have raised on (on_nonunitary == 'raise') when `check`."""
        _lib.check(self._L.gf_simplex_run(self._h, self.max_rounds()), "gf_simplex_run")
        return self._checked(self.result(), check)

    def result(self):
        n = self.nruns
        ml = np.zeros(n)
        cube = np.zeros((n, self.nscan))
        ns, fl = np.zeros(n, np.int32), np.zeros(n, np.int32)
        it, fe, ev = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        nu, pk = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        p64 = C.POINTER(C.c_int64)
        _lib.check(self._L.gf_simplex_result(self._h, ml.ctypes.data_as(_lib._dp), cube.ctypes.data_as(_lib._dp),
                                             ns.ctypes.data_as(_lib._ip), it.ctypes.data_as(p64), fe.ctypes.data_as(p64),
                                             ev.ctypes.data_as(p64), nu.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             pk.ctypes.data_as(C.POINTER(C.c_uint32)), fl.ctypes.data_as(_lib._ip)),
                   "gf_simplex_result")
        theta = self.bases.copy()
        for r in range(n):
            theta[r, self.cols] = self.cube_to_theta(r, cube[r])
        return dict(max_lnl=ml, argmax_cube=cube, argmax_theta=theta, nstarts=ns, niter=it, nfev=fe, nevals=ev,
                    nonunitary=nu, parked=pk, failed=fl.astype(bool))

    def starts(self, run=0):
        """Run `run`'s starts: dict(lnl = -final f, cube, nit, nfev), [nstarts + nuser] rows; only the first `used` are starts."""
        k = self.nstarts + self.nuser
        f, cube = np.zeros(k), np.zeros((k, self.nscan))
        nit, nfev = np.zeros(k, np.int32), np.zeros(k, np.int64)
        _lib.check(self._L.gf_simplex_get_starts(self._h, int(run), f.ctypes.data_as(_lib._dp), cube.ctypes.data_as(_lib._dp),
                                                 nit.ctypes.data_as(_lib._ip), nfev.ctypes.data_as(C.POINTER(C.c_int64))),
                   "gf_simplex_get_starts")
        return dict(lnl=-f, cube=cube, nit=nit, nfev=nfev)

    def cube_to_theta(self, run, cube):
        """theta of cube points on the scanned columns, as the device forms it: (hi - lo) u + lo, each operation rounded."""
        desc = getattr(self.models[run], "model", self.models[run]).desc
        lo, hi = np.asarray(desc.lo)[self.cols], np.asarray(desc.hi)[self.cols]
        return (hi - lo) * np.asarray(cube, dtype=np.float64) + lo


def profile_scan(args, asimov_paramset, llh_paramset, scales, run_ids=None, nstarts=None, nseed=None, xatol=None, fatol=None,
                 maxiter=None, restarts=None, adaptive=None, seed=None, on_nonunitary="raise", smearing=None, device=0,
                 return_maximizer=False, binned=None, table=None):
    """The profile likelihood at every scale in one device call, with evidence_scan's conventions: the scanned columns are every
    column but the scale (sens.py:217-218), the scale column is fixed at each scale with its box lowered for the null point.
    `args` as for evidence_scan plus the --pl-* options.  Returns dict(scales, max_lnl, argmax_theta, nstarts, nfev, nevals,
    niter, nonunitary, seconds, starts_agreeing: the starts whose final lnL is within AGREE_TOL of the run's best).
    binned (`llh.BinnedMeasurement`): the profile of the energy-resolved likelihood -- the measurement is attached to
    every scale's model.  table (`llh.TabulatedLikelihood`): the profile of the tabulated flavour-plane likelihood."""
    scales = np.asarray(scales, dtype=np.float64)
    cols, models, bases, labels = _scan_models(args, asimov_paramset, llh_paramset, scales, smearing, device, binned=binned, table=table)

    def pick(v, name, default):
        return v if v is not None else _opt(args, name, default)

    try:
        s = SimplexMaximizer(models, cols, bases, nstarts=int(pick(nstarts, "pl_starts", DEFAULT_STARTS)),
                             nseed=int(pick(nseed, "pl_seed_points", DEFAULT_SEED_POINTS)),
                             seed=int(seed if seed is not None else _opt(args, "seed", 0)), on_nonunitary=on_nonunitary,
                             xatol=float(pick(xatol, "pl_xatol", DEFAULT_XATOL)), fatol=float(pick(fatol, "pl_fatol", DEFAULT_FATOL)),
                             maxiter=pick(maxiter, "pl_maxiter", None), adaptive=bool(pick(adaptive, "pl_adaptive", True)),
                             restarts=int(pick(restarts, "pl_restarts", DEFAULT_RESTARTS)), run_ids=run_ids, labels=labels)
        t0 = time.perf_counter()
        try:
            res = s.run()
            res["seconds"] = time.perf_counter() - t0
            agree = np.zeros(len(scales), np.int64)
            for r in range(len(scales)):
                used = int(res["nstarts"][r])
                if used and np.isfinite(res["max_lnl"][r]):
                    agree[r] = int(np.sum(s.starts(r)["lnl"][:used] >= res["max_lnl"][r] - AGREE_TOL))
            res["starts_agreeing"] = agree
        finally:
            if not return_maximizer:
                s.close()
        res["scales"] = scales
        if return_maximizer:
            res["maximizer"] = s
            res["models"] = models
        return res
    finally:
        if not return_maximizer:
            for m in models:
                m.close()


def profile_likelihood_limit(scales, max_lnl, threshold=None):
    """The lowest scale on the splined curve (splprep, s=0, 1000 points) where the test statistic -2 (max lnL - null) exceeds
    `threshold`, minus log10(2) (the standard SME coefficient, as nested.bayes_factor_limit).  Non-finite rows are dropped first
    (plot_sens.py's masked_invalid, plot_statistic's compress_rows); the null is the row of the smallest scale, and a null row
    that is not finite gives None rather than a statistic measured against another scale.  None as
    bayes_factor_limit returns None: no such scale, a curve that does not exclude the large scales (two or more scanned points
    above the crossing within 0.1 of the threshold), or fewer than two scanned points above it beyond the threshold.
    The reference defines no frequentist limit (golemflavor/plot.py:155-156 raises NotImplementedError): the default
    threshold chi2.ppf(0.95, 1) = 3.84 (one parameter, 95 %) is this package's choice."""
    from scipy.interpolate import splev, splprep
    from scipy.stats import chi2
    thr = float(chi2.ppf(0.95, 1) if threshold is None else threshold)
    scales = np.asarray(scales, dtype=np.float64)
    st = np.asarray(max_lnl, dtype=np.float64)
    if len(st) == 0 or not np.isfinite(st[np.argmin(scales)]):
        return None                                       # no null row to measure against
    ok = np.isfinite(scales) & np.isfinite(st)
    scales, st = scales[ok], st[ok]
    if len(scales) < 4:                                   # splprep's cubic spline needs m > k = 3 points
        return None
    tck, _ = splprep([scales, st], s=0)
    sc, sst = splev(np.linspace(0, 1, 1000), tck)
    null = st[np.argmin(scales)]
    ts = -2 * (sst - null)
    al = sc[ts > thr]
    if len(al) == 0:
        return None
    re = (-2 * (st - null))[scales > al[0]]
    if np.sum(re < thr - 0.1) >= 2:
        return None
    if np.sum(re >= thr + 0.0) < 2:
        return None
    return al[0] - np.log10(2.)
