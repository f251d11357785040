"""Realisation ensembles: the profile likelihood of many mock measurements at every new-physics scale in one call (DESIGN.md 6j;
gf_toys_common.hip, gf_toys.hip, include/golemflavor_hip.h gf_toys_*, gf_toys_set_measurements).

The frequentist statistic of scripts/sens.py is -2 (max lnL(scale) - max lnL(null)); the reference cuts its Asimov curve at a chi2
quantile (Wilks' theorem) and notes that the statistic's distribution "can be approximated by generating mock data or realisations of
the null hypothesis", which it finds computationally difficult (docs/source/statistics.rst:95-110).  Here a realisation of the
Gaussian measurement (bf, smearing) is m = bf + smearing z, z ~ N(0, I_3) -- the generative model of multi_gaussian's isotropic
Gaussian, not projected onto the simplex -- and every realisation is profiled at every scale: the scales' seed points are drawn and
propagated once, ranked under every realisation on the device, and the best K of each (scale, realisation) polished by the device
Nelder-Mead maximiser under that realisation's measurement.

    draw_realisations      m = bf + smearing z on the host (numpy's default_rng): bring your own instead if you like
    ToySeeds               the shared seeding: the seeds of every scale, their selection under realisations
    realisation_scan       max lnL and the test statistic of every (realisation, scale), the limit of every realisation
    sensitivity_band       quantiles of the limits: the median expected limit with its one- and two-sigma band
    ts_quantiles           the empirical critical value of the statistic per scale, to hold against chi2.ppf(0.95, 1)
    save_realisations      the scan's arrays as one .npz

The energy-resolved likelihood has the frequentist ensembles too (gf_toys_binned.hip): a realisation of a
`BinnedMeasurement` (m_k, sigma_k) is m_{t,k} = m_k + sigma_k z_{t,k}, independent per energy bin, the seeds carry their composition at
every bin, and the polish runs under a binned measurement per run.

    draw_binned_realisations   m_k + sigma_k z on the host
    BinnedToySeeds             the shared seeding with per-bin compositions, their selection under binned realisations
    binned_realisation_scan    realisation_scan for the energy-resolved likelihood: the same dict, for sensitivity_band and ts_quantiles

The Bayesian statistic has the same ensembles without a run per realisation (gf_ns_toys.hip): one evidence scan keeps
its dead points, and the evidence of every realisation at every scale is a reweighting of them.

    evidence_realisation_scan    ln Z of every (realisation, scale), the Bayes-factor limit of every realisation
    evidence_limits              bayes_factor_limit row by row: the limits, and which realisations "discovered" new physics
    save_evidence_realisations   the scan's arrays and the band as one .npz
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from . import fr as fr_utils
from . import rowsets
from .enums import ParamTag
from . import nested
from .nested import _opt, _scan_models
from .profile_llh import (DEFAULT_FATOL, DEFAULT_RESTARTS, DEFAULT_SEED_POINTS, DEFAULT_XATOL, SimplexMaximizer,
                          profile_likelihood_limit)

__all__ = ["draw_realisations", "ToySeeds", "realisation_scan", "sensitivity_band", "ts_quantiles", "save_realisations",
           "draw_binned_realisations", "BinnedToySeeds", "toy_select_binned", "binned_realisation_scan",
           "evidence_realisation_scan", "evidence_limits", "save_evidence_realisations",
           "DEFAULT_TOY_STARTS", "MAX_TOY_STARTS", "MAX_RUNS"]

DEFAULT_TOY_STARTS = 8
MAX_TOY_STARTS = _lib.GF_TOY_MAX_STARTS
MAX_RUNS = 65535              # runs of one maximiser (gf_simplex_create)
BAND_QUANTILES = (2.5, 16., 50., 84., 97.5)


def draw_realisations(bf, smearing, n, seed=0):
    """`n` realisations m = bf + smearing z of the Gaussian measurement (bf [3], smearing), z ~ N(0, I_3) from
    np.random.default_rng(seed): [n][3].  Not projected onto the simplex: the likelihood's own generative model."""
    bf = np.asarray(bf, dtype=np.float64).reshape(3)
    if not (float(smearing) > 0.0 and np.isfinite(smearing)):
        raise ValueError("smearing must be positive and finite")
    z = np.random.default_rng(seed).standard_normal((int(n), 3))
    return bf + float(smearing) * z


class _SeedSet:
    """What ToySeeds and BinnedToySeeds share (the device's one seed set, csrc/gf_toys_common.hip): the construction, the lifetime and
    the seeds' theta.  A subclass names its entry points by `_SUFFIX` (gf_toys_create<_SUFFIX>, ...) and has its own _measurements,
    the arguments and docstrings of select and scores, and the arrays its seeds() fetches."""
    _SUFFIX = ""

    def __init__(self, models, cols, bases, nseed=DEFAULT_SEED_POINTS, seed=0, run_ids=None):
        self._L = _lib.lib()
        self.models = list(models)
        self.nscales = len(self.models)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32)
        self.nscan, self.nseed = len(self.cols), int(nseed)
        ndim = self._L.gf_model_ndim(rowsets.handle(self.models[0]))
        b = np.asarray(bases, dtype=np.float64)
        if b.ndim == 1:
            b = np.tile(b, (self.nscales, 1))
        self.bases = np.ascontiguousarray(b.reshape(self.nscales, ndim))
        self._h = C.c_void_p()
        self._call("gf_toys_create", rowsets.model_handles(self.models, self.nscales), self.nscales, self.nscan,
                   self.cols.ctypes.data_as(_lib._ip), self.bases.ctypes.data_as(_lib._dp), self.nseed, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(self._h))
        try:
            if run_ids is not None:
                self._call("gf_toys_set_run_ids", self._h, np.ascontiguousarray(run_ids, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)))
            self.nonunitary_seeds = np.zeros(self.nscales, np.uint32)
            self._call("gf_toys_seed", self._h, self.nonunitary_seeds.ctypes.data_as(C.POINTER(C.c_uint32)))
        except BaseException:
            self.close()
            raise

    def _call(self, name, *args):
        """the entry point `name` of this class's handle, checked"""
        _lib.check(getattr(self._L, name + self._SUFFIX)(*args), name + self._SUFFIX)

    def _select(self, T, head, K):
        """select() for the measurements `head`, the entry point's arguments in front of T (from _measurements)"""
        S, K, Kc = self.nscales, int(K), max(int(K), 0)
        out = dict(cube=np.empty((S, T, Kc, self.nscan)), index=np.empty((S, T, Kc), np.int32), score=np.empty((S, T, Kc)),
                   count=np.empty((S, T), np.int32))
        self._call("gf_toys_select", self._h, *head, T, K, out["cube"].ctypes.data_as(_lib._dp), out["index"].ctypes.data_as(_lib._ip),
                   out["score"].ctypes.data_as(_lib._dp), out["count"].ctypes.data_as(_lib._ip))
        return out

    def _scores(self, T, head):
        out = np.empty((self.nscales, T, self.nseed))
        self._call("gf_toys_scores", self._h, *head, T, out.ctypes.data_as(_lib._dp))
        return out

    def _seeds(self, scale, shapes):
        """seeds(): the arrays of `shapes` (name: a seed's shape, in the entry point's order), status and theta"""
        M = self.nseed
        out = {k: np.empty((M,) + tuple(shape)) for k, shape in shapes.items()}
        out["status"] = np.empty(M, np.int32)
        self._call("gf_toys_get_seeds", self._h, int(scale), *[out[k].ctypes.data_as(_lib._dp) for k in shapes], out["status"].ctypes.data_as(_lib._ip))
        desc = getattr(self.models[scale], "model", self.models[scale]).desc
        lo, hi = np.asarray(desc.lo)[self.cols], np.asarray(desc.hi)[self.cols]
        theta = out["theta"] = np.tile(self.bases[scale], (M, 1))
        theta[:, self.cols] = (hi - lo) * out["cube"] + lo
        return out

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, "gf_toys_destroy" + self._SUFFIX)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ToySeeds(_SeedSet):
    """The shared seeding of a realisation ensemble: `nseed` uniform cube points per scale (models, cols, bases, run_ids as for
    SimplexMaximizer -- the points its seeding draws for the same seed and run id), evaluated once by each scale model's bulk path.
    `nonunitary_seeds` [nscales]: the seeds the reference would have raised on."""

    def _measurements(self, bestfit_fr, smearing):
        bf = np.ascontiguousarray(bestfit_fr, dtype=np.float64)
        if bf.ndim not in (2, 3) or bf.shape[-1] != 3 or (bf.ndim == 3 and bf.shape[0] != self.nscales):
            raise ValueError("measurements must be [T][3] or [nscales][T][3]")
        T = bf.shape[-2]
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (T,)))
        return T, (bf.ctypes.data_as(_lib._dp), int(bf.ndim == 3), sm.ctypes.data_as(_lib._dp))

    def select(self, bestfit_fr, smearing, K):
        """The starts of every (scale, realisation): the K best seeds under score = lp + gauss(m_t, fr), score descending then seed
        index ascending, finite scores only.  bestfit_fr [T][3] (shared by the scales) or [nscales][T][3]; smearing [T] or one value.
        Returns dict(cube [nscales][T][K][nscan] (NaN behind the count), index, score [nscales][T][K] (-1, -inf), count [nscales][T])."""
        return self._select(*self._measurements(bestfit_fr, smearing), K)

    def scores(self, bestfit_fr, smearing):
        """Every score the selection ranks, [nscales][T][nseed]."""
        return self._scores(*self._measurements(bestfit_fr, smearing))

    def seeds(self, scale=0):
        """Scale `scale`'s seeds: dict(cube [nseed][nscan], theta [nseed][ndim] (the device's map: product and sum each rounded),
        lnprob (the scale model's own), lp (the prior sum, -inf outside the box), fr [nseed][3], status)."""
        return self._seeds(scale, dict(cube=(self.nscan,), lnprob=(), lp=(), fr=(3,)))


def toy_select(lp, fr, status, bestfit_fr, smearing, offset, K, device=0):
    """gf_toy_select: the selection alone on host arrays (one seed set: lp [M], fr [M][3], status [M]; bestfit_fr [T][3], smearing
    [T] or one value).  Returns (index [T][K], score [T][K], count [T])."""
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    fr = np.ascontiguousarray(fr, dtype=np.float64).reshape(len(lp), 3)
    status = np.ascontiguousarray(status, dtype=np.int32)
    bf = np.ascontiguousarray(bestfit_fr, dtype=np.float64).reshape(-1, 3)
    T, K = len(bf), int(K)
    sm = np.ascontiguousarray(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (T,)))
    index, score, count = np.empty((T, max(K, 0)), np.int32), np.empty((T, max(K, 0))), np.empty(T, np.int32)
    _lib.check(_lib.lib().gf_toy_select(int(device), lp.ctypes.data_as(_lib._dp), fr.ctypes.data_as(_lib._dp), status.ctypes.data_as(_lib._ip),
                                        len(lp), bf.ctypes.data_as(_lib._dp), sm.ctypes.data_as(_lib._dp), float(offset), T, K,
                                        index.ctypes.data_as(_lib._ip), score.ctypes.data_as(_lib._dp), count.ctypes.data_as(_lib._ip)),
               "gf_toy_select")
    return index, score, count


def draw_binned_realisations(binned, n, seed=0):
    """`n` realisations m_{t,k} = m_k + sigma_k z_{t,k} of the `llh.BinnedMeasurement` `binned`, z from
    np.random.default_rng(seed).standard_normal((n, nb, 3)): [n][nb][3].  Independent per energy bin and not projected onto the simplex:
    the generative model of the likelihood's own sum of isotropic Gaussians."""
    z = np.random.default_rng(seed).standard_normal((int(n), binned.nbins, 3))
    return binned.fr_bins[None] + binned.sigma[None, :, None] * z


class BinnedToySeeds(_SeedSet):
    """The shared seeding of a realisation ensemble of the energy-resolved likelihood: ToySeeds over models that carry a
    binned measurement (`Model.set_binned_measurement`), the seeds keeping their composition at every energy bin.  The compositions take
    24 * nscales * nseed * nbins bytes on the device."""
    _SUFFIX = "_binned"

    def __init__(self, models, cols, bases, nseed=DEFAULT_SEED_POINTS, seed=0, run_ids=None):
        super().__init__(models, cols, bases, nseed, seed, run_ids)
        self.nbins = int(self._L.gf_model_nbins(rowsets.handle(self.models[0])))

    def _measurements(self, meas, sigma):
        m = np.ascontiguousarray(meas, dtype=np.float64)
        if m.ndim not in (3, 4) or m.shape[-2:] != (self.nbins, 3) or (m.ndim == 4 and m.shape[0] != self.nscales):
            raise ValueError("measurements must be [T][%d][3] or [nscales][T][%d][3]" % (self.nbins, self.nbins))
        T = m.shape[-3]
        sg = np.ascontiguousarray(sigma, dtype=np.float64)
        if sg.shape not in ((self.nbins,), (T, self.nbins)):
            raise ValueError("widths must be [%d], shared by the realisations, or [T][%d]" % (self.nbins, self.nbins))
        return T, (m.ctypes.data_as(_lib._dp), int(m.ndim == 4), sg.ctypes.data_as(_lib._dp), int(sg.ndim == 2))

    def select(self, meas, sigma, K):
        """The starts of every (scale, realisation): the K best seeds under the binned score, score descending then seed index ascending,
        finite scores only.  meas [T][nb][3] (shared by the scales) or [nscales][T][nb][3]; sigma [nb] or [T][nb].  Returns ToySeeds.select's
        dict."""
        return self._select(*self._measurements(meas, sigma), K)

    def scores(self, meas, sigma):
        """Every score the selection ranks, [nscales][T][nseed]."""
        return self._scores(*self._measurements(meas, sigma))

    def seeds(self, scale=0):
        """Scale `scale`'s seeds: ToySeeds.seeds' dict (lnprob: the scale model's own, under its binned measurement; fr: the flux-averaged
        composition) and fr_bins [nseed][nb][3], NaN for a seed whose status is not GF_ST_OK."""
        return self._seeds(scale, dict(cube=(self.nscan,), lnprob=(), lp=(), fr=(3,), fr_bins=(self.nbins, 3)))


def toy_select_binned(lp, fr_bins, status, meas, sigma, offset, K, device=0):
    """gf_toy_select_binned: the selection alone on host arrays (one seed set: lp [M], fr_bins [M][nb][3], status [M]; meas [T][nb][3],
    sigma [nb] or [T][nb]).  Returns (index [T][K], score [T][K], count [T])."""
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    fb = np.ascontiguousarray(fr_bins, dtype=np.float64)
    nb = fb.shape[-2] if fb.ndim == 3 else 0
    status = np.ascontiguousarray(status, dtype=np.int32)
    m = np.ascontiguousarray(meas, dtype=np.float64)
    if fb.ndim != 3 or fb.shape != (len(lp), nb, 3) or m.ndim != 3 or m.shape[1:] != (nb, 3):
        raise ValueError("fr_bins must be [M][nb][3] and meas [T][nb][3]")
    T, K = len(m), int(K)
    sg = np.ascontiguousarray(sigma, dtype=np.float64)
    if sg.shape not in ((nb,), (T, nb)):
        raise ValueError("widths must be [nb] or [T][nb]")
    index, score, count = np.empty((T, max(K, 0)), np.int32), np.empty((T, max(K, 0))), np.empty(T, np.int32)
    _lib.check(_lib.lib().gf_toy_select_binned(int(device), lp.ctypes.data_as(_lib._dp), fb.ctypes.data_as(_lib._dp), status.ctypes.data_as(_lib._ip),
                                               len(lp), nb, m.ctypes.data_as(_lib._dp), sg.ctypes.data_as(_lib._dp), int(sg.ndim == 2), float(offset),
                                               T, K, index.ctypes.data_as(_lib._ip), score.ctypes.data_as(_lib._dp),
                                               count.ctypes.data_as(_lib._ip)), "gf_toy_select_binned")
    return index, score, count


def realisation_scan(args, asimov_paramset, llh_paramset, scales, measurements=None, ntoys=None, toy_seed=0, smearings=None,
                     nstarts=DEFAULT_TOY_STARTS, nseed=None, run_ids=None, xatol=None, fatol=None, maxiter=None, restarts=None,
                     adaptive=None, seed=None, on_nonunitary="raise", smearing=None, device=0, batch=None, threshold=None, check=True,
                     binned=None):
    """The profile likelihood of T realisations at every scale, with profile_scan's conventions (its --pl-* options, its scanned
    columns, its seed points per scale for the same `seed` and `run_ids`).

    measurements: [T][3], shared by all scales, or [S][T][3], per scale (throws under a scale's own hypothesis); None: `ntoys`
    realisations of the model's own measurement by draw_realisations(bf, smearing, ntoys, toy_seed).  smearings: [T], default the
    model's.  nstarts = K <= 16 starts per (realisation, scale): the best seeds under that realisation.  batch: realisations per
    maximiser (default: as many as keep its runs within 65535); no result depends on it.

    For realisation t and scale s, max_lnl[t, s] is the maximum of ln_prob over every column but the scale under (m_t, smearing_t),
    and ts[t, s] = -2 (max_lnl[t, s] - max_lnl[t, null]), the null the row of the smallest scale.  Returns dict(scales, measurements,
    smearings, max_lnl [T][S], ts [T][S], argmax_theta [T][S][ndim], nstarts, nfev, niter, nonunitary (points the polish counted),
    parked, failed [T][S], start_cube [T][S][K][nscan], start_score [T][S][K] and start_count [T][S] (the selected seeds: NaN and -inf
    behind the count), nonunitary_seeds [S], limits [T] (profile_likelihood_limit per realisation at `threshold`, NaN where it
    gives None), seconds, seconds_seed, seconds_select, seconds_polish).  on_nonunitary == 'raise': a non-unitary seed fails every
    run of its scale, as it fails profile_scan's run; AssertionError when `check`."""
    if binned is not None:
        raise ValueError("realisations are of the flux-averaged Gaussian likelihood; the energy-resolved one is not supported")
    K, opts = _scan_options(args, nstarts, xatol, fatol, maxiter, adaptive, restarts, on_nonunitary)
    scales = np.asarray(scales, dtype=np.float64)
    sm0, meas, sms = _gaussian_measurements(args, asimov_paramset, len(scales), measurements, ntoys, toy_seed, smearings, smearing)
    return _scan(ToySeeds, "measurements", meas, sms, meas.ndim == 3, {}, args, asimov_paramset, llh_paramset, scales, K, nseed, run_ids,
                 opts, seed, sm0, device, batch, threshold, check)


def _gaussian_measurements(args, asimov_paramset, S, measurements, ntoys, toy_seed, smearings, smearing):
    """Gaussian measurements given or drawn, validated: (the model's smearing, measurements [T][3] or [S][T][3], smearings [T])"""
    sm0 = float(smearing if smearing is not None else _opt(args, "smearing", 0.02))
    if measurements is None:
        if ntoys is None:
            raise ValueError("give measurements or ntoys")
        measurements = draw_realisations(fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True)), sm0, ntoys, toy_seed)
    meas = np.ascontiguousarray(measurements, dtype=np.float64)
    if meas.ndim not in (2, 3) or meas.shape[-1] != 3 or (meas.ndim == 3 and meas.shape[0] != S):
        raise ValueError("measurements must be [T][3] or [S][T][3]")
    return sm0, meas, np.ascontiguousarray(np.broadcast_to(np.asarray(sm0 if smearings is None else smearings, dtype=np.float64), (meas.shape[-2],)))


def _scan(seed_class, keyword, meas, widths, per_scale, extra, args, asimov_paramset, llh_paramset, scales, K, nseed, run_ids, opts, seed,
          smearing, device, batch, threshold, check, binned=None):
    """The body of a realisation scan over validated measurements (`meas` per scale when `per_scale`, `widths` [T] first): the seeds of
    `seed_class`, their selection, the polish with the runs' measurements under the maximiser's `keyword`, the statistic, and the
    result with the `extra` keys."""
    S, T = len(scales), len(widths)
    per_run = MAX_RUNS // S if batch is None else int(batch)
    if per_run < 1 or per_run * S > MAX_RUNS:
        raise ValueError("batch must keep batch * len(scales) within %d runs" % MAX_RUNS)
    cols, models, bases, labels = _scan_models(args, asimov_paramset, llh_paramset, scales, smearing, device, binned=binned)
    try:
        t0 = time.perf_counter()
        with seed_class(models, cols, bases, nseed=int(nseed if nseed is not None else _opt(args, "pl_seed_points", DEFAULT_SEED_POINTS)),
                        seed=int(seed if seed is not None else _opt(args, "seed", 0)), run_ids=run_ids) as seeds:
            t1 = time.perf_counter()
            sel = seeds.select(meas, widths, K)
            nu_seeds = seeds.nonunitary_seeds.copy()
        t2 = time.perf_counter()
        res, dead = _polish(models, cols, bases, labels, sel, nu_seeds, T, per_run, opts, keyword, meas, widths, per_scale)
        t3 = time.perf_counter()
    finally:
        for m in models:
            m.close()
    _statistic(res, dead, labels, scales, threshold, check and opts["on_nonunitary"] == "raise")
    res.update(scales=scales, measurements=meas, smearings=widths, nonunitary_seeds=nu_seeds, **extra, **_starts_of(sel),
               seconds=t3 - t0, seconds_seed=t1 - t0, seconds_select=t2 - t1, seconds_polish=t3 - t2)
    return res


def _scan_options(args, nstarts, xatol, fatol, maxiter, adaptive, restarts, on_nonunitary):
    """(K, the maximiser's options) of a realisation scan: the keyword, else args' --pl-* option, else the default"""
    if on_nonunitary not in ("raise", "-inf"):
        raise ValueError("on_nonunitary must be 'raise' or '-inf'")
    K = int(nstarts)
    if not 1 <= K <= MAX_TOY_STARTS:
        raise ValueError("nstarts must be 1 to %d, the starts the shared seeding selects" % MAX_TOY_STARTS)

    def pick(v, name, default):
        return v if v is not None else _opt(args, name, default)
    return K, dict(xatol=float(pick(xatol, "pl_xatol", DEFAULT_XATOL)), fatol=float(pick(fatol, "pl_fatol", DEFAULT_FATOL)),
                maxiter=pick(maxiter, "pl_maxiter", None), adaptive=bool(pick(adaptive, "pl_adaptive", True)),
                restarts=int(pick(restarts, "pl_restarts", DEFAULT_RESTARTS)), on_nonunitary=on_nonunitary)


def _polish(models, cols, bases, labels, sel, nu_seeds, T, per_run, opts, keyword, meas, widths, per_scale):
    """The selected seeds of every (scale, realisation) polished, `per_run` realisations per maximiser, whose `keyword` carries the runs'
    own measurements (`meas` per scale when `per_scale`, `widths` [T] first).  Returns (res [T][S] arrays, dead [S])."""
    S, ndim = len(models), len(bases[0])
    res = dict(max_lnl=np.full((T, S), -np.inf), argmax_theta=np.full((T, S, ndim), np.nan), nstarts=np.zeros((T, S), np.int32),
               nfev=np.zeros((T, S), np.int64), niter=np.zeros((T, S), np.int64), nonunitary=np.zeros((T, S), np.uint32),
               parked=np.zeros((T, S), np.uint32), failed=np.zeros((T, S), bool))
    dead = (nu_seeds > 0) if opts["on_nonunitary"] == "raise" else np.zeros(S, bool)
    res["failed"][:, dead] = True
    count = sel["count"]                                              # [S][T]
    for lo in range(0, T, per_run):
        hi = min(T, lo + per_run)
        ss, tt = np.nonzero(np.broadcast_to(~dead[:, None], (S, hi - lo)))
        if len(ss) == 0:
            continue
        tt = tt + lo
        order = np.lexsort((ss, tt))                                  # realisation by realisation, its scales in order
        ss, tt = ss[order], tt[order]
        # a run with fewer than K finite seeds keeps that many starts; the rows behind them are never evaluated
        with SimplexMaximizer([models[s] for s in ss], cols, [bases[s] for s in ss], nstarts=0, nseed=0,
                              starts=np.nan_to_num(sel["cube"][ss, tt], nan=0.5), start_counts=count[ss, tt],
                              labels=["realisation %d, %s" % (t, labels[s]) for s, t in zip(ss, tt)],
                              **{keyword: (meas[ss, tt] if per_scale else meas[tt], widths[tt])}, **opts) as mx:
            r = mx.run(check=False)
        for k in res:
            res[k][tt, ss] = r[k]
    return res, dead


def _statistic(res, dead, labels, scales, threshold, check):
    """ts and limits of a polished scan into `res`; AssertionError for a failed run when `check`"""
    if check and res["failed"].any():
        t, s = np.argwhere(res["failed"])[0]
        what = "a seed point of" if dead[s] else "realisation %d," % t
        raise AssertionError("Matrix is not unitary! ({0} {1})".format(what, labels[s]))
    null = int(np.argmin(scales))
    with np.errstate(invalid="ignore"):
        res["ts"] = -2.0 * (res["max_lnl"] - res["max_lnl"][:, null:null + 1])
    limits = np.full(len(res["max_lnl"]), np.nan)
    for t in range(len(limits)):
        lim = profile_likelihood_limit(scales, res["max_lnl"][t], threshold)
        if lim is not None:
            limits[t] = lim
    res["limits"] = limits


def _starts_of(sel):
    """the selection as a scan reports it: [T][S] first"""
    return dict(start_cube=np.ascontiguousarray(sel["cube"].transpose(1, 0, 2, 3)), start_score=np.ascontiguousarray(sel["score"].transpose(1, 0, 2)),
                start_count=np.ascontiguousarray(sel["count"].T))


def binned_realisation_scan(args, asimov_paramset, llh_paramset, scales, binned, measurements=None, ntoys=None, toy_seed=0, sigmas=None,
                            nstarts=DEFAULT_TOY_STARTS, nseed=None, run_ids=None, xatol=None, fatol=None, maxiter=None, restarts=None,
                            adaptive=None, seed=None, on_nonunitary="raise", smearing=None, device=0, batch=None, threshold=None, check=True):
    """realisation_scan for the energy-resolved likelihood: the profile likelihood of T realisations of the
    `llh.BinnedMeasurement` `binned` at every scale, with profile_scan(binned=...)'s conventions and seed points.

    measurements: [T][nb][3], shared by all scales, or [S][T][nb][3]; None: `ntoys` realisations by
    draw_binned_realisations(binned, ntoys, toy_seed).  sigmas: [nb], shared by the realisations (default: binned.sigma), or [T][nb].
    Everything else, and the dict returned, as realisation_scan: max_lnl[t, s] is the maximum under (m_t, sigma_t), `measurements` is
    [T][nb][3] (or [S][T][nb][3]) and `sigmas` [T][nb] takes the place of `smearings`."""
    K, opts = _scan_options(args, nstarts, xatol, fatol, maxiter, adaptive, restarts, on_nonunitary)
    scales = np.asarray(scales, dtype=np.float64)
    S, nb = len(scales), binned.nbins
    if measurements is None:
        if ntoys is None:
            raise ValueError("give measurements or ntoys")
        measurements = draw_binned_realisations(binned, ntoys, toy_seed)
    meas = np.ascontiguousarray(measurements, dtype=np.float64)
    if meas.ndim not in (3, 4) or meas.shape[-2:] != (nb, 3) or (meas.ndim == 4 and meas.shape[0] != S):
        raise ValueError("measurements must be [T][%d][3] or [S][T][%d][3]" % (nb, nb))
    T = meas.shape[-3]
    sg = np.asarray(binned.sigma if sigmas is None else sigmas, dtype=np.float64)
    if sg.shape not in ((nb,), (T, nb)):
        raise ValueError("sigmas must be [%d], shared by the realisations, or [T][%d]" % (nb, nb))
    sgs = np.ascontiguousarray(np.broadcast_to(sg, (T, nb)))
    return _scan(BinnedToySeeds, "binned_measurements", meas, sgs, meas.ndim == 4, dict(sigmas=sgs), args, asimov_paramset, llh_paramset, scales,
                 K, nseed, run_ids, opts, seed, smearing, device, batch, threshold, check, binned=binned)


def sensitivity_band(limits, quantiles=BAND_QUANTILES):
    """The band of the limits over realisations: dict(quantiles, limits (np.percentile of the realisations that have a limit; NaN
    when none has), n, n_without_limit).  `limits`: realisation_scan's, NaN or None where a realisation sets no limit."""
    lim = np.array([np.nan if v is None else v for v in np.asarray(limits, dtype=object).ravel()], dtype=np.float64)
    have = lim[np.isfinite(lim)]
    q = np.asarray(quantiles, dtype=np.float64)
    vals = np.percentile(have, q) if len(have) else np.full(len(q), np.nan)
    return dict(quantiles=q, limits=vals, n=int(len(lim)), n_without_limit=int(len(lim) - len(have)))


def ts_quantiles(ts, q=95.):
    """The empirical critical value of the test statistic per scale: the q-th percentile (q a number or a list) over the realisations
    (axis 0) whose statistic is finite there; NaN for a scale without one.  [S], or [len(q)][S].  To hold against Wilks' chi2.ppf(0.95, 1)
    = 3.84, profile_likelihood_limit's default threshold, which this replaces for nobody: pass it as `threshold` if you want it."""
    ts = np.asarray(ts, dtype=np.float64)
    qq = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.full((len(qq), ts.shape[1]), np.nan)
    for s in range(ts.shape[1]):
        col = ts[:, s][np.isfinite(ts[:, s])]
        if len(col):
            out[:, s] = np.percentile(col, qq)
    return out if np.ndim(q) else out[0]


SAVED = ("scales", "measurements", "smearings", "max_lnl", "ts", "argmax_theta", "nstarts", "nfev", "niter", "nonunitary",
         "nonunitary_seeds", "failed", "limits")


def save_realisations(path, res, quantiles=BAND_QUANTILES):
    """realisation_scan's arrays plus the band (band_quantiles, band_limits, band_without_limit) as one .npz; returns the band."""
    band = sensitivity_band(res["limits"], quantiles)
    with open(path, "wb") as fh:
        np.savez(fh, band_quantiles=band["quantiles"], band_limits=band["limits"], band_without_limit=np.int64(band["n_without_limit"]),
                 seconds=np.float64(res["seconds"]), **{k: res[k] for k in SAVED})
    return band


def evidence_limits(scales, lnz, k=nested.BAYES_K, ess_fraction=None, min_ess_fraction=None):
    """nested.bayes_factor_limit(scales, lnz[t], k) for every realisation t of lnz [T][S]: dict(limits [T] (NaN where it returns None
    or raises 'Discovered LV!'), discovered [T] (it raised), low_ess [T]).  min_ess_fraction (a user's cut, off by default) with
    ess_fraction [T][S]: a realisation with any scale below it gets limit NaN and is flagged in low_ess.  A row that holds a NaN or an
    infinity (a run without a posterior, a realisation no point carries weight under) has no limit."""
    scales = np.asarray(scales, dtype=np.float64)
    lnz = np.asarray(lnz, dtype=np.float64)
    T = lnz.shape[0]
    limits, discovered, low = np.full(T, np.nan), np.zeros(T, bool), np.zeros(T, bool)
    if min_ess_fraction is not None:
        with np.errstate(invalid="ignore"):
            low = ~(np.asarray(ess_fraction, dtype=np.float64) >= float(min_ess_fraction)).all(axis=1)
    for t in range(T):
        if low[t] or not np.all(np.isfinite(lnz[t])):
            continue
        try:
            lim = nested.bayes_factor_limit(scales, lnz[t], k)
        except AssertionError as exc:
            if "Discovered LV!" not in str(exc):
                raise
            discovered[t] = True
            continue
        if lim is not None:
            limits[t] = lim
    return dict(limits=limits, discovered=discovered, low_ess=low)


def evidence_realisation_scan(args, asimov_paramset, llh_paramset, scales, measurements=None, ntoys=None, toy_seed=0, smearings=None,
                              k=nested.BAYES_K, min_ess_fraction=None, run_ids=None, nlive=None, tol=None, batch=None, walks=None, seed=None,
                              on_nonunitary="raise", smearing=None, device=0, max_iter=100000, posterior=None, binned=None):
    """The evidence of T realisations at every scale from ONE evidence scan (`nested.evidence_scan`, whose nested options these are):
    the scan's runs keep their points, and `NestedSampler.reweight_evidence` gives ln Z of every (realisation, scale) from them
    (DESIGN.md 6k).

    measurements: [T][3], shared by all scales, or [S][T][3]; None: `ntoys` realisations of the model's own measurement by
    draw_realisations(bf, smearing, ntoys, toy_seed), as realisation_scan draws them for the same seed.  smearings: [T], default the
    model's.  Returns dict(scales, measurements, smearings, lnz [T][S], ess [T][S], ess_fraction (ess over the run's own posterior()
    ESS), kept [T][S], max_x [T][S], lnz_run, lnz_err_run, ess_run [S] (the Asimov run), bayes [T][S] = lnz - lnz[:, null] (the null
    the smallest scale), limits [T] (nested.bayes_factor_limit(scales, lnz[t], k); NaN where it returns None or raises 'Discovered
    LV!'), discovered [T] (it raised), low_ess [T] and n_low_ess (min_ess_fraction: evidence_limits), asimov (evidence_scan's own
    result), seconds, seconds_nested, seconds_reweight).  Every realisation of a scale shares that run's compression error lnz_err_run:
    their lnz are correlated through it, and the band of the limits does not include it."""
    if binned is not None:
        raise ValueError("realisations are of the flux-averaged Gaussian likelihood; the energy-resolved one is not supported")
    scales = np.asarray(scales, dtype=np.float64)
    sm0, meas, sms = _gaussian_measurements(args, asimov_paramset, len(scales), measurements, ntoys, toy_seed, smearings, smearing)
    t0 = time.perf_counter()
    run = nested.evidence_scan(args, asimov_paramset, llh_paramset, scales, run_ids=run_ids, nlive=nlive, tol=tol, batch=batch, walks=walks,
                               seed=seed, on_nonunitary=on_nonunitary, smearing=sm0, device=device, max_iter=max_iter, return_sampler=True,
                               posterior=posterior)
    sampler, models = run.pop("sampler"), run.pop("models")
    try:
        t1 = time.perf_counter()
        rw = sampler.reweight_evidence(meas, sms)
        t2 = time.perf_counter()
        ess_run = sampler.posterior()["ess"]
    finally:
        sampler.close()
        for m in models:
            m.close()
    null = int(np.argmin(scales))
    with np.errstate(invalid="ignore", divide="ignore"):
        bayes = rw["lnz"] - rw["lnz"][:, null:null + 1]
        frac = rw["ess"] / ess_run[None, :]
    lim = evidence_limits(scales, rw["lnz"], k, frac, min_ess_fraction)
    return dict(scales=scales, measurements=meas, smearings=sms, lnz=rw["lnz"], ess=rw["ess"], ess_fraction=frac, kept=rw["kept"],
                max_x=rw["max_x"], lnz_run=run["lnz"], lnz_err_run=run["lnz_err"], ess_run=ess_run, bayes=bayes, limits=lim["limits"],
                discovered=lim["discovered"], low_ess=lim["low_ess"], n_low_ess=int(lim["low_ess"].sum()), asimov=run,
                seconds=t2 - t0, seconds_nested=t1 - t0, seconds_reweight=t2 - t1)


EVIDENCE_SAVED = ("scales", "measurements", "smearings", "lnz", "ess", "ess_fraction", "kept", "lnz_run", "lnz_err_run", "ess_run", "bayes",
                  "limits", "discovered", "low_ess")


def save_evidence_realisations(path, res, quantiles=BAND_QUANTILES):
    """evidence_realisation_scan's arrays plus the band of the limits (band_quantiles, band_limits, band_without_limit) as one .npz;
    returns the band."""
    band = sensitivity_band(res["limits"], quantiles)
    with open(path, "wb") as fh:
        np.savez(fh, band_quantiles=band["quantiles"], band_limits=band["limits"], band_without_limit=np.int64(band["n_without_limit"]),
                 seconds=np.float64(res["seconds"]), seconds_nested=np.float64(res["seconds_nested"]),
                 seconds_reweight=np.float64(res["seconds_reweight"]), **{k: res[k] for k in EVIDENCE_SAVED})
    return band
