"""Reweighting a stored chain to other targets (include/golemflavor_hip.h `gf_sampler_reweight*`).

A chain sampled under one model carries the posterior of any other model it covers: weight the stored samples by
exp(ln_prob_target - ln_prob_sampled).  `DeviceEnsembleSampler.reweight(targets)` does this where the chain lies; this module holds the
target types, a numpy restatement of the definitions (`reweight_host`, for tests and documentation) and the result object.

Rows are in the DEVICE's storage order, i = step * nwalkers + walker -- `DeviceEnsembleSampler.flat_steps()`, not emcee's walker-major
`flatchain`; every `index` returned here refers to that order.
"""
import ctypes as C

import numpy as np

from . import _lib, rowsets
from ._lib import GF_REWEIGHT_MAX_TARGETS, GF_ST_NON_UNITARY, GfReweightOut, GfReweightSpec


class Measurement:
    """A measurement target: the chain's own sampling model with the measured composition, its smearing and the offset replaced.
    Give the composition as bestfit_fr, or as injected_ratio (normalised to sum 1, as the scripts treat --injected-ratio); smearing and
    offset default to the sampling model's own."""

    def __init__(self, bestfit_fr=None, injected_ratio=None, smearing=None, offset=None):
        if (bestfit_fr is None) == (injected_ratio is None):
            raise ValueError("give exactly one of bestfit_fr and injected_ratio")
        f = np.asarray(bestfit_fr if injected_ratio is None else injected_ratio, dtype=np.float64)
        if f.shape != (3,) or not np.all(np.isfinite(f)):
            raise ValueError("a composition has three finite components")
        if injected_ratio is not None:
            if np.any(f < 0.0) or not float(np.sum(f)) > 0.0:
                raise ValueError("an injected ratio has non-negative components and a positive sum")
            f = f / float(np.sum(f))
        if smearing is not None and not float(smearing) > 0.0:
            raise ValueError("smearing must be positive")
        self.bestfit_fr = f
        self.smearing = None if smearing is None else float(smearing)
        self.offset = None if offset is None else float(offset)

    def __repr__(self):
        return "Measurement(bestfit_fr=%r, smearing=%r, offset=%r)" % (tuple(self.bestfit_fr), self.smearing, self.offset)


def _is_model(x):
    return hasattr(getattr(x, "model", x), "_h")


def parse_targets(targets, nchains):
    """targets: one list applied to every chain, or one list per chain -> (kind, [chain][target]), kind "measurement" or "model".
    Every chain has the same number of targets, 1 to GF_REWEIGHT_MAX_TARGETS, all of one kind."""
    targets = list(targets)
    if not targets:
        raise ValueError("no targets")
    if all(isinstance(t, (list, tuple)) for t in targets):
        if len(targets) != nchains:
            raise ValueError("%d lists of targets for %d chains" % (len(targets), nchains))
        per = [list(t) for t in targets]
    elif any(isinstance(t, (list, tuple)) for t in targets):
        raise ValueError("targets is one list for every chain or one list per chain, not a mixture")
    else:
        per = [list(targets) for _ in range(nchains)]
    T = len(per[0])
    if any(len(p) != T for p in per):
        raise ValueError("every chain needs the same number of targets")
    if T < 1 or T > GF_REWEIGHT_MAX_TARGETS:
        raise ValueError("1 to %d targets per chain, got %d" % (GF_REWEIGHT_MAX_TARGETS, T))
    flat = [t for p in per for t in p]
    if all(isinstance(t, Measurement) for t in flat):
        return "measurement", per
    if all(_is_model(t) for t in flat):
        return "model", per
    raise TypeError("targets are all Measurement or all Model / LnProb; the two kinds do not mix in one call")


def lnw_host(lnprob_target, lnprob, status=None):
    """csrc/gf_reweight.hpp in numpy: (lnw, kind) with kind 0 kept, 1 bad base, 2 non-unitary, 3 outside; one rounded subtraction."""
    lt, l0 = np.asarray(lnprob_target, dtype=np.float64), np.asarray(lnprob, dtype=np.float64)
    st = np.zeros(lt.shape, np.int32) if status is None else np.asarray(status)
    kind = np.zeros(lt.shape, np.int32)
    kind[np.isnan(lt) | np.isneginf(lt)] = 3
    kind[st == GF_ST_NON_UNITARY] = 2
    kind[~np.isfinite(l0)] = 1
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(kind == 0, np.subtract(lt, l0), -np.inf), kind


def reweight_host(rows, lnprob, lnprob_target, status=None, nrows=None, u=0.5):
    """The definitions in numpy for one chain and one target: rows (n, ndim) in storage order, lnprob (n,) what they were sampled
    under, lnprob_target (n,) [status (n,) under the target].  Returns dict(lnw, kind, ess, lnz_ratio, mean, cov, p, C) and, with nrows,
    index / rows of the systematic resampling at t_k = (k + u) / nrows.  No kept row: ess 0, NaN moments, index -1."""
    x = np.asarray(rows, dtype=np.float64)
    n, nd = x.shape
    lnw, kind = lnw_host(lnprob_target, lnprob, status)
    out = dict(lnw=lnw, kind=kind, bad_base=int((kind == 1).sum()), nonunitary=int((kind == 2).sum()), outside=int((kind == 3).sum()))
    if not np.any(kind == 0):
        out.update(ess=0.0, lnz_ratio=np.nan, mean=np.full(nd, np.nan), cov=np.full((nd, nd), np.nan), p=np.zeros(n), C=np.zeros(n))
        if nrows:
            out.update(index=np.full(int(nrows), -1, np.int64), rows=np.full((int(nrows), nd), np.nan))
        return out
    m = lnw.max()
    with np.errstate(under="ignore"):
        e = np.where(np.isneginf(lnw), 0.0, np.exp(lnw - m))
    S = e.sum()
    p = e / S
    out.update(ess=S * S / (e * e).sum(), lnz_ratio=m + np.log(S) - np.log(n), mean=np.average(x, axis=0, weights=p),
               cov=np.atleast_2d(np.cov(x.T, aweights=p)) if n > 1 else np.full((nd, nd), np.nan), p=p, C=np.cumsum(p))
    if nrows:
        t = (np.arange(int(nrows), dtype=np.float64) + u) / float(nrows)
        last = int(np.searchsorted(out["C"], out["C"][-1], side="left"))
        out["index"] = np.minimum(np.searchsorted(out["C"], t, side="right"), last).astype(np.int64)
        out["rows"] = x[out["index"]]
    return out


class Reweighted(rowsets.RowSetSource):
    """What `DeviceEnsembleSampler.reweight` returns: the chains of `sampler` under `targets`.  Everything is computed on the device
    while the sampler holds the chain; the object keeps the sampler and the targets alive.  Layouts are those of the sampler's chain
    methods with a target axis after the chain axis (the chain axis is dropped when nchains == 1).

    The summary is computed when the object is made (`on_nonunitary="raise"` needs its counts) and kept.  Every later call --
    `lnw`, `rows`, `marginals`, `intervals`, `regions` -- is one library call that starts from the chain again: propagation (once for
    all targets), log-weights and the weight pipeline are repeated per call, nothing is carried over between calls but the summary."""

    def __init__(self, sampler, targets, seed=None, on_nonunitary="raise"):
        if on_nonunitary not in ("raise", "-inf"):
            raise ValueError("on_nonunitary must be 'raise' or '-inf'")
        self.sampler, self.on_nonunitary = sampler, on_nonunitary
        self.nchains, self.ndim = sampler.nchains, sampler.dim
        self.kind, self.targets = parse_targets(targets, self.nchains)
        self.ntargets = len(self.targets[0])
        self._L = sampler._L
        self._spec = GfReweightSpec(self.ntargets, 1 if seed is None else 0, 0 if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    None, None, None, None)
        if self.kind == "model":
            ms = [getattr(t, "model", t) for p in self.targets for t in p]
            for m in ms:
                if m.ndim != self.ndim:
                    raise AssertionError("a target has %d parameters, the chain %d columns" % (m.ndim, self.ndim))
            self._keep = rowsets.model_handles(ms, len(ms))
            self._spec.models = self._keep
        else:
            own = sampler.models if sampler.models is not None else [sampler.model] * self.nchains
            bf, sm, off = np.empty((self.nchains, self.ntargets, 3)), np.empty((self.nchains, self.ntargets)), np.empty((self.nchains, self.ntargets))
            for c, p in enumerate(self.targets):
                d = own[c].desc
                for t, tg in enumerate(p):
                    bf[c, t] = tg.bestfit_fr
                    sm[c, t] = d.smearing if tg.smearing is None else tg.smearing
                    off[c, t] = d.offset if tg.offset is None else tg.offset
            self._keep = (bf, sm, off)
            self._spec.bestfit_fr, self._spec.smearing, self._spec.offset = (a.ctypes.data_as(_lib._dp) for a in self._keep)
            self.bestfit_fr, self.smearing, self.offset = bf, sm, off
        self._summary = self._run_summary()
        if on_nonunitary == "raise" and self._summary["nonunitary"].sum():
            raise AssertionError("Matrix is not unitary! (%d rows under the targets)" % int(self._summary["nonunitary"].sum()))

    # rowsets.RowSetSource: one row set per (chain, target), chain-major; the defaults of the sampler's model
    _prefix = "gf_sampler_reweight_"
    _nsets = property(lambda self: self.nchains * self.ntargets)
    _ncols = property(lambda self: self.ndim)

    def _desc0(self):
        return self.sampler.model.desc

    def _lead(self, N):
        return (self.sampler._h, C.byref(self._spec), int(N))

    def _sq(self, a):
        return a[0] if self.nchains == 1 else a

    def _shape(self, per_set):
        """[chain][target] of a per-set list, (nchains, ntargets) leading in an array; the chain level dropped for a single chain"""
        T = self.ntargets
        if isinstance(per_set, np.ndarray):
            return self._sq(per_set.reshape((self.nchains, T) + per_set.shape[1:]))
        return self._sq([per_set[c * T:(c + 1) * T] for c in range(self.nchains)])

    def _run_summary(self):
        nc, T, d = self.nchains, self.ntargets, self.ndim
        a = dict(ess=np.zeros((nc, T)), lnz_ratio=np.zeros((nc, T)), mean=np.zeros((nc, T, d)), cov=np.zeros((nc, T, d, d)),
                 bad_base=np.zeros(nc, np.int64), nonunitary=np.zeros((nc, T), np.int64), outside=np.zeros((nc, T), np.int64), n=np.zeros(nc, np.int64))
        out = GfReweightOut(**{k: a[k].ctypes.data_as(_lib._lp if a[k].dtype == np.int64 else _lib._dp) for k, _ in GfReweightOut._fields_})
        _lib.check(self._L.gf_sampler_reweight(self.sampler._h, C.byref(self._spec), C.byref(out)), "gf_sampler_reweight")
        return a

    def summary(self):
        """dict(ess (Kish), lnz_ratio, mean, cov, nonunitary, outside: (nchains, ntargets, ...); bad_base, n: (nchains,)).  lnz_ratio =
        max lnw + log sum exp(lnw - max) - log n is a diagnostic that estimates ln(Z_target / Z_sampled); it is a Bayes factor only for
        model targets on the same data.  A target whose weights are all zero has ess 0 and NaN lnz_ratio, mean and cov."""
        return {k: self._sq(v) for k, v in self._summary.items()}

    def lnw(self, chain=0):
        """The log-weights of one chain, (ntargets, n), rows in the device's storage order (step-major: `flat_steps()`)."""
        n = int(self._summary["n"][int(chain)])
        out = np.empty((self.ntargets, n))
        _lib.check(self._L.gf_sampler_reweight_lnw(self.sampler._h, C.byref(self._spec), int(chain), out.ctypes.data_as(_lib._dp)),
                   "gf_sampler_reweight_lnw")
        return out

    def rows(self, N, with_fr=False, return_index=False):
        """N equal-weight rows per (chain, target) by systematic resampling, (nchains, ntargets, N, ndim) -- with_fr: the row's
        composition under the target in front.  return_index: also (nchains, ntargets, N) int64, the row of the chain in the device's
        storage order (i = step * nwalkers + walker, NOT emcee's flatchain order) each came from; -1 and NaN rows for a target without
        a posterior."""
        if int(N) < 1:
            raise ValueError("N must be at least 1")
        width = (3 if with_fr else 0) + self.ndim
        rows = np.empty((self.nchains, self.ntargets, int(N), width))
        index = np.empty(rows.shape[:3], np.int64)
        _lib.check(self._L.gf_sampler_reweight_rows(self.sampler._h, C.byref(self._spec), int(N), int(bool(with_fr)),
                                                    rows.ctypes.data_as(_lib._dp), index.ctypes.data_as(_lib._lp)), "gf_sampler_reweight_rows")
        return (self._sq(rows), self._sq(index)) if return_index else self._sq(rows)

    def marginals(self, N, ranges=None, with_fr=False, names=None, **kw):
        """`DeviceEnsembleSampler.marginals`' reduction of the N equal-weight rows of every (chain, target), which stay on the device:
        [chain][target] `marginals.MarginalResult`."""
        return self._marginals(self._lead(N), ranges, names, with_fr, kw)

    def intervals(self, N, percentiles=(68., 90.), with_fr=False):
        """`DeviceEnsembleSampler.intervals`' dict for the N equal-weight rows, with (nchains, ntargets) leading."""
        return self._intervals(self._lead(N), percentiles, with_fr)

    def regions(self, N, nbins, coverage, hist_smooth=0.05, oversample=1., truncate=4.0, cap=None):
        """`DeviceEnsembleSampler.regions`' reduction of the compositions of the N equal-weight rows: [chain][target]
        `contour.RegionResult` (lists of them for several coverages)."""
        return self._regions(self._lead(N), nbins, coverage, hist_smooth, oversample, truncate, cap)
