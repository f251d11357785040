"""Nested sampling on the device: the Bayesian evidence golemflavor/mn.py asks MultiNest for, at every new-physics scale of
scripts/sens.py, computed for all scales in one set of launches (gf_nested.hip, include/golemflavor_hip.h gf_nested_*).

The semantics are the reference's (mn.py:22-45): the prior is uniform on the unit cube of the scanned columns, the
log-likelihood is the full ln_prob (lnprior + llh) of theta, theta_i = (hi_i - lo_i) u_i + lo_i on the scanned columns, the
paramset's value elsewhere; so Z = int_[0,1]^n exp(ln_prob(theta(u))) du.  Each iteration removes the `batch` lowest live points
(the j-th removed sees nlive - j live points: dynamic nested sampling, Higson et al. 2019) and replaces them by constrained
Metropolis walks started from survivors above L*; the run stops at MultiNest's evidence tolerance ln(Z + L_max X) - ln Z < tol.
Points of zero likelihood (lnL = -inf) are never replaced by such points, so the i-th of them removed in a run sees nlive - i
live points, whatever the batch (nlive_sequence; Fowlie, Handley & Su 2021).

    NestedSampler          the device sampler over several posteriors (one run each)
                           and their posterior: posterior(), posterior_rows(), marginals(), regions() (gf_nested_post.hip);
                           reweight_evidence(): every run's evidence under other Gaussian measurements (gf_ns_toys.hip)
    mn_evidence            mn.py:71-108, same name and return: (ln Z, max ln L)
    evidence_scan          sens.py's loop over scales in one device call
    evidence_from_dead     the accounting restated on the host (the tests' reference for the device accumulators)
    bayes_factor_limit     plot.py:149-213 get_limit, BAYESIAN branch
"""
import copy
import ctypes as C
import math

import numpy as np

from . import _lib
from . import configs as Cf
from . import fr as fr_utils
from . import rowsets
from .descriptor import compile_model
from .enums import ParamTag
from .model import Model

__all__ = ["NestedSampler", "mn_evidence", "evidence_scan", "evidence_from_dead", "evidence_lnz", "nlive_sequence", "bayes_factor_limit",
           "sens_scales", "BAYES_K"]

BAYES_K = 1.0                 # golemflavor/plot.py: Bayes factor threshold 10^K
DEFAULT_NLIVE = 3000          # mn.py:51-53 --mn-live-points
DEFAULT_TOL = 0.01            # mn.py:55-57 --mn-tolerance
DEFAULT_WALKS = 25


class _CubeRuns:
    """What NestedSampler and SimplexMaximizer share: `nruns` runs, run r on posterior models[r] (Model or LnProb; they share
    device, ndim and mode and must stay open while the object lives) over the unit cube of the columns `cols` (indices into
    theta), every other column at `bases` ([nruns][ndim] or [ndim]); the device object of the C ABI's gf_<_abi>_* calls.
    `run_ids`: the Philox stream of each run (default 0..nruns-1); a scan passes each point's index in its full list so that a
    point's result does not depend on what else shares the call.  `labels`: what an AssertionError names for a failed run
    (default: the run index).  A table or binned measurement replaced on a model before the first run() is what the runs evaluate; one
    replaced after the runs have begun, or given to a model that had none when the object was created, makes run() raise
    GolemHipError (GF_ERR_INVALID_ARG) -- results so far stay readable."""
    _abi = None                 # "nested" or "simplex"
    _what = None                # a run's name in the AssertionError

    def _open(self, models, cols, bases, on_nonunitary, labels):
        """Checks and keeps the common arguments; returns the models' handles for gf_<_abi>_create."""
        if on_nonunitary not in ("raise", "-inf"):
            raise ValueError("on_nonunitary must be 'raise' or '-inf'")
        self._L = _lib.lib()
        self.models = list(models)
        self.nruns = len(self.models)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32)
        self.nscan = len(self.cols)
        ndim = self._L.gf_model_ndim(rowsets.handle(self.models[0]))
        b = np.asarray(bases, dtype=np.float64)
        if b.ndim == 1:
            b = np.tile(b, (self.nruns, 1))
        self.bases = np.ascontiguousarray(b.reshape(self.nruns, ndim))
        self.on_nonunitary = on_nonunitary
        self.labels = list(labels) if labels is not None else list(range(self.nruns))
        return rowsets.model_handles(self.models, self.nruns)

    def _set_run_ids(self, run_ids):
        if run_ids is not None:
            ids = np.ascontiguousarray(run_ids, dtype=np.uint64)
            name = "gf_{0}_set_run_ids".format(self._abi)
            _lib.check(getattr(self._L, name)(self._h, ids.ctypes.data_as(C.POINTER(C.c_uint64))), name)

    def _checked(self, res, check):
        """res, or AssertionError for the first run that failed on a non-unitary point (on_nonunitary == 'raise') when `check`."""
        if check and self.on_nonunitary == "raise" and res["failed"].any():
            r = int(np.argmax(res["failed"]))
            raise AssertionError("Matrix is not unitary! ({0} {1}: {2})".format(self._what, r, self.labels[r]))
        return res

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, "gf_{0}_destroy".format(self._abi))(self._h)
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


class NestedSampler(_CubeRuns, rowsets.RowSetSource):
    """`nruns` independent nested-sampling runs (_CubeRuns: models, cols, bases, run_ids, labels)."""
    _abi, _what = "nested", "nested run"

    def __init__(self, models, cols, bases, nlive=DEFAULT_NLIVE, batch=None, walks=DEFAULT_WALKS, seed=0,
                 on_nonunitary="raise", tol=DEFAULT_TOL, run_ids=None, labels=None):
        hs = self._open(models, cols, bases, on_nonunitary, labels)
        self.nlive = int(nlive)
        self.batch = int(batch) if batch is not None else max(1, self.nlive // 8)
        self.walks = int(walks)
        self.seed = int(seed)
        h = C.c_void_p()
        _lib.check(self._L.gf_nested_create(hs, self.nruns, self.nscan, self.cols.ctypes.data_as(_lib._ip),
                                            self.bases.ctypes.data_as(_lib._dp), self.nlive, self.batch, self.walks,
                                            self.seed & 0xFFFFFFFFFFFFFFFF, 0 if on_nonunitary == "raise" else 1, C.byref(h)),
                   "gf_nested_create")
        self._h = h
        _lib.check(self._L.gf_nested_set_tolerance(self._h, float(tol)), "gf_nested_set_tolerance")
        self._set_run_ids(run_ids)

    def run(self, max_iter=100000, check=True):
        """Iterate every run to its tolerance; returns result(), raising AssertionError for a run that met a proposal the
        reference would have raised on (on_nonunitary == 'raise', sens.py:283-285) when `check`."""
        _lib.check(self._L.gf_nested_run(self._h, int(max_iter)), "gf_nested_run")
        return self._checked(self.result(), check)

    def result(self):
        n = self.nruns
        out = {k: np.zeros(n) for k in ("lnz", "lnz_err", "info", "max_lnl")}
        it, ev = np.zeros(n, np.int64), np.zeros(n, np.int64)
        nu, fl = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        _lib.check(self._L.gf_nested_result(self._h, *[out[k].ctypes.data_as(_lib._dp) for k in ("lnz", "lnz_err", "info", "max_lnl")],
                                            it.ctypes.data_as(C.POINTER(C.c_int64)), ev.ctypes.data_as(C.POINTER(C.c_int64)),
                                            nu.ctypes.data_as(C.POINTER(C.c_uint32)), fl.ctypes.data_as(_lib._ip)),
                   "gf_nested_result")
        out.update(niter=it, nevals=ev, nonunitary=nu, failed=fl.astype(bool))
        return out

    def dead(self, run=0):
        """Run `run`'s dead points in removal order, then its final live set: dict(lnl, lnw (log-weights), cube, theta,
        nlive_seq (live points each removed point saw), ndead (removed points; the rest is the final live set))."""
        n = C.c_int64(0)
        _lib.check(self._L.gf_nested_get_dead(self._h, int(run), 0, None, None, None, C.byref(n)), "gf_nested_get_dead")
        n = n.value
        lnl, lnw = np.empty(n), np.empty(n)
        cube = np.empty((n, len(self.cols)))
        m = C.c_int64(0)
        _lib.check(self._L.gf_nested_get_dead(self._h, int(run), n, lnl.ctypes.data_as(_lib._dp), lnw.ctypes.data_as(_lib._dp),
                                              cube.ctypes.data_as(_lib._dp), C.byref(m)), "gf_nested_get_dead")
        ndead = n - self.nlive
        seq = nlive_sequence(lnl[:ndead], self.nlive, self.batch)
        desc = getattr(self.models[run], "model", self.models[run]).desc
        lo, hi = np.asarray(desc.lo)[self.cols], np.asarray(desc.hi)[self.cols]
        theta = np.tile(self.bases[run], (n, 1))
        theta[:, self.cols] = (hi - lo) * cube + lo          # mn.py:35-36
        return dict(lnl=lnl, lnw=lnw, cube=cube, theta=theta, nlive_seq=seq, ndead=ndead)

    # ---- the posterior of every run, computed on the device from the points dead() would read back -------------
    @property
    def ndim(self):
        return self.bases.shape[1]

    # rowsets.RowSetSource: one row set per run, the defaults of run 0's model, the run axis never dropped
    _prefix, _sets, _ncols = "gf_nested_", "runs", ndim
    _nsets = property(lambda self: self.nruns)

    def _desc0(self):
        return getattr(self.models[0], "model", self.models[0]).desc

    def _shape(self, per_run):
        return per_run

    def posterior(self):
        """Per run: dict(npoints, ess (Kish), lnz_check (= max lnw + log sum exp, a diagnostic), mean (nruns, ndim), cov (nruns,
        ndim, ndim)) of the weighted points, theta full-width.  A run without a posterior (not run, failed, ln Z = -inf) has
        npoints 0, ess 0 and NaN elsewhere."""
        n, d = self.nruns, self.ndim
        out = dict(npoints=np.zeros(n, np.int64), ess=np.zeros(n), lnz_check=np.zeros(n), mean=np.zeros((n, d)), cov=np.zeros((n, d, d)))
        _lib.check(self._L.gf_nested_posterior(self._h, out["npoints"].ctypes.data_as(_lib._lp), *[out[k].ctypes.data_as(_lib._dp)
                                               for k in ("ess", "lnz_check", "mean", "cov")]), "gf_nested_posterior")
        return out

    def reweight_evidence(self, measurements, smearings=None):
        """The evidence of every run under other Gaussian measurements, from the points the runs keep (DESIGN.md 6k;
        gf_nested_toys_evidence): ln Z_t = ln sum_i exp(lnw_i + l_t(fr_i) - l_0(fr_i)) over dead()'s points, l_0 the Gaussian of the
        run's own measurement, l_t that of realisation t.  measurements: [T][3], shared by the runs, or [nruns][T][3]; smearings: [T]
        or one value, default the runs' models' own (which they must then share, as a scan's do).  Returns dict(lnz, ess (Kish), kept (the
        points that carry weight), max_x), each [T][nruns].  A realisation equal to a run's own measurement gives posterior()'s
        lnz_check and ess bit for bit; the error of lnz is the run's own lnz_err, shared by all its realisations.  No kept point:
        lnz -inf, ess 0.  A run without a posterior (not run, failed, ln Z = -inf): lnz NaN, ess 0, kept 0."""
        bf = np.ascontiguousarray(measurements, dtype=np.float64)
        if bf.ndim not in (2, 3) or bf.shape[-1] != 3 or bf.shape[-2] < 1 or (bf.ndim == 3 and bf.shape[0] != self.nruns):
            raise ValueError("measurements must be [T][3] or [nruns][T][3]")
        T = bf.shape[-2]
        if smearings is None:
            own = {float(getattr(getattr(m, "model", m).desc, "smearing", np.nan)) for m in self.models}
            if len(own) != 1 or not np.isfinite(next(iter(own))):
                raise ValueError("the runs' models do not share one smearing: give smearings")
            smearings = own.pop()
        sm = np.ascontiguousarray(np.broadcast_to(np.asarray(smearings, dtype=np.float64), (T,)))
        n = self.nruns
        m, s, s2, ess = (np.empty((n, T)) for _ in range(4))
        kept = np.empty((n, T), np.int64)
        _lib.check(self._L.gf_nested_toys_evidence(self._h, bf.ctypes.data_as(_lib._dp), sm.ctypes.data_as(_lib._dp), T, int(bf.ndim == 3),
                                                   *[a.ctypes.data_as(_lib._dp) for a in (m, s, s2, ess)], kept.ctypes.data_as(_lib._lp)),
                   "gf_nested_toys_evidence")
        return dict(lnz=evidence_lnz(m, s).T.copy(), ess=ess.T.copy(), kept=kept.T.copy(), max_x=m.T.copy())

    def posterior_rows(self, nrows, with_fr=False, return_index=False):
        """`nrows` equal-weight rows per run by systematic resampling, (nruns, nrows, ndim) -- with_fr: (nruns, nrows, 3 + ndim),
        the composition of the run's model in front, NaN where the reference would have raised.  return_index: also (nruns, nrows)
        int64, the point of dead() each row came from.  A run without a posterior gives NaN rows and index -1."""
        width = (3 if with_fr else 0) + self.ndim
        rows = np.empty((self.nruns, int(nrows), width) if nrows >= 1 else (self.nruns, 0, width))
        index = np.empty(rows.shape[:2], np.int64)
        _lib.check(self._L.gf_nested_posterior_rows(self._h, int(nrows), int(bool(with_fr)), rows.ctypes.data_as(_lib._dp),
                                                    index.ctypes.data_as(_lib._lp)), "gf_nested_posterior_rows")
        return (rows, index) if return_index else rows

    def marginals(self, nrows, ranges=None, space="angles", llh_paramset=None, with_fr=False, names=None, round32=True, **prepare_kwargs):
        """One `marginals.MarginalResult` per run of its `nrows` equal-weight rows, which stay on the device (`marginals.prepare`'s
        keyword arguments: bins_1d, bins_2d, coverage, percentiles, ranks, hist_smooth, truncate; cap_2d).  space="angles": the
        theta columns (with_fr: the composition in front), ranges default to the box of the run-0 model and (0, 1);
        space="elements": `elements.element_plan(llh_paramset, round32)`'s row, names and ranges the plan's."""
        if space not in ("angles", "elements"):
            raise ValueError("space must be 'angles' or 'elements'")
        return self._marginals((self._h, int(nrows)), ranges, names, with_fr, prepare_kwargs, space == "elements" and (llh_paramset, round32, None))

    def intervals(self, nrows, percentiles=(68., 90.), with_fr=False):
        """The reference's shortest interval around the mode (`misc.interval`) of every column of every run's `nrows` equal-weight
        rows, which stay on the device: `intervals.chain_intervals`'s dict with a leading run axis.  A run without a posterior has
        NaN rows: status 1."""
        return self._intervals((self._h, int(nrows)), percentiles, with_fr)

    def spectrum(self, nrows, percentiles=(5, 16, 50, 84, 95), bins=50):
        """The composition at every energy bin of every run's `nrows` equal-weight rows, reduced on the device: one
        `spectrum.SpectrumResult` per run.  A run without a posterior has nvalid 0 and NaN moments.  Models without energy bins:
        ValueError."""
        if int(nrows) < 1:
            raise ValueError("nrows must be at least 1")
        return self._spectrum((self._h, int(nrows)), self.models, percentiles, bins)

    def regions(self, nrows, nbins, coverage, hist_smooth=0.05, oversample=1., truncate=4.0, cap=None):
        """The flavor-triangle credible regions (`DeviceEnsembleSampler.regions`'s reduction) of every run's `nrows` equal-weight
        rows propagated with the run's model: [run] of `contour.RegionResult` (of lists of them for several coverages)."""
        return self._regions((self._h, int(nrows)), nbins, coverage, hist_smooth, oversample, truncate, cap)


def _logaddexp(x, y):
    if x == -math.inf:
        return y
    if y == -math.inf:
        return x
    m = x if x > y else y
    return m + math.log1p(math.exp(-abs(x - y)))


def evidence_lnz(max_x, s):
    """ln Z = max_x + log(s) elementwise with the C library's log (math.log), the expression gf_nested_posterior forms lnz_check
    with; s = 0 (no point carries weight) gives -inf, a NaN gives NaN."""
    max_x, s = np.asarray(max_x, dtype=np.float64), np.asarray(s, dtype=np.float64)
    out = np.full(s.shape, np.nan)
    flat = out.reshape(-1)
    for i, (m, v) in enumerate(zip(max_x.reshape(-1).tolist(), s.reshape(-1).tolist())):
        if v > 0.0:
            flat[i] = m + math.log(v)
        elif v == 0.0:
            flat[i] = -math.inf
    return out


def nlive_sequence(lnl_dead, nlive, batch):
    """The live points each dead point saw, in removal order (`lnl_dead`: the dead lnL, whole batches).  The j-th point removed
    in a batch sees nlive - j; a point of zero likelihood is removed without replacement over the whole run, so the i-th
    lnL = -inf point of the run (they come first) sees nlive - i."""
    lnl = np.asarray(lnl_dead, dtype=np.float64)
    seq = nlive - np.arange(len(lnl), dtype=np.int64) % int(batch)
    plat = lnl == -np.inf
    seq[plat] = nlive - np.arange(int(plat.sum()), dtype=np.int64)
    return seq


def evidence_from_dead(lnl, nlive_seq, live_lnl=None):
    """The device's accounting on the host.  Dead point i (in removal order, lnL lnl[i]) saw nlive_seq[i] live points:
    ln X_{i+1} = ln X_i - 1/n_i, weight L_i (X_i - X_{i+1}); Z and H (Skilling 2006) accumulate in that order.  `live_lnl`: the
    final live set, added as X mean(L_live) in ascending lnL.  Returns dict(lnz, lnz_err = sqrt(H / n_last + plateau_var), info,
    lnx, plateau_var = sum 1/n_i^2 over the dead points with lnL = -inf: the variance their compression adds to ln X)."""
    lnl = np.asarray(lnl, dtype=np.float64)
    seq = np.asarray(nlive_seq)
    lnz, h, lnx, pvar = -math.inf, 0.0, 0.0, 0.0

    def acc(l, lnw):
        nonlocal lnz, h
        if lnw == -math.inf:
            return
        new = _logaddexp(lnz, lnw)
        if lnz == -math.inf:
            h = math.exp(lnw - new) * l - new
        else:
            h = math.exp(lnw - new) * l + math.exp(lnz - new) * (h + lnz) - new
        lnz = new

    for l, n in zip(lnl.tolist(), seq.tolist()):
        dx = 1.0 / n
        acc(l, l + lnx + math.log(-math.expm1(-dx)))
        lnx -= dx
        if l == -math.inf:
            pvar += dx * dx
    nlast = int(seq[0]) if len(seq) else 1
    if live_lnl is not None:
        live = np.sort(np.asarray(live_lnl, dtype=np.float64))
        nlast = len(live)
        w0 = lnx - math.log(len(live))
        for l in live.tolist():
            acc(l, l + w0)
    return dict(lnz=lnz, lnz_err=math.sqrt(max(h, 0.0) / nlast + pvar), info=h, lnx=lnx, plateau_var=pvar)


def bayes_factor_limit(scales, lnZ, k=BAYES_K):
    """golemflavor/plot.py:149-213 get_limit, BAYESIAN branch: the lowest scale on the splined curve (splprep, s=0, 1000
    points) where the evidence has fallen by more than ln(10^k) below the null point (the smallest scale), minus log10(2)
    (the standard SME coefficient).  None where the reference returns None: no such scale, a curve that does not exclude the
    large scales (two or more scanned points above the crossing within 0.1 of the threshold), or fewer than two scanned points
    above it beyond the threshold.  AssertionError('Discovered LV!') as the reference."""
    from scipy.interpolate import splev, splprep
    scales = np.asarray(scales, dtype=np.float64)
    st = np.asarray(lnZ, dtype=np.float64)
    thr = np.log(10 ** k)
    if (st[0] - np.max(st)) > thr:
        raise AssertionError('Discovered LV!')
    tck, _ = splprep([scales, st], s=0)
    sc, sst = splev(np.linspace(0, 1, 1000), tck)
    null = st[np.argmin(scales)]
    reduced = -(sst - null)
    al = sc[reduced > thr]
    if len(al) == 0:
        return None
    re = -(st - null)[scales > al[0]]
    if np.sum(re < thr - 0.1) >= 2:
        return None
    if np.sum(re >= thr + 0.0) < 2:
        return None
    return al[0] - np.log10(2.)


def sens_scales(dimension, segments):
    """scripts/sens.py:226-229: the null point -100 then linspace over SCALE_BOUNDARIES[d] in segments - 1 steps."""
    b = Cf.SCALE_BOUNDARIES[dimension]
    return np.concatenate([[-100.], np.linspace(b[0], b[1], segments - 1)])


def _scale_paramset(llh_paramset, scale):
    """sens.py:255-263: the scale column fixed at `scale`, its lower boundary lowered for the null point."""
    ps = copy.deepcopy(llh_paramset)
    prm = ps.from_tag(ParamTag.SCALE)[0]
    if scale < prm.ranges[0]:
        prm.ranges = (scale, prm.ranges[1])
    prm.value = scale
    return ps


def _bsm_desc(args, asimov_paramset, llh_paramset, smearing):
    bf = fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    return compile_model(llh_paramset, "BSM_GAUSS", bestfit_fr=bf, smearing=smearing, source_ratio=args.source_ratio,
                         texture=args.texture, dimension=args.dimension, binning=args.binning)


def _opt(args, name, default):
    v = getattr(args, name, None)
    return default if v is None else v


def _scan_models(args, asimov_paramset, llh_paramset, scales, smearing, device, binned=None, table=None):
    """The per-scale set-up of sens.py's scans: the scanned columns are every column but the scale (sens.py:217-218), the scale
    column is fixed at each scale with its box lowered for the null point, one Model per scale.  Returns (cols, models, bases,
    labels); a model that cannot be built closes the ones before it.  `binned` (`llh.BinnedMeasurement`): attached to every scale's
    model, whose lnprob is then the energy-resolved likelihood.  `table` (`llh.TabulatedLikelihood`): likewise, the
    tabulated flavour-plane likelihood; not together with `binned`."""
    if binned is not None and table is not None:
        raise ValueError("binned and table are two likelihoods: give one")
    names = list(llh_paramset.names)
    scale_col = names.index(llh_paramset.from_tag(ParamTag.SCALE)[0].name)
    cols = [i for i in range(len(names)) if i != scale_col]
    smearing = float(smearing if smearing is not None else _opt(args, "smearing", 0.02))
    models, bases = [], []
    try:
        for sc in scales:
            ps = _scale_paramset(llh_paramset, float(sc))
            models.append(Model(_bsm_desc(args, asimov_paramset, ps, smearing), device=device))
            if binned is not None:
                models[-1].set_binned_measurement(binned)
            if table is not None:
                models[-1].set_table_likelihood(table)
            bases.append(np.array(ps.values, dtype=np.float64))
    except BaseException:
        for m in models:
            m.close()
        raise
    labels = ["scale {0:.6g} (Lambda^-1 = {1:.0E})".format(sc, np.power(10., sc)) for sc in scales]
    return cols, models, bases, labels


def evidence_scan(args, asimov_paramset, llh_paramset, scales, run_ids=None, nlive=None, tol=None, batch=None, walks=None,
                  seed=None, on_nonunitary="raise", smearing=None, device=0, max_iter=100000, return_sampler=False, posterior=None,
                  binned=None, table=None):
    """sens.py:231-303 for every scale at once: the scanned columns are every column but the scale (sens.py:217-218), the scale
    column is fixed at each scale (with its box lowered for the null point), one device call.  `args` as for bsm_ln_prob
    (source_ratio, dimension, texture, binning) plus the --mn-* options.  Returns dict(scales, lnz, lnz_err, max_lnl, niter,
    nevals, nonunitary, seconds).  posterior=dict(nrows=..., elements=False, and `NestedSampler.marginals`'s keyword arguments):
    the result also carries "posterior" (`NestedSampler.posterior()`), "marginals" ([scale] MarginalResult over llh_paramset's
    columns) and, with elements, "marginals_elements"; spectrum=[percentiles] adds "spectrum" ([scale] `spectrum.SpectrumResult`); all
    computed before the sampler is closed.  binned (`llh.BinnedMeasurement`): the evidence of the energy-resolved likelihood
     -- the measurement is attached to every scale's model.  table (`llh.TabulatedLikelihood`): the evidence of the
    tabulated flavour-plane likelihood, attached to every scale's model."""
    import time
    scales = np.asarray(scales, dtype=np.float64)
    cols, models, bases, labels = _scan_models(args, asimov_paramset, llh_paramset, scales, smearing, device, binned=binned, table=table)
    try:
        s = NestedSampler(models, cols, bases, nlive=int(nlive or _opt(args, "mn_live_points", DEFAULT_NLIVE)),
                          batch=batch if batch is not None else _opt(args, "mn_batch", None),
                          walks=int(walks or _opt(args, "mn_walks", DEFAULT_WALKS)),
                          seed=int(seed if seed is not None else _opt(args, "seed", 0)), on_nonunitary=on_nonunitary,
                          tol=float(tol or _opt(args, "mn_tolerance", DEFAULT_TOL)), run_ids=run_ids, labels=labels)
        t0 = time.perf_counter()
        try:
            res = s.run(max_iter=max_iter)
            res["seconds"] = time.perf_counter() - t0
            if posterior is not None:
                kw = dict(posterior)
                nrows, elements = int(kw.pop("nrows")), bool(kw.pop("elements", False))
                spectrum = kw.pop("spectrum", None)
                kw.setdefault("names", list(llh_paramset.names))
                kw.setdefault("ranges", [tuple(float(v) for v in p.ranges) for p in llh_paramset])
                post = dict(posterior=s.posterior(), marginals=s.marginals(nrows, **kw))
                if elements:
                    ekw = {k: v for k, v in kw.items() if k not in ("names", "ranges")}
                    post["marginals_elements"] = s.marginals(nrows, space="elements", llh_paramset=llh_paramset, **ekw)
                if spectrum is not None:
                    post["spectrum"] = s.spectrum(nrows, percentiles=spectrum)
                res.update(post)
        finally:
            if not return_sampler:
                s.close()
        res["scales"] = scales
        if return_sampler:
            res["sampler"] = s
            res["models"] = models
        return res
    finally:
        if not return_sampler:
            for m in models:
                m.close()


def mn_evidence(mn_paramset, llh_paramset, asimov_paramset, args, prefix=None):
    """golemflavor/mn.py:71-108, same name, arguments and return: (evidence, maxllh) = (ln Z, max ln L) of the nested run over
    mn_paramset's columns with every other column of llh_paramset at its value.  `prefix` (MultiNest's output basename) is
    accepted and unused: nothing is written."""
    for n in mn_paramset.names:
        llh_paramset[n].value = mn_paramset[n].value
    names = list(llh_paramset.names)
    cols = [names.index(n) for n in mn_paramset.names]
    smearing = float(_opt(args, "smearing", 0.02))
    with Model(_bsm_desc(args, asimov_paramset, llh_paramset, smearing), device=int(_opt(args, "device", 0))) as m:
        s = NestedSampler([m], cols, np.array(llh_paramset.values, dtype=np.float64),
                          nlive=int(_opt(args, "mn_live_points", DEFAULT_NLIVE)), batch=_opt(args, "mn_batch", None),
                          walks=int(_opt(args, "mn_walks", DEFAULT_WALKS)), seed=int(_opt(args, "seed", 0)),
                          tol=float(_opt(args, "mn_tolerance", DEFAULT_TOL)), labels=[prefix or "mn"])
        try:
            res = s.run()
        finally:
            s.close()
    return float(res["lnz"][0]), float(res["max_lnl"][0])
