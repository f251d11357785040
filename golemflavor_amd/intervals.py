"""The reference's one 1-D credible interval on the device: "the *percentile* shortest interval around the mode"
(golemflavor/misc.py:174-213: `calc_nbins`, `calc_bins`, `most_likely`, `interval`) of every column of a chain -- the number
`plot.chainer_plot` prints on every diagonal panel and as the "Scale 90% Interval" (plot.py:503-519) -- and the number of distinct
values per column (`np.unique(samples[:, 0]).shape`, mcmc.py:47), without the chain crossing PCIe.

Per sorted column s of n finite values (csrc/gf_interval.hpp states every operation):
  nbins    floor((s[-1] - s[0]) / (2 * n**(-1/3) * (p75 - p25))), np.percentile's default rule;
  center   the centre of the first bin of maximal count of np.histogram(s, np.linspace(s[0], s[-1] + 2, nbins + 1));
  low, up  s[curr_low], s[curr_up] of the reference's walk from the first index nearest to center;
  nunique  the distinct values;
  status   per (column, percentile): 0 ok; 1 a NaN or an infinity in the column (this package's rule: NaN outputs, nbins and
           nunique -1); 2 nbins NaN, infinite or below 1 (the reference raises before the walk); 3 the walk would index s[n] (the
           reference raises IndexError); 4 nbins above 2**20 (unsupported).
`interval_host` and `most_likely_host` restate the definition in numpy and return the status instead of raising.  The kernels are
in csrc/gf_interval.hip.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GF_INTERVAL_MAX_BINS, GF_INTERVAL_MAX_PERCENTILES, check  # noqa: F401

ST_OK, ST_NONFINITE, ST_NBINS, ST_INDEX, ST_TOO_MANY_BINS = range(5)
FIELDS = ("low", "up", "status", "center", "nbins", "nunique")


def _percentiles(percentiles):
    p = np.atleast_1d(np.asarray(percentiles, dtype=np.float64)).copy()
    if p.ndim != 1 or not 1 <= len(p) <= GF_INTERVAL_MAX_PERCENTILES:
        raise ValueError("1 to %d percentiles" % GF_INTERVAL_MAX_PERCENTILES)
    if not np.all((p > 0) & (p <= 100)):
        raise ValueError("percentiles must lie in (0, 100]")
    return p


def run_interval_call(call, what, nchains, width, percentiles):
    """Drive one of the C entry points: `call(spec_pointer, out_pointer)`.  Returns a dict of FIELDS: low, up, status
    (nchains, width, npct), center, nbins, nunique (nchains, width), and `percentiles`."""
    p = _percentiles(percentiles)
    a = dict(low=np.full((nchains, width, len(p)), np.nan), up=np.full((nchains, width, len(p)), np.nan),
             status=np.full((nchains, width, len(p)), -1, np.int32), center=np.full((nchains, width), np.nan),
             nbins=np.full((nchains, width), -1, np.int64), nunique=np.full((nchains, width), -1, np.int64))
    spec = _lib.GfIntervalSpec(len(p), p.ctypes.data_as(_lib._dp))
    ptr = {np.dtype(np.int64): _lib._lp, np.dtype(np.int32): _lib._ip, np.dtype(np.float64): _lib._dp}
    out = _lib.GfIntervalOut(**{name: a[name].ctypes.data_as(ptr[a[name].dtype]) for name, _ in _lib.GfIntervalOut._fields_})
    check(call(C.byref(spec), C.byref(out)), what)
    a["percentiles"] = p
    return a


def chain_intervals(rows, *, model, percentiles=(68., 90.)):
    """The intervals of host rows (n, width) -- or (nchains, n, width), all chains in one call: a dict of low, up, status
    (width, npct), center, nbins, nunique (width,) [leading chain axis for stacked rows] and `percentiles`.
    model: any `Model` on the device to use."""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    single = x.ndim == 2
    if single:
        x = x[None]
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("rows must be (n, width) or (nchains, n, width), n >= 1")
    nchains, n, W = x.shape
    model = getattr(model, "model", model)
    if single:
        def call(spec, out):
            return model._L.gf_column_intervals(model._h, x.ctypes.data_as(_lib._dp), n, W, spec, out)
        res = run_interval_call(call, "gf_column_intervals", 1, W, percentiles)
        return {k: (v if k == "percentiles" else v[0]) for k, v in res.items()}
    d_rows = model.alloc(x.nbytes)
    try:
        d_rows.upload(x)

        def call(spec, out):
            return model._L.gf_column_intervals_device(model._h, d_rows.ptr, nchains, n, W, spec, out)
        return run_interval_call(call, "gf_column_intervals_device", nchains, W, percentiles)
    finally:
        d_rows.free()


def sort_columns(rows, *, model):
    """Every column of host rows (n, width) or (nchains, n, width) sorted on the device: (width, n) or (nchains, width, n),
    ascending, -0.0 before +0.0, NaN last."""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    single = x.ndim == 2
    if single:
        x = x[None]
    if x.ndim != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("rows must be (n, width) or (nchains, n, width), n >= 1")
    nchains, n, W = x.shape
    model = getattr(model, "model", model)
    out = np.empty((nchains, W, n))
    d_rows, d_sorted = model.alloc(x.nbytes), model.alloc(x.nbytes)
    try:
        d_rows.upload(x)
        check(model._L.gf_sort_columns_device(model._h, d_rows.ptr, nchains, n, W, d_sorted.ptr), "gf_sort_columns_device")
        d_sorted.download(out.shape, out=out)
    finally:
        d_rows.free()
        d_sorted.free()
    return out[0] if single else out


# ---- the definition in numpy ------------------------------------------------------------------------------------------------------

def _nbins(s):
    """calc_nbins of the sorted column: np.float64, possibly NaN, infinite or below 1"""
    n = len(s)
    with np.errstate(all="ignore"):
        p25, p75 = np.percentile(s, 25), np.percentile(s, 75)
        return np.floor((s[-1] - s[0]) / (2 * n ** (-1. / 3) * (p75 - p25)))


def _nbins_reported(nb):
    """the int64 the device reports for calc_nbins' value: -1 for NaN, the largest int64 for what does not fit"""
    return -1 if np.isnan(nb) else np.iinfo(np.int64).max if nb >= 9.2e18 else int(nb)


def most_likely_host(arr):
    """(center, nbins, status): the centre of the densest bin as `misc.most_likely` forms it; center is NaN unless status is 0.
    nbins is the integer reported by the device: -1 where the value is NaN."""
    s = np.sort(np.asarray(arr, dtype=np.float64).ravel())
    if len(s) < 1:
        raise ValueError("an empty column")
    if not np.all(np.isfinite(s)):
        return np.float64(np.nan), -1, ST_NONFINITE
    nb = _nbins(s)
    if not nb >= 1 or np.isinf(nb):
        return np.float64(np.nan), _nbins_reported(nb), ST_NBINS
    if nb > GF_INTERVAL_MAX_BINS:
        return np.float64(np.nan), _nbins_reported(nb), ST_TOO_MANY_BINS
    nb = int(nb)
    with np.errstate(all="ignore"):
        edges = np.linspace(s[0], s[-1] + 2, nb + 1)
        pos = np.concatenate([np.searchsorted(s, edges[:-1], "left"), np.searchsorted(s, edges[-1:], "right")])
        b = int(np.argmax(np.diff(pos)))
        return (edges[b] + edges[b + 1]) * 0.5, nb, ST_OK


def interval_host(arr, percentile=68.):
    """(low, center, up, status) of `misc.interval(arr, percentile)`: low and up are NaN unless status is 0, center is given for
    status 0 and 3."""
    s = np.sort(np.asarray(arr, dtype=np.float64).ravel())
    center, _, status = most_likely_host(s)
    nan = np.float64(np.nan)
    if status != ST_OK:
        return nan, center, nan, status
    n = len(s)
    with np.errstate(all="ignore"):
        low = up = int(np.argmin(np.abs(s - center)))
    v = s.tolist()                                                   # Python floats: the same IEEE doubles, a faster loop
    thr = float(percentile) / 100. * n
    while up - low < thr:
        if low == 0:
            if up == n - 1:
                return nan, center, nan, ST_INDEX
            up += 1
        elif up == n - 1:
            low -= 1
        else:
            a, b = v[up] - v[low - 1], v[up + 1] - v[low]
            if a < b or (a == b and (up - low) % 2):
                low -= 1
            else:
                up += 1
    return s[low], center, s[up], ST_OK


def nunique_host(arr):
    s = np.sort(np.asarray(arr, dtype=np.float64).ravel())
    return -1 if not np.all(np.isfinite(s)) else 1 + int(np.count_nonzero(s[1:] != s[:-1]))


def rows_intervals_host(rows, percentiles=(68., 90.)):
    """`chain_intervals`' dict for host rows (n, width), computed by the numpy restatement column by column."""
    x = np.asarray(rows, dtype=np.float64)
    p = _percentiles(percentiles)
    W = x.shape[1]
    a = dict(low=np.full((W, len(p)), np.nan), up=np.full((W, len(p)), np.nan), status=np.zeros((W, len(p)), np.int32),
             center=np.full(W, np.nan), nbins=np.full(W, -1, np.int64), nunique=np.full(W, -1, np.int64), percentiles=p)
    for c in range(W):
        col = x[:, c]
        _, a["nbins"][c], _ = most_likely_host(col)
        a["nunique"][c] = nunique_host(col)
        for k, q in enumerate(p):
            a["low"][c, k], a["center"][c], a["up"][c, k], a["status"][c, k] = interval_host(col, q)
    return a


def save(path, res, names=None):
    """One result dict as the `.npz` a scan writes."""
    out = {k: np.asarray(v) for k, v in res.items()}
    if names is not None:
        out["names"] = np.array([str(n) for n in names])
    with open(path, "wb") as f:
        np.savez(f, **out)
