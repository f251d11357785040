"""Posterior marginals of a chain on the device: the numbers behind the triangle plot the reference's scripts end in
(`plot.chainer_plot` -> `plot_Tchain`, golemflavor/plot.py:450-469) -- 1-D and 2-D histograms of every sampled parameter over its
range, credible regions of each of them, percentiles, mean and covariance -- without the chain crossing PCIe.

getdist, which draws the reference's plot, is not a dependency of this package, so there is no kernel density estimate to pin
against: THE DEFINITION IS THIS PACKAGE'S OWN.  It uses only arithmetic with an executable statement elsewhere:
  histograms   np.histogram(x, bins, range) / np.histogram2d(x_i, x_j) over `np.linspace(lo, hi, bins + 1)`, pairs i < j in
               lexicographic order; a value outside its range or NaN is dropped from that column's histogram and from every pair
               with that column;
  regions      `flavor_contour`'s reduction (plot.py:371-383: H / np.sum(H), gaussian_filter, descending argsort, cumsum,
               searchsorted) applied to each marginal instead of the flavor cube -- `contour.RegionResult`s;
  percentiles  np.percentile's default `linear` rule on two exact order statistics of the column's non-NaN values;
  moments      mean and covariance (ddof 1) over the rows without NaN, summed along a fixed tree (see `moment_tree_depth`).
The kernels are in csrc/gf_marginal.hip and csrc/gf_region.hip.
"""
import ctypes as C

import numpy as np

from . import _lib, contour
from ._lib import GF_MARGINAL_MAX_RANKS, check  # noqa: F401

DEFAULT_CAP_2D = 1024    # sorted cells per 2-D marginal fetched by the first call; a larger region costs a second call
LEAF_ROWS = 4096         # rows per leaf of the device's summation tree


def pair_list(width):
    """The pairs (i, j), i < j, in the order of `counts2`'s second axis."""
    return [(i, j) for i in range(width) for j in range(i + 1, width)]


def bin_edges(ranges, bins):
    """(width, bins + 1): np.linspace(lo, hi, bins + 1) per column, which is np.histogram_bin_edges(x, bins, (lo, hi))."""
    r = _ranges(ranges)
    return np.stack([np.linspace(lo, hi, int(bins) + 1) for lo, hi in r])


def _ranges(ranges):
    r = np.array(ranges, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != 2 or r.shape[0] < 1:
        raise ValueError("ranges must be (width, 2)")
    if not np.all(np.isfinite(r)) or not np.all(r[:, 0] < r[:, 1]):
        raise ValueError("every range must be finite with lo < hi")
    return r


def percentile_ranks(n, q):
    """The two ranks np.percentile(x, q) (method 'linear', numpy 2.x `_quantile`) reads from the sorted x of length n, and the
    weight between them: virtual index (n - 1) * (q / 100), its floor and the next one (both n - 1 at the top), gamma = the
    fractional part."""
    quantile = np.true_divide(np.float64(q), 100)
    vi = (n - 1) * quantile
    lo = np.floor(vi)
    gamma = np.float64(vi - lo)
    if vi >= n - 1:
        return n - 1, n - 1, gamma
    lo = int(lo)
    return lo, lo + 1, gamma


def lerp(a, b, t):
    """numpy's `_lerp`, both branches: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def percentile_from_order_statistics(n, q, x_lo, x_hi):
    """np.percentile(x, q) from x's order statistics at `percentile_ranks(n, q)`."""
    if n < 1:
        return np.float64(np.nan)
    return lerp(x_lo, x_hi, percentile_ranks(n, q)[2])


def moment_tree_depth(n):
    """Additions a term passes through, at most, in the device's sum of n rows: 16 (a lane's rows of a 4096-row leaf, in
    order) + 6 (shuffle levels) + 3 (the four waves), then ceil(leaves / 256) + 6 + 3 over the leaves."""
    leaves = max(1, -(-int(n) // LEAF_ROWS))
    return 16 + 6 + 3 + (-(-leaves // 256)) + 6 + 3


class MarginalResult:
    """One chain's marginals.

    names, ranges (width, 2), edges1 (width, bins_1d + 1), edges2 (width, bins_2d + 1), pairs [(i, j)];
    counts1 (width, bins_1d), counts2 (npairs, bins_2d, bins_2d) uint64;
    nvalid (rows without NaN), mean (width,), cov (width, width);
    ncol (width,) non-NaN values per column; order_ranks / order_stats (width, nslots): the exact order statistics fetched
    (first the caller's `ranks`, then two per percentile; -1 / NaN where the column has none);
    percentiles (width, len(q)) with `percentile_q` the q's;
    regions1 [column][coverage], regions2 [pair][coverage]: `contour.RegionResult` whose `cells` are (b,) or (b_i, b_j) rows."""

    ARRAYS = ("ranges", "edges1", "edges2", "pairs", "counts1", "counts2", "nvalid", "mean", "cov", "ncol", "order_ranks", "order_stats",
              "percentile_q", "percentiles", "coverage")
    REGION_ARRAYS = ("thres", "saturated", "level_in", "level_out", "mass")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def region_arrays(self):
        """The regions as flat arrays: r1_<field> (width, ncov), r2_<field> (npairs, ncov), r1_cells (width, bins_1d),
        r2_cells (npairs, max cells) flat indices padded with -1, r*_density alongside."""
        out = {}
        for tag, regs in (("r1", self.regions1), ("r2", self.regions2)):
            for f in self.REGION_ARRAYS:
                out["%s_%s" % (tag, f)] = np.array([[getattr(r, f) for r in row] for row in regs]).reshape(len(regs), len(self.coverage))
            longest = [max(row, key=lambda r: len(r.flat_cells)) if row else None for row in regs]
            width = max([len(r.flat_cells) for r in longest if r is not None], default=0)
            cells = np.full((len(regs), width), -1, dtype=np.int32)
            dens = np.zeros((len(regs), width))
            for k, r in enumerate(longest):
                if r is not None:
                    cells[k, :len(r.flat_cells)] = r.flat_cells
                    dens[k, :len(r.density)] = r.density
            out[tag + "_cells"], out[tag + "_density"] = cells, dens
        return out

    def as_arrays(self):
        """Everything as a dict of arrays: the layout of the `.npz` a scan writes."""
        out = {k: np.asarray(getattr(self, k)) for k in self.ARRAYS}
        out["names"] = np.array([str(n) for n in self.names])
        out.update(self.region_arrays())
        return out

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **self.as_arrays())

    def __repr__(self):
        return "MarginalResult(width=%d, nvalid=%d, bins=(%d, %d))" % (len(self.names), int(self.nvalid), self.counts1.shape[-1],
                                                                      self.counts2.shape[-1])


class _Region1(contour.RegionResult):
    """a region of a 1-D marginal: cells (thres, 1)"""

    def __init__(self, nbins, *a):
        super().__init__(nbins, *a)
        self.cells = self.flat_cells.reshape(-1, 1)


class _Region2(contour.RegionResult):
    """a region of a 2-D marginal: cells (thres, 2) = (b_i, b_j)"""

    def __init__(self, nbins, *a):
        super().__init__(nbins, *a)
        self.cells = np.stack([self.flat_cells // self.nbins, self.flat_cells % self.nbins], axis=1)


def prepare(width, ranges, names=None, bins_1d=100, bins_2d=50, coverage=(90., 99.), percentiles=(5., 50., 95.), ranks=(),
            hist_smooth=0.05, truncate=4.0):
    """Validate the arguments and build what every entry point shares: a dict with the edges, weights, coverages, ..."""
    r = _ranges(ranges)
    if r.shape[0] != width:
        raise ValueError("%d ranges for %d columns" % (r.shape[0], width))
    bins_1d, bins_2d = int(bins_1d), int(bins_2d)
    if not (1 <= bins_1d <= 1024 and 1 <= bins_2d <= 1024):
        raise ValueError("bins must lie in [1, 1024]")
    _, cov = contour._coverages(list(np.atleast_1d(coverage)))
    if not np.all((cov > 0) & (cov <= 100)):
        raise ValueError("coverages must lie in (0, 100]")
    q = np.atleast_1d(np.asarray(percentiles, dtype=np.float64)).copy()
    if q.ndim != 1 or not np.all((q >= 0) & (q <= 100)):
        raise ValueError("percentiles must lie in [0, 100]")
    rk = np.atleast_1d(np.asarray(ranks, dtype=np.int64)).copy() if len(np.atleast_1d(ranks)) else np.zeros(0, dtype=np.int64)
    if len(rk) + 2 * len(q) > GF_MARGINAL_MAX_RANKS:
        raise ValueError("ranks + 2 x percentiles must not exceed %d" % GF_MARGINAL_MAX_RANKS)
    names = ["x%d" % c for c in range(width)] if names is None else [str(n) for n in names]
    if len(names) != width:
        raise ValueError("%d names for %d columns" % (len(names), width))
    w = np.ascontiguousarray(contour.gaussian_weights(hist_smooth, truncate))
    return dict(width=width, names=names, ranges=r, bins_1d=bins_1d, bins_2d=bins_2d, edges1=np.ascontiguousarray(bin_edges(r, bins_1d)),
                edges2=np.ascontiguousarray(bin_edges(r, bins_2d)), coverage=cov, q=q, ranks=rk, weights=w, radius=(len(w) - 1) // 2)


def run_marginal_call(call, what, nchains, prep, cap_2d=None):
    """Drive one of the C entry points: `call(spec_pointer, out_pointer)`.  Returns [chain] MarginalResult."""
    W, nb1, nb2 = prep["width"], prep["bins_1d"], prep["bins_2d"]
    cov, q, rk = prep["coverage"], prep["q"], prep["ranks"]
    ncov, npairs, R = len(cov), W * (W - 1) // 2, len(rk) + 2 * len(q)
    fixed = cap_2d is not None
    cap2 = int(cap_2d) if fixed else min(DEFAULT_CAP_2D, nb2 * nb2)
    dp, ip, lp, up = _lib._dp, _lib._ip, _lib._lp, _lib._up
    while True:
        a = dict(counts1=np.zeros((nchains, W, nb1), np.uint64), counts2=np.zeros((nchains, npairs, nb2, nb2), np.uint64),
                 nvalid=np.zeros(nchains, np.int64), mean=np.full((nchains, W), np.nan), cov=np.full((nchains, W, W), np.nan),
                 ncol=np.zeros((nchains, W), np.int64), orank=np.full((nchains, W, R), -1, np.int64), ostat=np.full((nchains, W, R), np.nan))
        for tag, nm, cap in (("1", W, nb1), ("2", npairs, cap2)):
            a["thres" + tag] = np.zeros((nchains, nm, ncov), np.int64)
            a["saturated" + tag] = np.zeros((nchains, nm, ncov), np.int32)
            for f in ("level_in", "level_out", "mass"):
                a[f + tag] = np.full((nchains, nm, ncov), np.nan)
            a["cells" + tag] = np.full((nchains, nm, cap), -1, np.int32)
            a["density" + tag] = np.zeros((nchains, nm, cap))
        spec = _lib.GfMarginalSpec(nb1, nb2, prep["edges1"].ctypes.data_as(dp), prep["edges2"].ctypes.data_as(dp), prep["radius"], ncov,
                                   prep["weights"].ctypes.data_as(dp), cov.ctypes.data_as(dp), len(rk), len(q), rk.ctypes.data_as(lp),
                                   q.ctypes.data_as(dp), nb1, cap2)
        ptr = {np.dtype(np.uint64): up, np.dtype(np.int64): lp, np.dtype(np.int32): ip, np.dtype(np.float64): dp}
        out = _lib.GfMarginalOut(**{name: a[name].ctypes.data_as(ptr[a[name].dtype]) for name, _ in _lib.GfMarginalOut._fields_})
        check(call(C.byref(spec), C.byref(out)), what)
        need = int(np.where(a["saturated2"] != 0, 0, a["thres2"]).max(initial=0))
        if fixed or need <= cap2:
            break
        cap2 = need
    results = []
    pairs = pair_list(W)
    for ch in range(nchains):
        n = a["ncol"][ch]
        pct = np.full((W, len(q)), np.nan)
        for c in range(W):
            for k in range(len(q)):
                pct[c, k] = percentile_from_order_statistics(int(n[c]), q[k], a["ostat"][ch, c, len(rk) + 2 * k],
                                                             a["ostat"][ch, c, len(rk) + 2 * k + 1])
        regs = {}
        for tag, cls, nm, nb, cap in (("1", _Region1, W, nb1, nb1), ("2", _Region2, npairs, nb2, cap2)):
            rows = []
            for k in range(nm):
                row = []
                for j in range(ncov):
                    t = int(a["thres" + tag][ch, k, j])
                    take = min(t, cap)
                    row.append(cls(nb, cov[j], t, a["saturated" + tag][ch, k, j], a["level_in" + tag][ch, k, j], a["level_out" + tag][ch, k, j],
                                   a["mass" + tag][ch, k, j], a["cells" + tag][ch, k, :take].copy(), a["density" + tag][ch, k, :take].copy()))
                rows.append(row)
            regs[tag] = rows
        results.append(MarginalResult(
            names=prep["names"], ranges=prep["ranges"], edges1=prep["edges1"], edges2=prep["edges2"], pairs=np.array(pairs, np.int64).reshape(-1, 2),
            counts1=a["counts1"][ch], counts2=a["counts2"][ch], nvalid=int(a["nvalid"][ch]), mean=a["mean"][ch], cov=a["cov"][ch], ncol=n,
            order_ranks=a["orank"][ch], order_stats=a["ostat"][ch], percentile_q=q, percentiles=pct, coverage=cov, regions1=regs["1"],
            regions2=regs["2"]))
    return results


def chain_marginals(rows, ranges, *, model, names=None, bins_1d=100, bins_2d=50, coverage=(90., 99.), percentiles=(5., 50., 95.), ranks=(),
                    hist_smooth=0.05, truncate=4.0, cap_2d=None):
    """The marginals of host rows (n, width) -- or (nchains, n, width): a list, all chains in one set of launches.

    ranges: (width, 2) per-column (lo, hi); bins_1d / bins_2d, coverage, hist_smooth: plot_Tchain's settings
    (golemflavor/plot.py:456-459: 90 % and 99 % contours, 50 fine 2-D bins); percentiles: the q of np.percentile; ranks: extra
    exact order statistics (k >= 0 from the bottom, k < 0 from the top); model: any `Model` on the device to use."""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    single = x.ndim == 2
    if single:
        x = x[None]
    if x.ndim != 3 or x.shape[2] < 1:
        raise ValueError("rows must be (n, width) or (nchains, n, width)")
    nchains, n, W = x.shape
    prep = prepare(W, ranges, names, bins_1d, bins_2d, coverage, percentiles, ranks, hist_smooth, truncate)
    model = getattr(model, "model", model)
    if single:
        def call(spec, out):
            return model._L.gf_marginals(model._h, x.ctypes.data_as(_lib._dp), n, W, spec, out)
        return run_marginal_call(call, "gf_marginals", 1, prep, cap_2d)[0]
    d_rows = model.alloc(max(x.nbytes, 8))
    try:
        if x.nbytes:
            d_rows.upload(x)

        def call(spec, out):
            return model._L.gf_marginals_device(model._h, d_rows.ptr, nchains, n, W, spec, out)
        return run_marginal_call(call, "gf_marginals_device", nchains, prep, cap_2d)
    finally:
        d_rows.free()
