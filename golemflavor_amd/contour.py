"""Credible regions of the flavor triangle on the device: what `plot.flavor_contour` (golemflavor/plot.py:359-392) computes
before it turns to geometry -- histogram, `H / np.sum(H)`, `scipy.ndimage.gaussian_filter`, then the cells in descending order
of density until the running sum reaches the coverage.  The kernels are in csrc/gf_region.hip; this module computes the
smoothing weights (scipy's own expression, on the host), marshals the arrays and unravels the cell indices.

The hull / alpha shape / spline part of `flavor_contour` (plot.py:393-448) is host geometry on the few thousand cells returned
here and is not part of this package.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GF_REGION_MAX_COVERAGES, GF_REGION_MAX_RADIUS, check  # noqa: F401

DEFAULT_CAP = 16384     # cells per (chain, coverage) fetched by the first call; a larger region costs a second call


def gaussian_radius(sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d's radius: int(truncate * sigma + 0.5)."""
    return int(truncate * float(sigma) + 0.5)


def gaussian_weights(sigma, truncate=4.0):
    """The 2 r + 1 weights scipy.ndimage.gaussian_filter correlates with (order 0), by scipy's expression, bit for bit."""
    sigma = float(sigma)
    radius = gaussian_radius(sigma, truncate)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


class RegionResult:
    """One chain's credible region at one coverage.

    thres: cells inside (np.searchsorted of the running sum: the cell that crosses the coverage is outside);
    saturated: the running sum never reaches coverage / 100 -- the reference's mask is then the whole cube; `thres` counts the
    cells with non-zero density and `cells` lists (at most the fetched capacity of) them;
    level_in / level_out: density of the last cell inside / first cell outside (NaN where there is none);
    mass: the running sum at the last cell inside;
    cells: (thres, 3) int array of (i, j, k) in descending order of density (equal densities: descending flat index);
    density: (thres,) the smoothed, normalised histogram at those cells.
    `cells` / `density` are shorter than thres only when the caller limited `cap` (or the region is saturated)."""

    def __init__(self, nbins, coverage, thres, saturated, level_in, level_out, mass, flat_cells, density):
        self.nbins, self.coverage = int(nbins), float(coverage)
        self.thres, self.saturated = int(thres), bool(saturated)
        self.level_in, self.level_out, self.mass = float(level_in), float(level_out), float(mass)
        self.flat_cells = np.asarray(flat_cells, dtype=np.int64)
        self.cells = unravel_cells(self.flat_cells, self.nbins)
        self.density = np.asarray(density, dtype=np.float64)

    def as_dict(self):
        """{(i, j, k): H_s[i, j, k]} of the cells inside: the `interp_dict` of plot.py:387-392."""
        return {(int(i), int(j), int(k)): float(d) for (i, j, k), d in zip(self.cells, self.density)}

    def __repr__(self):
        return "RegionResult(coverage=%g, nbins=%d, thres=%d, mass=%.6g, saturated=%s)" % (
            self.coverage, self.nbins, self.thres, self.mass, self.saturated)


def unravel_cells(flat, nbins):
    """flat index (i * nbins + j) * nbins + k -> (n, 3) array of (i, j, k)."""
    flat = np.asarray(flat, dtype=np.int64).reshape(-1)
    nb = int(nbins)
    return np.stack([flat // (nb * nb), (flat // nb) % nb, flat % nb], axis=1)


def _coverages(coverage):
    scalar = np.ndim(coverage) == 0
    cov = np.atleast_1d(np.asarray(coverage, dtype=np.float64)).copy()
    if cov.ndim != 1 or not 1 <= len(cov) <= GF_REGION_MAX_COVERAGES:
        raise ValueError("between 1 and %d coverages per call" % GF_REGION_MAX_COVERAGES)
    return scalar, cov


def run_region_call(call, what, nchains, nbins, coverage, hist_smooth, truncate=4.0, cap=None):
    """Drive one of the C entry points: `call(radius, weights, coverage, ncov, cap, thres, saturated, level_in, level_out, mass,
    cells, density)` with ctypes arguments.  cap None: DEFAULT_CAP first, and once more with the largest region's size if that did
    not hold every (non-saturated) region.  Returns [chain][coverage] RegionResult."""
    _, cov = _coverages(coverage)
    ncov = len(cov)
    w = np.ascontiguousarray(gaussian_weights(hist_smooth, truncate))
    radius = (len(w) - 1) // 2
    fixed = cap is not None
    cap = int(cap) if fixed else min(DEFAULT_CAP, int(nbins) ** 3)
    dp, ip, lp = _lib._dp, _lib._ip, C.POINTER(C.c_int64)
    while True:
        thres = np.zeros((nchains, ncov), dtype=np.int64)
        sat = np.zeros((nchains, ncov), dtype=np.int32)
        lin, lout, mass = (np.full((nchains, ncov), np.nan) for _ in range(3))
        cells = np.empty((nchains, ncov, max(cap, 0)), dtype=np.int32)
        dens = np.empty((nchains, ncov, max(cap, 0)), dtype=np.float64)
        check(call(radius, w.ctypes.data_as(dp), cov.ctypes.data_as(dp), ncov, cap, thres.ctypes.data_as(lp), sat.ctypes.data_as(ip),
                   lin.ctypes.data_as(dp), lout.ctypes.data_as(dp), mass.ctypes.data_as(dp), cells.ctypes.data_as(ip),
                   dens.ctypes.data_as(dp)), what)
        need = int(np.where(sat != 0, 0, thres).max(initial=0))
        if fixed or need <= cap:
            break
        cap = need
    out = []
    for ch in range(nchains):
        row = []
        for q in range(ncov):
            n = min(int(thres[ch, q]), cap)
            row.append(RegionResult(nbins, cov[q], thres[ch, q], sat[ch, q], lin[ch, q], lout[ch, q], mass[ch, q],
                                    cells[ch, q, :n].copy(), dens[ch, q, :n].copy()))
        out.append(row)
    return out


def shape_results(res, scalar_coverage, single_chain):
    """[chain][coverage] -> drop the axes the caller did not ask for."""
    if scalar_coverage:
        res = [row[0] for row in res]
    return res[0] if single_chain else res


def credible_region(counts, coverage, hist_smooth=0.05, *, model, truncate=4.0, cap=None, want_smoothed=False):
    """The credible region(s) of a flavor histogram `counts` (nbins, nbins, nbins) -- or (nchains, nbins, nbins, nbins), all
    chains in one set of launches -- as `Model.flavor_histogram` / `DeviceEnsembleSampler.postprocess` return it.

    coverage: percent, a number (-> RegionResult) or up to 8 of them (-> list); hist_smooth: the sigma of
    `scipy.ndimage.gaussian_filter` in bins (below 0.125 nothing is smoothed, as in scipy); model: any `Model` on the device to
    use.  want_smoothed: also return the smoothed, normalised histogram H_s, same shape as counts.  A leading chain axis in
    `counts` gives a leading list level in the result."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    single = c.ndim == 3
    if single:
        c = c[None]
    if c.ndim != 4 or not (c.shape[1] == c.shape[2] == c.shape[3]):
        raise ValueError("counts must be (nbins, nbins, nbins) or (nchains, nbins, nbins, nbins)")
    nchains, nb = c.shape[0], c.shape[1]
    scalar, _ = _coverages(coverage)
    model = getattr(model, "model", model)
    d_counts = model.alloc(c.nbytes).upload(c)
    d_smooth = model.alloc(c.size * 8) if want_smoothed else None
    try:
        def call(*args):
            return model._L.gf_flavor_region_device(model._h, d_counts.ptr, nchains, nb, *args, d_smooth.ptr if d_smooth else None)
        res = shape_results(run_region_call(call, "gf_flavor_region_device", nchains, nb, coverage, hist_smooth, truncate, cap),
                            scalar, single)
        if want_smoothed:
            hs = d_smooth.download(c.shape)
            return res, (hs[0] if single else hs)
        return res
    finally:
        d_counts.free()
        if d_smooth is not None:
            d_smooth.free()


def flavor_region(frs, nbins, coverage, hist_smooth=0.05, oversample=1., *, model, truncate=4.0, cap=None):
    """`flavor_contour`'s arguments (plot.py:359-361) up to the region: frs (n, 3) compositions are binned into
    int(nbins * oversample) + 1 bins per axis (plot.py:365-369), normalised, smoothed and selected on the device."""
    f = np.ascontiguousarray(frs, dtype=np.float64).reshape(-1, 3)
    nb = int(nbins * oversample) + 1
    scalar, _ = _coverages(coverage)
    model = getattr(model, "model", model)

    def call(*args):
        return model._L.gf_flavor_region(model._h, f.ctypes.data_as(_lib._dp), f.shape[0], nb, *args, None)
    return shape_results(run_region_call(call, "gf_flavor_region", 1, nb, coverage, hist_smooth, truncate, cap), scalar, True)
