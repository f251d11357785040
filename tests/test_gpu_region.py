"""GPU: the credible regions of the flavor triangle (csrc/gf_region.hip, golemflavor_amd.contour) against numpy + scipy executing
what plot.flavor_contour calls between its histogram and its geometry (golemflavor/plot.py:365-383).

`reference_region` below is that restatement: np.histogramdd, H / np.sum(H), scipy.ndimage.gaussian_filter, np.argsort()[::-1],
np.cumsum, np.searchsorted.  What is compared how:

  * unsmoothed (radius 0, the reference's default hist_smooth=0.05): thres, level_in, level_out and mass EXACTLY -- the running sum
    is the same sequence of fp64 additions of the same numbers; every cell denser than level_in is inside, none less dense is, the
    density of every returned cell is H_s there, and as many cells AT level_in are inside as in the reference.  Which of several
    equal cells at the cut are inside is not compared: np.argsort leaves the order of equal values unspecified.  The package's own
    rule (descending flat index) is asserted on a hand-made histogram.
  * smoothed: H_s within 3 (2 r + 3) 2^-52 relative of scipy's on every non-zero cell (each pass sums 2 r + 1 non-negative products,
    so any summation order is within (2 r + 2) u of the exact pass, u = 2^-53, and so is scipy; three passes compound) and exactly
    zero where scipy's is zero; thres equal whenever the reference's own margin to the coverage exceeds nb^3 2^-52, the most that
    tolerance can move a running sum that never exceeds 1.

Unsmoothed cases: the cells AT level_in must be at most 10 % of thres (asserted from the reference alone), so that the exemption of
equal cells cannot hide a failure.  Measured on the reference before writing the list: of the 18 combinations of {flat, peak} x
{26, 126, 201} x {68, 90, 99} two exceed it -- flat, nb = 126, coverage 68 (1037 of 9826 cells, 10.6 %) and flat, nb = 201,
coverage 68 (4163 of 23420, 17.8 %): 600 000 samples over 16 000 / 40 000 occupied cells leave many cells with equal counts --
and are left out of UNSMOOTHED_CASES; the largest fraction kept is 8.4 % (flat, 201, 90).
Smoothed cases below the margin (measured the same way): flat, sigma = 0.125, coverage 90 at nb = 126 and 201 (the reference's
running sum passes within 1e-12 of 0.9), 2 of 72.
"""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from golemflavor_amd import _lib, contour
from golemflavor_amd import configs as Cf
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

COVERAGES = (68., 90., 99.)
NBINS = (26, 126, 201)
SIGMAS = (0.125, 0.6, 1.5, 3.0)          # radius 1, 2, 6, 12
NSAMPLES = 600000
EXCLUDED_UNSMOOTHED = {("flat", 126, 68.), ("flat", 201, 68.)}       # more than 10 % of the region at the cut level: see above
UNSMOOTHED_CASES = [(name, nb, c) for name in ("flat", "peak") for nb in NBINS for c in COVERAGES
                    if (name, nb, c) not in EXCLUDED_UNSMOOTHED]


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


_inputs = {}


def compositions(name):
    if name not in _inputs:
        _inputs[name] = {"flat": lambda: np.random.default_rng(1).dirichlet((1, 1, 1), NSAMPLES),
                         "peak": lambda: np.random.default_rng(2).dirichlet((60, 20, 25), NSAMPLES)}[name]()
    return _inputs[name]


def reference_region(frs, nb, coverage, sigma):
    """plot.py:365-383 in numpy / scipy.  Returns H_s, the descending order, its running sum and thres per coverage."""
    frs = np.asarray(frs, dtype=np.float64).reshape(-1, 3)
    H, _ = np.histogramdd((frs[:, 0], frs[:, 1], frs[:, 2]), bins=(nb, nb, nb), range=((0, 1), (0, 1), (0, 1)))
    counts = H.astype(np.uint64)
    H = H / np.sum(H)
    H_s = gaussian_filter(H, sigma=sigma)
    H_r = np.ravel(H_s)
    H_rs = np.argsort(H_r)[::-1]
    H_crs = np.cumsum(H_r[H_rs])
    thres = [int(np.searchsorted(H_crs, c / 100.)) for c in np.atleast_1d(coverage)]
    return counts, H_s, H_rs, H_crs, thres


def check_sorted(r):
    """the package's order: descending density, equal densities by descending flat index"""
    d, f = r.density, r.flat_cells
    assert np.all(d[:-1] >= d[1:])
    same = d[:-1] == d[1:]
    assert np.all(f[:-1][same] > f[1:][same])
    assert len(np.unique(f)) == len(f)


def check_exact_region(r, H_s, H_rs, H_crs, thres, what):
    """everything the reference defines, exactly (module docstring); returns the fraction of the region at the cut level"""
    H_r = H_s.ravel()
    n = len(H_r)
    if thres == n:                                   # the running sum never reaches the coverage: the whole cube
        nnz = int(np.count_nonzero(H_r))
        assert r.saturated and r.thres == nnz, what
        assert r.mass == H_crs[-1] and np.isnan(r.level_out), what
        return 0.0
    print("%s: thres %d (reference %d) level_in %r (%r) level_out %r (%r) mass %r (%r)" % (
        what, r.thres, thres, r.level_in, H_r[H_rs[thres - 1]] if thres else None, r.level_out, H_r[H_rs[thres]], r.mass,
        H_crs[thres - 1] if thres else 0.0))
    assert not r.saturated and r.thres == thres, what
    assert r.level_out == H_r[H_rs[thres]], what
    if thres == 0:
        assert np.isnan(r.level_in) and r.mass == 0.0 and len(r.flat_cells) == 0, what
        return 0.0
    lin = H_r[H_rs[thres - 1]]
    assert r.level_in == lin and r.mass == H_crs[thres - 1], what
    assert len(r.flat_cells) == thres and r.cells.shape == (thres, 3), what
    check_sorted(r)
    inside = np.zeros(n, dtype=bool)
    inside[r.flat_cells] = True
    assert np.all(inside[H_r > lin]) and not np.any(inside[H_r < lin]), what
    assert np.array_equal(r.density, H_r[r.flat_cells]), what
    at_level_ref = int(np.count_nonzero(H_r[H_rs[:thres]] == lin))
    assert int(np.count_nonzero(r.density == lin)) == at_level_ref, what
    assert np.array_equal(r.cells, np.stack(np.unravel_index(r.flat_cells, H_s.shape), axis=1)), what
    return at_level_ref / thres


def same_region(a, b):
    """two results identical in every field, cell order included"""
    return ((a.thres, a.saturated) == (b.thres, b.saturated) and
            np.array_equal([a.level_in, a.level_out, a.mass], [b.level_in, b.level_out, b.mass], equal_nan=True) and
            np.array_equal(a.flat_cells, b.flat_cells) and np.array_equal(a.density, b.density))


# ---- unsmoothed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb", [(name, nb) for name in ("flat", "peak") for nb in NBINS])
def test_unsmoothed_region_equals_the_reference_exactly(model, name, nb):
    frs = compositions(name)
    covs = [c for c in COVERAGES if (name, nb, c) in UNSMOOTHED_CASES]
    assert covs
    counts, H_s, H_rs, H_crs, thres = reference_region(frs, nb, covs, 0.05)
    # from compositions (histogram on the device), from counts, and through Model.flavor_region's reference arguments
    res = contour.flavor_region(frs, nb - 1, covs, hist_smooth=0.05, oversample=1., model=model)
    res2, hs = contour.credible_region(counts, covs, 0.05, model=model, want_smoothed=True)
    assert np.array_equal(hs, H_s)                                   # radius 0: H_s is H, one division per cell
    for q, c in enumerate(covs):
        what = "%s nb=%d coverage=%g" % (name, nb, c)
        # the condition on the input, from the reference alone
        lin = H_s.ravel()[H_rs[thres[q] - 1]]
        frac = np.count_nonzero(H_s == lin) / thres[q]
        print("%s: cells at level_in / thres = %.4f" % (what, frac))
        assert frac <= 0.10, what
        check_exact_region(res[q], H_s, H_rs, H_crs, thres[q], what)
        check_exact_region(res2[q], H_s, H_rs, H_crs, thres[q], what + " (from counts)")
        assert np.array_equal(res[q].flat_cells, res2[q].flat_cells)
        assert res[q].as_dict() == {tuple(int(x) for x in ijk): H_s[tuple(ijk)] for ijk in res[q].cells}
    one = model.flavor_region(frs, nb - 1, covs[-1])                 # a single coverage: one RegionResult, default arguments
    assert one.thres == thres[-1] and np.array_equal(one.flat_cells, res[-1].flat_cells)


# ---- smoothed ------------------------------------------------------------------------------------------------------------------
def test_smoothed_volume_and_region_against_scipy(model):
    cases = skipped = 0
    for name in ("flat", "peak"):
        frs = compositions(name)
        for nb in NBINS:
            for sigma in SIGMAS:
                r = contour.gaussian_radius(sigma)
                tol = 3 * (2 * r + 3) * 2.0 ** -52
                counts, H_s, H_rs, H_crs, thres = reference_region(frs, nb, COVERAGES, sigma)
                res, hs = contour.credible_region(counts, COVERAGES, sigma, model=model, want_smoothed=True)
                nz = H_s != 0
                rel = np.abs(hs[nz] - H_s[nz]) / H_s[nz]
                print("%s nb=%d sigma=%g radius=%d: H_s bit-equal %s, max rel err %.3e (tolerance %.3e)" % (
                    name, nb, sigma, r, np.array_equal(hs, H_s), rel.max(), tol))
                assert rel.max() <= tol, (name, nb, sigma)
                assert np.all(hs[~nz] == 0), (name, nb, sigma)
                H_r, n = H_s.ravel(), H_s.size
                for q, c in enumerate(COVERAGES):
                    cases += 1
                    t = thres[q]
                    assert 0 < t < n
                    margin = min(c / 100. - H_crs[t - 1], H_crs[t] - c / 100.)
                    if not margin > n * 2.0 ** -52:
                        skipped += 1
                        print("  coverage %g: reference margin %.3e below %.3e, thres not compared" % (c, margin, n * 2.0 ** -52))
                        continue
                    got = res[q]
                    print("  coverage %g: thres %d (reference %d)" % (c, got.thres, t))
                    assert got.thres == t and not got.saturated, (name, nb, sigma, c)
                    check_sorted(got)
                    assert np.array_equal(got.density, hs.ravel()[got.flat_cells])
                    lin, lout = H_r[H_rs[t - 1]], H_r[H_rs[t]]
                    assert abs(got.level_in - lin) <= tol * lin and abs(got.level_out - lout) <= tol * lout
                    assert abs(got.mass - H_crs[t - 1]) <= n * 2.0 ** -52
                    clear = (np.abs(H_r - lin) > tol * lin) & (np.abs(H_r - lout) > tol * lout)
                    ref_in = np.zeros(n, dtype=bool)
                    ref_in[H_rs[:t]] = True
                    ours = np.zeros(n, dtype=bool)
                    ours[got.flat_cells] = True
                    assert np.array_equal(ours[clear], ref_in[clear]), (name, nb, sigma, c)
    print("smoothed: %d of %d cases below the reference's margin" % (skipped, cases))
    assert cases == 2 * len(NBINS) * len(SIGMAS) * len(COVERAGES) and skipped * 10 <= cases


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def raw_call(model, counts, coverage, radius=0, weights=None, cap=0, nbins=None, ncov=None, want_cells=True):
    """gf_flavor_region_device itself; returns (code, thres, saturated, level_in, level_out, mass, cells, density)"""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    nch = 1 if c.ndim == 3 else c.shape[0]
    nb = c.shape[-1] if nbins is None else nbins
    cov = np.ascontiguousarray(coverage, dtype=np.float64)
    ncov = len(cov) if ncov is None else ncov
    n = max(len(cov), 1)
    d = model.alloc(max(c.nbytes, 8)).upload(c)
    thres = np.full((nch, n), -7, dtype=np.int64)
    sat = np.full((nch, n), -7, dtype=np.int32)
    lin, lout, mass = (np.full((nch, n), -7.0) for _ in range(3))
    cells_c = np.full((nch, n, max(cap, 0)), -7, dtype=np.int32)         # -7: what the call did not write
    dens_c = np.full((nch, n, max(cap, 0)), -7.0)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    lp = C.POINTER(C.c_int64)
    code = model._L.gf_flavor_region_device(
        model._h, d.ptr, nch, nb, radius, None if w is None else w.ctypes.data_as(_lib._dp), cov.ctypes.data_as(_lib._dp), ncov, cap,
        thres.ctypes.data_as(lp), sat.ctypes.data_as(_lib._ip), lin.ctypes.data_as(_lib._dp), lout.ctypes.data_as(_lib._dp),
        mass.ctypes.data_as(_lib._dp), cells_c.ctypes.data_as(_lib._ip) if want_cells else None,
        dens_c.ctypes.data_as(_lib._dp) if want_cells else None, None)
    d.free()
    return code, thres, sat, lin, lout, mass, cells_c, dens_c


def test_all_mass_in_one_cell(model):
    """The cell that crosses the coverage is outside, so one cell holding everything is an empty region at every coverage --
    at 100 too: its running sum 1.0 is not < 100 / 100., np.searchsorted(side='left') answers 0 there as well, and the sum HAS
    reached the coverage, so this is not the saturated case (test_saturated_when_the_sum_stays_below_the_coverage is)."""
    counts = np.zeros((5, 5, 5), dtype=np.uint64)
    counts[1, 2, 3] = 1000
    res = contour.credible_region(counts, [50., 99., 100.], model=model)
    for r in res:                                     # the cell that crosses the coverage is outside: the region is empty
        assert r.thres == 0 and not r.saturated and np.isnan(r.level_in) and r.level_out == 1.0 and r.mass == 0.0
        assert r.cells.shape == (0, 3) and r.as_dict() == {}
    # the running sum 1.0 reaches 100 / 100. exactly, as np.searchsorted(side='left') sees it: not saturated either
    _, H_s, H_rs, H_crs, thres = reference_region(np.tile([[0.3, 0.5, 0.7]], (1000, 1)), 5, [50., 99., 100.], 0.05)
    assert thres == [0, 0, 0] and H_s[1, 2, 3] == 1.0
    # two cells, 0.9 and 0.1
    counts[:] = 0
    counts[0, 0, 0], counts[4, 4, 4] = 1, 9
    r95, r100 = contour.credible_region(counts, [95., 100.], model=model)
    H = counts / counts.sum()
    crs = np.cumsum(np.sort(H.ravel())[::-1])
    t100 = int(np.searchsorted(crs, 1.0))
    assert r95.thres == 1 and r95.level_in == 0.9 and r95.level_out == 0.1 and r95.mass == 0.9
    assert np.array_equal(r95.cells, [[4, 4, 4]])
    if t100 == H.size:                                # never reached: saturated, thres = the non-zero cells
        assert r100.saturated and r100.thres == 2 and np.isnan(r100.level_out) and r100.mass == crs[1]
    else:
        assert not r100.saturated and r100.thres == t100


def test_saturated_when_the_sum_stays_below_the_coverage(model):
    """ten cells of 1/10: the fp64 running sum ends at 0.9999999999999999 < 100 / 100."""
    counts = np.zeros((4, 4, 4), dtype=np.uint64)
    counts.ravel()[3:13] = 7
    crs = np.cumsum(np.full(10, 0.1))
    assert crs[-1] < 1.0
    r = contour.credible_region(counts, 100., model=model)
    assert r.saturated and r.thres == 10 and r.mass == crs[-1] and r.level_in == 0.1 and np.isnan(r.level_out)
    assert np.array_equal(r.flat_cells, np.arange(12, 2, -1))
    H_r = (counts / np.sum(counts)).ravel()
    assert int(np.searchsorted(np.cumsum(H_r[np.argsort(H_r)[::-1]]), 100. / 100.)) == 64          # the reference: the whole cube


def test_equal_cells_are_ordered_by_descending_flat_index(model):
    nb = 6
    counts = np.zeros((nb, nb, nb), dtype=np.uint64)
    flat = counts.reshape(-1)
    flat[[5, 17, 100, 215]] = 10                     # four equal cells
    flat[[3, 50]] = 30                               # two equal, denser
    flat[7] = 1
    res = contour.credible_region(counts, [20., 50., 70., 90., 99.9], model=model)
    order = [50, 3, 215, 100, 17, 5, 7]
    crs = np.cumsum(flat[order] / flat.sum())
    for r, c in zip(res, [20., 50., 70., 90., 99.9]):
        t = int(np.searchsorted(crs, c / 100.))
        assert r.thres == t and np.array_equal(r.flat_cells, order[:t]), c
        assert r.mass == (crs[t - 1] if t else 0.0)
    # two equal cells and nothing else: the higher flat index first
    counts[:] = 0
    flat[[40, 41]] = 5
    r = contour.credible_region(counts, 60., model=model)
    assert r.thres == 1 and np.array_equal(r.flat_cells, [41]) and r.level_in == 0.5 and r.level_out == 0.5 and r.mass == 0.5


def test_empty_histogram_has_no_region(model):
    res = contour.credible_region(np.zeros((2, 9, 9, 9), dtype=np.uint64), [90., 100.], model=model)
    for row in res:
        for r in row:
            assert r.thres == 0 and not r.saturated and r.mass == 0.0 and np.isnan(r.level_in) and np.isnan(r.level_out)
            assert r.cells.shape == (0, 3)
    res, hs = contour.credible_region(np.zeros((3, 3, 3), dtype=np.uint64), 90., 0.6, model=model, want_smoothed=True)
    assert res.thres == 0 and np.all(hs == 0)        # zeros, not numpy's NaN
    # an empty chain beside a filled one
    counts = np.zeros((2, 4, 4, 4), dtype=np.uint64)
    counts[1, 0, 0, :] = [4, 3, 2, 1]
    res = contour.credible_region(counts, 65., model=model)
    assert res[0].thres == 0 and res[1].thres == 1 and np.array_equal(res[1].cells, [[0, 0, 0]])


def test_cap_smaller_than_the_region(model):
    counts = np.zeros((2, 8, 8, 8), dtype=np.uint64)
    rng = np.random.default_rng(5)
    counts.reshape(2, -1)[:, :300] = rng.permutation(600).reshape(2, 300) + 1       # all distinct
    full = contour.credible_region(counts, [50., 90.], model=model)
    cap = 20
    code, thres, sat, lin, lout, mass, cells, dens = raw_call(model, counts, [50., 90.], cap=cap)
    assert code == _lib.GF_OK
    for ch in range(2):
        for q in range(2):
            f = full[ch][q]
            assert f.thres > cap and thres[ch, q] == f.thres and lin[ch, q] == f.level_in and mass[ch, q] == f.mass
            assert np.array_equal(cells[ch, q], f.flat_cells[:cap]) and np.array_equal(dens[ch, q], f.density[:cap])
    # a cap between the two regions' sizes: the smaller one complete, nothing written behind it
    t0 = full[0][0].thres
    code, thres, sat, lin, lout, mass, cells, dens = raw_call(model, counts, [50., 90.], cap=t0 + 5)
    assert code == _lib.GF_OK
    assert np.array_equal(cells[0, 0, :t0], full[0][0].flat_cells) and np.all(cells[0, 0, t0:] == -7) and np.all(dens[0, 0, t0:] == -7.0)
    assert np.array_equal(cells[0, 1], full[0][1].flat_cells[:t0 + 5])
    # cap 0 and no arrays: the counts alone
    code, thres, *_ = raw_call(model, counts, [50., 90.], cap=0, want_cells=False)
    assert code == _lib.GF_OK and thres[1, 1] == full[1][1].thres
    # the Python wrapper with an explicit cap returns the truncated list and the true count
    r = contour.credible_region(counts[0], 90., model=model, cap=7)
    assert r.thres == full[0][1].thres and np.array_equal(r.flat_cells, full[0][1].flat_cells[:7])


def test_reflect_boundary_against_scipy(model):
    """one count in a corner cell, radius 2: every tap that leaves the cube comes back reflected (d c b a | a b c d | d c b a)"""
    for nb, corner in ((7, (0, 0, 0)), (7, (6, 6, 6)), (7, (0, 6, 3)), (3, (2, 0, 2)), (2, (1, 0, 1)), (1, (0, 0, 0))):
        counts = np.zeros((nb, nb, nb), dtype=np.uint64)
        counts[corner] = 1
        for sigma in (0.6, 1.5):                     # radius 2 and 6: wider than the small cubes
            res, hs = contour.credible_region(counts, 90., sigma, model=model, want_smoothed=True)
            want = gaussian_filter(counts / counts.sum(), sigma=sigma)
            tol = 3 * (2 * contour.gaussian_radius(sigma) + 3) * 2.0 ** -52
            print("corner %r of %d^3, sigma %g: bit-equal %s" % (corner, nb, sigma, np.array_equal(hs, want)))
            assert np.all(np.abs(hs - want) <= tol * want), (nb, corner, sigma)
            assert abs(hs.sum() - 1.0) < 1e-12


def test_bad_arguments(model):
    counts = np.zeros((3, 3, 3), dtype=np.uint64)
    counts[0, 0, 0] = 1
    ok = raw_call(model, counts, [90.])[0]
    assert ok == _lib.GF_OK
    w5 = contour.gaussian_weights(0.6)
    assert raw_call(model, counts, [90.], nbins=0)[0] == _lib.GF_ERR_INVALID_ARG
    assert raw_call(model, np.zeros((1, 1, 1), dtype=np.uint64), [90.], nbins=1025)[0] == _lib.GF_ERR_INVALID_ARG
    assert raw_call(model, counts, [90.], ncov=0)[0] == _lib.GF_ERR_INVALID_ARG
    assert raw_call(model, counts, [90.] * 9)[0] == _lib.GF_ERR_INVALID_ARG
    for bad in (0., -1., 100.0000001, np.nan, np.inf):
        assert raw_call(model, counts, [90., bad])[0] == _lib.GF_ERR_INVALID_ARG, bad
    assert raw_call(model, counts, [90.], cap=-1)[0] == _lib.GF_ERR_INVALID_ARG
    assert raw_call(model, counts, [90.], radius=-1, weights=w5)[0] == _lib.GF_ERR_INVALID_ARG
    assert raw_call(model, counts, [90.], radius=2, weights=None)[0] == _lib.GF_ERR_INVALID_ARG
    big = np.full(2 * (_lib.GF_REGION_MAX_RADIUS + 1) + 1, 1.0 / (2 * (_lib.GF_REGION_MAX_RADIUS + 1) + 1))
    assert raw_call(model, counts, [90.], radius=_lib.GF_REGION_MAX_RADIUS + 1, weights=big)[0] == _lib.GF_ERR_UNSUPPORTED
    with pytest.raises(_lib.GolemHipError) as exc:
        contour.credible_region(counts, 90., (_lib.GF_REGION_MAX_RADIUS + 0.5) / 4., model=model)
    assert exc.value.code == _lib.GF_ERR_UNSUPPORTED
    # the largest supported radius works
    edge = np.nextafter((_lib.GF_REGION_MAX_RADIUS + 0.5) / 4., 0.)
    assert contour.gaussian_radius(edge) == _lib.GF_REGION_MAX_RADIUS
    r, hs = contour.credible_region(counts, 90., edge, model=model, want_smoothed=True)
    want = gaussian_filter(counts / 1.0, sigma=edge)
    assert np.all(np.abs(hs - want) <= 3 * (2 * _lib.GF_REGION_MAX_RADIUS + 3) * 2.0 ** -52 * want)
    # 2^53 samples or more in one chain
    counts[1, 1, 1] = 2 ** 53
    assert raw_call(model, counts, [90.])[0] == _lib.GF_ERR_UNSUPPORTED
    counts[1, 1, 1] = 2 ** 53 - 2
    assert raw_call(model, counts, [90.])[0] == _lib.GF_OK


def test_eight_coverages_in_one_call_equal_eight_calls(model):
    frs = compositions("peak")[:200000]
    counts = model.flavor_histogram(frs, 64)
    covs = [99., 10., 68.27, 90., 50., 95.45, 100., 1.]              # any order
    for sigma in (0.05, 0.6):
        together = contour.credible_region(counts, covs, sigma, model=model)
        for c, r in zip(covs, together):
            one = contour.credible_region(counts, c, sigma, model=model)
            assert same_region(r, one) and r.coverage == c, (sigma, c)
        by_cov = dict(zip(covs, together))
        assert by_cov[1.].thres <= by_cov[10.].thres <= by_cov[50.].thres <= by_cov[90.].thres <= by_cov[99.].thres


# ---- from the sampler ----------------------------------------------------------------------------------------------------------
def test_sampler_regions():
    ps = Cf.unitary_paramset()
    m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    pms = [Model(compile_model(ps, "PRIOR_ONLY", source_ratio=x)) for x in ([1., 0., 0.], [0., 1., 0.])]
    np.random.seed(8)
    p0 = np.stack([mcmc_utils.flat_seed(ps, 64) for _ in range(2)])
    s = mcmc_utils.DeviceEnsembleSampler(64, 4, m, nchains=2, seed=21)
    covs = [90., 99.]
    try:
        s.run_mcmc(p0, 400)
        for nbins, oversample in ((20, 1.), (25, 2.)):
            nb = int(nbins * oversample) + 1
            for models in (None, pms):
                post = s.postprocess(want_fr=True, nbins=nb, models=models)
                for sigma in (0.05, 0.6):
                    got = s.regions(nbins, covs, hist_smooth=sigma, oversample=oversample, models=models)
                    want = contour.credible_region(post["hist"], covs, sigma, model=m)
                    assert len(got) == 2 and len(got[0]) == 2
                    for c in range(2):
                        for q in range(2):
                            assert same_region(got[c][q], want[c][q]), (nb, models is None, sigma, c, q)
                            assert got[c][q].nbins == nb and got[c][q].thres > 0
                for c in range(2):                   # and the reference on the compositions the sampler returns
                    _, H_s, H_rs, H_crs, thres = reference_region(post["fr"][c], nb, covs, 0.05)
                    got = s.regions(nbins, covs, oversample=oversample, models=models)
                    for q in range(2):
                        check_exact_region(got[c][q], H_s, H_rs, H_crs, thres[q], "sampler chain %d coverage %g" % (c, covs[q]))
        one = s.regions(20, 90.)                     # one coverage: [chain] RegionResult
        assert len(one) == 2 and isinstance(one[0], contour.RegionResult)
    finally:
        s.close()
        for x in pms + [m]:
            x.close()


# ---- from the scan -------------------------------------------------------------------------------------------------------------
def test_scan_saves_the_regions_of_every_point(tmp_path, capsys):
    from golemflavor_amd import scan
    args = ["--config", "C4", "--points", "2", "--nwalkers", "128", "--burnin", "20", "--nsteps", "60"]
    covs = [90., 99.]
    ns = argparse.Namespace(dimension=6, texture="OET")
    pts = scan.texture_grid(6)[:2]
    dirs = {}
    for tag, extra in (("plain", []), ("regions", ["--regions", "90", "99"]), ("nostack", ["--no-stack", "--regions", "90", "99"])):
        dirs[tag] = str(tmp_path / tag)
        scan.main(args + ["--datadir", dirs[tag]] + extra)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert ("regions" in line) == bool(extra)
        if extra:
            assert line["regions"]["coverage"] == covs and line["regions"]["points"] == 2 and line["regions"]["bins_per_axis"] == 126
    assert sorted(os.listdir(dirs["plain"])) == sorted(scan.point_filename("C4", p, ns) + ".npy" for p in pts)
    for g, p in enumerate(pts):
        stem = scan.point_filename("C4", p, ns)
        with open(os.path.join(dirs["plain"], stem + ".npy"), "rb") as f, open(os.path.join(dirs["regions"], stem + ".npy"), "rb") as h:
            assert f.read() == h.read()              # --regions changes no chain file
        for tag in ("regions", "nostack"):
            rows = np.load(os.path.join(dirs[tag], stem + ".npy"))
            with np.load(os.path.join(dirs[tag], "contour_region_%s.npz" % stem)) as z:
                z = {k: z[k] for k in z.files}
            assert int(z["nbins"]) == 126 and np.array_equal(z["coverage"], covs)
            good = np.isfinite(rows[:, :3]).all(axis=1)
            if not good.any():                       # the reference would have raised on every sample: no region
                assert np.all(z["thres"] == 0) and z["cells"].shape == (0, 3)
                continue
            with np.errstate(invalid="ignore"):
                _, H_s, H_rs, H_crs, thres = reference_region(rows[:, :3], 126, covs, 0.05)
            assert np.sum(H_s) > 0
            for q in range(2):
                t = int(z["thres"][q])
                r = contour.RegionResult(126, covs[q], t, z["saturated"][q], z["level_in"][q], z["level_out"][q], z["mass"][q],
                                         (z["cells"][:t, 0] * 126 + z["cells"][:t, 1]) * 126 + z["cells"][:t, 2], z["density"][:t])
                check_exact_region(r, H_s, H_rs, H_crs, thres[q], "scan %s point %d coverage %g" % (tag, g, covs[q]))
