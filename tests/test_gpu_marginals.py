"""GPU: the posterior marginals of a chain (csrc/gf_marginal.hip, golemflavor_amd.marginals) against numpy / scipy restated here:
np.histogram, np.histogram2d, np.sort, np.percentile, and for the regions `reference_region` -- H / np.sum(H),
scipy.ndimage.gaussian_filter, np.argsort()[::-1], np.cumsum, np.searchsorted (golemflavor/plot.py:371-383 applied to a marginal).
The reference is never the package's own host code.

Exact (==, every element): counts1, counts2, nvalid, ncol, every order statistic, every percentile; of the unsmoothed regions
thres, level_in, level_out, mass, the density of every returned cell, "every cell denser than level_in is inside and none less
dense is" and the number of cells AT level_in that are inside.  Which of several equal cells at the cut are inside is not compared
(np.argsort leaves it unspecified); the package's rule (descending flat index within the marginal's own array) is asserted on a
hand-made histogram.  So that this exemption cannot hide a failure the cells at level_in must be at most 10 % of thres, asserted
from the reference alone, for every marginal of SYNTHETIC (6 columns, 250 000 continuous samples, 100 / 50 bins, coverages 90 and
99).  Measured on the reference before writing the list: the largest fraction over its 6 + 15 marginals x 2 coverages is 2.9 %
(1-D) and 3.2 % (2-D); no case is left out.

Bounds (derived, not tuned; u = 2^-53):
  mean   The device adds the n rows along a fixed tree in which a term passes through at most d additions: 16 (a lane's rows of
         a 4096-row leaf, in order) + 6 (shuffle levels) + 3 (four waves in order) + ceil(leaves / 256) + 6 + 3 over the leaves,
         d = 35 below 2^20 rows.  A sum over a tree of depth d is within d u sum|x| of exact, the division by n adds u |mean| <=
         u sum|x| / n:  |mean - exact| <= (d + 1) u sum|x| / n =: B.
  cov    With t_k = (x_ki - m_i)(x_kj - m_j), m the DEVICE mean: each computed term carries two rounded differences and one
         rounded product (3 u), the tree d u, the division by n - 1 one u: within (d + 4) u sum|t_k| / (n - 1) of
         sum t_k / (n - 1); and sum t_k = sum (x_ki - mu_i)(x_kj - mu_j) + n (mu_i - m_i)(mu_j - m_j) exactly, the centring term,
         at most n B_i B_j.  |cov - exact| <= ((d + 4) u sum|t_k| + n B_i B_j) / (n - 1).
         Exact values: fractions.Fraction on 20 000 rows (5 leaves); math.fsum for the mean of 250 000 rows (62 leaves).
  smoothed regions (sigma 0.6 and 1.5 bins)   every pass sums 2 r + 1 non-negative products, so any summation order is within
         (2 r + 2) u of the exact pass, and so is scipy; p passes compound (p = 1 for a 1-D marginal, 2 for a 2-D one: an axis of
         length 1 is not filtered): H_s within p (2 r + 3) 2^-52 relative of scipy's on every non-zero cell, zero where scipy's is
         zero; thres equal whenever the reference's own margin to the coverage exceeds ncells 2^-52.  Cases below that margin
         (counted from the reference alone): none of the 84.
"""
import fractions
import math
import os

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import scan
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TWO_PI = (0., 2 * np.pi)
LOGLAM = tuple(Cf.SCALE_BOUNDARIES[6])           # edges that are not representable exactly


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def reference_counts(x, ranges, nb1, nb2):
    W = x.shape[1]
    c1 = np.stack([np.histogram(x[:, c], bins=nb1, range=tuple(ranges[c]))[0] for c in range(W)])
    c2 = [np.histogram2d(x[:, i], x[:, j], bins=nb2, range=[tuple(ranges[i]), tuple(ranges[j])])[0] for i in range(W) for j in range(i + 1, W)]
    return c1.astype(np.uint64), np.array(c2, dtype=np.uint64).reshape(len(c2), nb2, nb2)        # (0, nb2, nb2) for one column


def reference_region(counts, coverage, sigma):
    """plot.py:371-383 on one marginal's counts.  Returns H_s, the descending order, its running sum and thres per coverage."""
    H = counts.astype(np.float64)
    H = H / np.sum(H)
    H_s = gaussian_filter(H, sigma=sigma)
    H_r = np.ravel(H_s)
    H_rs = np.argsort(H_r)[::-1]
    H_crs = np.cumsum(H_r[H_rs])
    return H_s, H_rs, H_crs, [int(np.searchsorted(H_crs, c / 100.)) for c in coverage]


def synthetic(n=250000, seed=5):
    """continuous densities in six columns; a few per cent of some columns lie outside their range"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.5, 0.12, n)
    x = np.stack([a, rng.beta(2., 5., n), rng.uniform(0., 2 * np.pi, n), LOGLAM[0] + (LOGLAM[1] - LOGLAM[0]) * (0.6 * a + 0.4 * rng.beta(3., 3., n)),
                  rng.exponential(0.8, n), np.where(rng.random(n) < 0.4, rng.normal(-1., 0.3, n), rng.normal(1.2, 0.5, n))], axis=1)
    return np.ascontiguousarray(x), [(0., 1.), (0., 1.), TWO_PI, LOGLAM, (0., 4.), (-2.5, 3.)]


def planted(ranges, nb_list, seed=9, nrows=None, nan_col=1):
    """rows with values on every edge of every binning, at lo and hi, one ulp on either side of each, outside the range, and NaN
    in one column only; the other entries uniform over a slightly wider range.  nrows: that many rows instead of the default."""
    rng = np.random.default_rng(seed)
    W = len(ranges)
    special = []
    for c, (lo, hi) in enumerate(ranges):
        vals = [lo, hi, lo - 1., hi + 1., np.inf, -np.inf]
        for nb in nb_list:
            e = np.linspace(lo, hi, nb + 1)
            vals += list(e) + list(np.nextafter(e, -np.inf)) + list(np.nextafter(e, np.inf))
        special.append(np.array(vals))
    n = max(len(s) for s in special) * 3 + 4000 if nrows is None else int(nrows)
    assert n >= max(len(s) for s in special) + 37
    x = np.stack([rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), n) for lo, hi in ranges], axis=1)
    for c, s in enumerate(special):
        x[rng.permutation(n)[:len(s)], c] = s
    x[rng.permutation(n)[:37], nan_col] = np.nan                # NaN in one column only
    return np.ascontiguousarray(x)


def check_counts_and_order_statistics(res, x, ranges, nb1, nb2, q, ranks, what):
    c1, c2 = reference_counts(x, ranges, nb1, nb2)
    assert res.counts1.dtype == np.uint64 and np.array_equal(res.counts1, c1), what
    assert np.array_equal(res.counts2, c2), what
    assert res.nvalid == int(np.count_nonzero(~np.isnan(x).any(axis=1))), what
    for c in range(x.shape[1]):
        col = x[:, c]
        s = np.sort(col[~np.isnan(col)])
        n = len(s)
        assert res.ncol[c] == n, what
        for slot, k in enumerate(ranks):
            kk = k if k >= 0 else n + k
            if 0 <= kk < n:
                assert res.order_ranks[c, slot] == kk and res.order_stats[c, slot] == s[kk], (what, c, k)
            else:
                assert res.order_ranks[c, slot] == -1 and np.isnan(res.order_stats[c, slot]), (what, c, k)
        for t, qq in enumerate(q):
            lo, hi = res.order_ranks[c, len(ranks) + 2 * t], res.order_ranks[c, len(ranks) + 2 * t + 1]
            if n == 0:                                            # a column of NaN alone: no rank, NaN as np.percentile of nothing
                assert lo == hi == -1 and np.all(np.isnan(res.order_stats[c, len(ranks) + 2 * t:len(ranks) + 2 * t + 2])), (what, c, qq)
                assert np.isnan(res.percentiles[c, t]), (what, c, qq)
                continue
            assert res.order_stats[c, len(ranks) + 2 * t] == s[lo] and res.order_stats[c, len(ranks) + 2 * t + 1] == s[hi], (what, c, qq)
            assert res.percentiles[c, t] == np.percentile(s, qq), (what, c, qq, res.percentiles[c, t], np.percentile(s, qq))


def check_exact_region(r, H_s, H_rs, H_crs, thres, what, cells_too=True):
    """everything the reference defines, exactly (module docstring); returns the fraction of the region at the cut level"""
    H_r = H_s.ravel()
    n = len(H_r)
    if thres == n:
        assert r.saturated and r.thres == int(np.count_nonzero(H_r)) and r.mass == H_crs[-1] and np.isnan(r.level_out), what
        return 0.0
    assert not r.saturated and r.thres == thres, (what, r.thres, thres)
    assert r.level_out == H_r[H_rs[thres]], what
    if thres == 0:
        assert np.isnan(r.level_in) and r.mass == 0.0 and len(r.flat_cells) == 0, what
        return 0.0
    lin = H_r[H_rs[thres - 1]]
    assert r.level_in == lin and r.mass == H_crs[thres - 1], what
    if not cells_too:
        return 0.0
    f, d = r.flat_cells[:thres], r.density[:thres]
    assert len(f) == thres and r.cells.shape[1] == H_s.ndim, what
    assert np.all(d[:-1] >= d[1:]) and np.all(f[:-1][d[:-1] == d[1:]] > f[1:][d[:-1] == d[1:]]) and len(np.unique(f)) == thres, what
    inside = np.zeros(n, dtype=bool)
    inside[f] = True
    assert np.all(inside[H_r > lin]) and not np.any(inside[H_r < lin]), what
    assert np.array_equal(d, H_r[f]), what
    at_level_ref = int(np.count_nonzero(H_r[H_rs[:thres]] == lin))
    assert int(np.count_nonzero(d == lin)) == at_level_ref, what
    assert np.array_equal(r.cells[:thres], np.stack(np.unravel_index(f, H_s.shape), axis=1)), what
    return at_level_ref / thres


def same_marginals(a, b):
    """two results identical in every array, regions and cell order included"""
    x, y = a.as_arrays(), b.as_arrays()
    assert set(x) == set(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"), k
    return True


# ---- histograms, order statistics, percentiles -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nb1,nb2", [(10, 10), (50, 51), (51, 50), (100, 50)])
def test_planted_rows_bin_exactly_as_numpy(model, nb1, nb2):
    ranges = [(0., 1.), LOGLAM, TWO_PI, (-3.7, 11.3)]
    x = planted(ranges, (10, 50, 51, 100))
    q, ranks = (2.5, 50., 99.5), (0, -1, 1, 5000000)
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=nb1, bins_2d=nb2, percentiles=q, ranks=ranks, cap_2d=nb2 * nb2)
    check_counts_and_order_statistics(res, x, ranges, nb1, nb2, q, ranks, "planted %d/%d" % (nb1, nb2))
    assert res.counts1.sum() > 0 and int(res.counts1[1].sum()) < int(np.count_nonzero(~np.isnan(x[:, 1]))) + 1


def test_constant_and_signed_zero_columns(model):
    n = 70000
    rng = np.random.default_rng(3)
    x = np.stack([np.full(n, 0.3), np.where(rng.random(n) < 0.5, 0.0, -0.0), rng.integers(0, 5, n).astype(np.float64) / 4.,
                  np.where(rng.random(n) < 0.3, np.nan, rng.normal(size=n))], axis=1)
    ranges = [(0., 1.), (-1., 1.), (0., 1.), (-4., 4.)]
    q, ranks = (5., 50., 95., 100., 0.), (0, -1, n // 2)
    res = mg.chain_marginals(x, ranges, model=model, percentiles=q, ranks=ranks, bins_1d=10, bins_2d=10)
    check_counts_and_order_statistics(res, x, ranges, 10, 10, q, ranks, "constant / zeros")
    assert np.all(res.order_stats[1] == 0.0)


# ---- moments ---------------------------------------------------------------------------------------------------------------------
def test_mean_and_covariance_within_the_tree_bound(model):
    rng = np.random.default_rng(17)
    n, W = 20000, 4
    x = np.stack([rng.normal(1e3, 1., n), rng.uniform(0., 1., n), rng.normal(0., 5., n), rng.exponential(2., n)], axis=1)
    x[rng.permutation(n)[:50], 2] = np.nan                       # rows left out of the moments
    ranges = [(990., 1010.), (0., 1.), (-30., 30.), (0., 30.)]
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=10)
    v = x[~np.isnan(x).any(axis=1)]
    nv = len(v)
    assert res.nvalid == nv == n - 50
    d = 16 + 6 + 3 + 1 + 6 + 3                                   # 5 leaves
    F = [[fractions.Fraction(float(t)) for t in v[:, c]] for c in range(W)]
    mu = [sum(col) / nv for col in F]
    B = [(d + 1) * U * float(sum(abs(t) for t in col)) / nv for col in F]
    for c in range(W):
        err = abs(fractions.Fraction(float(res.mean[c])) - mu[c])
        print("mean[%d]: error %.3e bound %.3e" % (c, float(err), B[c]))
        assert err <= B[c], c
    m = [fractions.Fraction(float(t)) for t in res.mean]
    for i in range(W):
        for j in range(W):
            exact = sum((a - mu[i]) * (b - mu[j]) for a, b in zip(F[i], F[j])) / (nv - 1)
            sabs = float(sum(abs((a - m[i]) * (b - m[j])) for a, b in zip(F[i], F[j])))
            bound = ((d + 4) * U * sabs + nv * B[i] * B[j]) / (nv - 1)
            err = abs(fractions.Fraction(float(res.cov[i, j])) - exact)
            print("cov[%d,%d]: error %.3e bound %.3e" % (i, j, float(err), bound))
            assert err <= bound, (i, j)
            assert res.cov[i, j] == res.cov[j, i]
    # 62 leaves
    x, ranges = synthetic()
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=10)
    d = 16 + 6 + 3 + 1 + 6 + 3
    for c in range(x.shape[1]):
        exact = fractions.Fraction(math.fsum(x[:, c])) / len(x)          # fsum: the exact sum, rounded once (u |sum|)
        bound = (d + 2) * U * math.fsum(np.abs(x[:, c])) / len(x)
        assert abs(fractions.Fraction(float(res.mean[c])) - exact) <= bound, c


# ---- regions -----------------------------------------------------------------------------------------------------------------------
def test_unsmoothed_regions_of_every_marginal_equal_the_reference(model):
    x, ranges = synthetic()
    cov = (90., 99.)
    res = mg.chain_marginals(x, ranges, model=model, coverage=cov)
    c1, c2 = reference_counts(x, ranges, 100, 50)
    assert np.array_equal(res.counts1, c1) and np.array_equal(res.counts2, c2)
    worst = {1: 0.0, 2: 0.0}
    for kind, counts, regs in ((1, c1, res.regions1), (2, c2, res.regions2)):
        for k in range(len(counts)):
            H_s, H_rs, H_crs, thres = reference_region(counts[k], cov, 0.05)
            for t, c in enumerate(cov):
                what = "%d-D marginal %d coverage %g" % (kind, k, c)
                lin = H_s.ravel()[H_rs[thres[t] - 1]]
                frac = np.count_nonzero(H_s == lin) / thres[t]
                worst[kind] = max(worst[kind], frac)
                assert frac <= 0.10, (what, frac)                 # the condition on the input, from the reference alone
                check_exact_region(regs[k][t], H_s, H_rs, H_crs, thres[t], what)
    print("largest fraction of a region at its cut level: 1-D %.4f, 2-D %.4f" % (worst[1], worst[2]))


def test_tie_rule_and_single_cell(model):
    # a hand-made 4 x 4 histogram with equal counts: the order is descending count, then descending flat index
    cnt = np.array([[5, 2, 2, 0], [2, 5, 1, 1], [0, 1, 5, 2], [3, 3, 0, 1]])
    centres = (np.arange(4) + 0.5) / 4.
    x = np.array([(centres[i], centres[j]) for i in range(4) for j in range(4) for _ in range(cnt[i, j])])
    res = mg.chain_marginals(x, [(0., 1.), (0., 1.)], model=model, bins_1d=4, bins_2d=4, coverage=(50., 100.))
    assert np.array_equal(res.counts2[0], cnt) and np.array_equal(res.counts1[0], cnt.sum(axis=1))
    flat = cnt.ravel()
    order = sorted(range(16), key=lambda f: (-flat[f], -f))
    order = [f for f in order if flat[f] > 0]
    big = res.regions2[0][1]
    H_s, H_rs, H_crs, thres = reference_region(cnt, (50., 100.), 0.05)
    for t in range(2):
        check_exact_region(res.regions2[0][t], H_s, H_rs, H_crs, thres[t], "hand-made, coverage %d" % t, cells_too=False)
    assert list(big.flat_cells) == order[:big.thres] and list(res.regions2[0][0].flat_cells) == order[:thres[0]]
    assert np.array_equal(big.density, (flat / flat.sum())[big.flat_cells])
    r1 = res.regions1[1][1]                                       # column 1: counts (10, 11, 8, 4): no ties
    assert list(r1.flat_cells) == [int(f) for f in np.argsort(cnt.sum(axis=0))[::-1][:r1.thres]]
    # all the mass in one cell, coverage 100: np.searchsorted(cumsum, 1.0) = 0 cells, the cell that reaches the coverage is outside
    x = np.tile([0.3, 0.7], (1000, 1))
    res = mg.chain_marginals(x, [(0., 1.), (0., 1.)], model=model, bins_1d=10, bins_2d=10, coverage=(100.,))
    for r, counts in ((res.regions1[0][0], res.counts1[0]), (res.regions2[0][0], res.counts2[0])):
        H_s, H_rs, H_crs, thres = reference_region(counts, (100.,), 0.05)
        assert thres == [0] and r.thres == 0 and not r.saturated and r.level_out == 1.0 and np.isnan(r.level_in) and r.mass == 0.0


def test_smoothed_regions_against_scipy(model):
    x, ranges = synthetic()
    cov = (90., 99.)
    c1, c2 = reference_counts(x, ranges, 100, 50)
    cases = below = 0
    for sigma in (0.6, 1.5):
        r = int(4.0 * sigma + 0.5)
        res = mg.chain_marginals(x, ranges, model=model, coverage=cov + (100.,), hist_smooth=sigma, cap_2d=2500)
        for kind, counts, regs, p in ((1, c1, res.regions1, 1), (2, c2, res.regions2, 2)):
            tol = p * (2 * r + 3) * 2.0 ** -52
            for k in range(len(counts)):
                H_s, H_rs, H_crs, thres = reference_region(counts[k], cov, sigma)
                H_r = H_s.ravel()
                big = max(regs[k], key=lambda g: len(g.flat_cells))           # the longest list: every cell the device sorted
                f, dens = big.flat_cells, big.density
                assert len(f) >= regs[k][1].thres and np.all(H_r[f] != 0), (kind, k, sigma)
                assert np.abs(dens - H_r[f]).max() <= tol * H_r[f].max() and np.all(np.abs(dens - H_r[f]) <= tol * H_r[f]), (kind, k, sigma)
                if regs[k][2].saturated:                           # the whole support came back: zero exactly where scipy's is zero
                    assert regs[k][2].thres == np.count_nonzero(H_r) == len(f), (kind, k, sigma)
                for t, c in enumerate(cov):
                    cases += 1
                    tt = thres[t]
                    margin = min(c / 100. - (H_crs[tt - 1] if tt else 0.), H_crs[tt] - c / 100.)
                    if margin <= H_s.size * 2.0 ** -52:
                        below += 1
                        print("below the margin: %d-D marginal %d sigma %g coverage %g (margin %.3e)" % (kind, k, sigma, c, margin))
                        continue
                    assert regs[k][t].thres == tt and not regs[k][t].saturated, (kind, k, sigma, c)
    print("smoothed cases %d, below the reference's margin %d" % (cases, below))
    assert cases == 84 and below <= 2


# ---- sampled chains ----------------------------------------------------------------------------------------------------------------
def notebook_sampler(nwalkers=512, nsteps=400):
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02))
    np.random.seed(4)
    s = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, m, seed=8)
    s.run_mcmc(mcmc_utils.flat_seed(ps, nwalkers), nsteps)
    return m, s


def test_notebook_chain_and_sampler_entry_point(model):
    m, s = notebook_sampler()
    try:
        x = s.flat_steps()
        assert x.shape == (512 * 400, 6)
        ranges = [(m.desc.lo[c], m.desc.hi[c]) for c in range(6)]
        q, ranks = (5., 50., 95.), (0, -1)
        got = s.marginals(percentiles=q, ranks=ranks)
        assert [tuple(r) for r in got.ranges] == ranges           # the default: the model's box
        check_counts_and_order_statistics(got, x, ranges, 100, 50, q, ranks, "notebook chain")
        for kind, counts, regs in ((1, got.counts1, got.regions1), (2, got.counts2, got.regions2)):
            for k in range(len(counts)):
                H_s, H_rs, H_crs, thres = reference_region(counts[k], (90., 99.), 0.05)
                for t in range(2):
                    check_exact_region(regs[k][t], H_s, H_rs, H_crs, thres[t], "notebook %d-D %d" % (kind, k), cells_too=False)
        # the stored chain on the device and the same rows uploaded: identical in every array
        want = mg.chain_marginals(x, ranges, model=model, names=got.names, percentiles=q, ranks=ranks)
        assert same_marginals(got, want)
        for nb in (10, 51):
            r = s.marginals(bins_1d=nb, bins_2d=nb, percentiles=(50.,))
            check_counts_and_order_statistics(r, x, ranges, nb, nb, (50.,), (), "notebook chain, %d bins" % nb)
    finally:
        s.close()
        m.close()


def test_c5_style_chain_in_a_multi_model_sampler(model):
    pts = scan.sens_grid()[:3]
    jobs = [scan._SensPoint(p, g, nwalkers=512, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(512, 12, [j.f for j in jobs], seed=25, stream_ids=[0, 1, 2])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 400)
        x = s.flat_steps()
        assert x.shape == (3, 512 * 400, 12)
        d = jobs[0].f.model.desc
        ranges = [(d.lo[c], d.hi[c]) for c in range(12)]
        got = s.marginals()
        assert len(got) == 3 and len(got[0].pairs) == 66
        for ch in range(3):
            check_counts_and_order_statistics(got[ch], x[ch], ranges, 100, 50, (5., 50., 95.), (), "C5-style chain %d" % ch)
            # the chains of a multi-model sampler give what the same chains give one at a time
            assert same_marginals(got[ch], mg.chain_marginals(x[ch], ranges, model=model, names=got[ch].names))
        many = mg.chain_marginals(x, ranges, model=model, names=got[0].names)
        assert all(same_marginals(a, b) for a, b in zip(got, many))
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_with_fr_equals_the_marginals_of_the_saved_rows(model):
    pts = scan.texture_grid(6)[:2]
    jobs = [scan._TexturePoint(p, g, dimension=6, texture=scan.Texture.OET, nwalkers=256, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(256, 6, [j.f for j in jobs], seed=25, stream_ids=[0, 1])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 100)
        models = [j.post_model for j in jobs]
        rows = s.postprocess_rows(models=models)
        got = s.marginals(with_fr=True, models=models)
        d = jobs[0].f.model.desc
        ranges = [(0., 1.)] * 3 + [(d.lo[c], d.hi[c]) for c in range(6)]
        assert [tuple(r) for r in got[0].ranges] == ranges
        for ch in range(2):
            check_counts_and_order_statistics(got[ch], rows[ch], ranges, 100, 50, (5., 50., 95.), (), "rows of chain %d" % ch)
            assert same_marginals(got[ch], mg.chain_marginals(rows[ch], ranges, model=model, names=got[ch].names))
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_scan_writes_marginals_beside_unchanged_chain_files(model, tmp_path, capsys):
    import json
    a, b = str(tmp_path / "plain"), str(tmp_path / "with")
    common = ["--config", "C4", "--points", "4", "--nwalkers", "128", "--burnin", "10", "--nsteps", "40"]
    scan.main(common + ["--datadir", a])
    capsys.readouterr()
    scan.main(common + ["--datadir", b, "--marginals", "--marginal-bins-1d", "51", "--marginal-percentiles", "16", "84"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["marginals"]["points"] == 4 and line["marginals"]["bins"] == [51, 50] and line["marginals"]["seconds"] > 0
    chains = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert len(chains) == 4 and sorted(os.listdir(a)) == chains
    assert sorted(os.listdir(b)) == sorted(chains + ["marginals_%s.npz" % f[:-4] for f in chains])
    for f in chains:
        with open(os.path.join(a, f), "rb") as fa, open(os.path.join(b, f), "rb") as fb:
            assert fa.read() == fb.read(), f                      # byte for byte what the scan writes without the flag
        z = np.load(os.path.join(b, "marginals_%s.npz" % f[:-4]))
        rows = np.load(os.path.join(b, f))
        assert rows.shape == (128 * 40, 9) and [tuple(r) for r in z["ranges"][:3]] == [(0., 1.)] * 3
        want = mg.chain_marginals(rows, z["ranges"], model=model, names=list(z["names"]), bins_1d=51, percentiles=(16., 84.)).as_arrays()
        assert set(want) == set(z.files)
        for k in want:
            assert np.array_equal(want[k], z[k], equal_nan=want[k].dtype.kind == "f"), (f, k)
