"""GPU: the posterior marginals (csrc/gf_marginal.hip, golemflavor_amd.marginals) at the shapes of their launch arithmetic that
tests/test_gpu_marginals.py -- widths 4, 6, 9 and 12, at most 62 leaves, 13 rank slots on 4 columns, 198 marginals a call -- does
not reach.  The restatements (np.histogram, np.histogram2d, np.sort, np.percentile, `reference_region`) are that module's; the
reference is never the package's own host code, and every comparison is == unless stated otherwise.

Restated from the source, so that each test can assert from its inputs alone that it reaches the path it is about:
  instance    the kernels are compiled for 8, 12 and 19 columns; a width takes the smallest that holds it (`instance`);
  pair groups a histogram workgroup has 65536 bytes of LDS: 4 W nb1 for the 1-D counters, the rest for whole pairs of 4 nb2^2 bytes
              (`pairs_per_group`); a binning with no room for one pair is refused;
  leaves      4096 rows each (marginals.LEAF_ROWS); the leaves of a chain are added 256 at a trip (`REDUCE_LANES`);
  select      a workgroup holds 60 (column, rank) digit histograms: min(W, 60 // R) columns a group (`columns_per_group`); the
              advance kernel has one lane per (column, rank), 320 of them;
  regions     at most 32768 marginals a batch (`REGION_BATCH`);
  capacity    a sampler's chain has room for 64 stored steps, doubled until it holds them (`chain_capacity`).

Bounds of the moments (derived in tests/test_gpu_marginals.py, not tuned; u = 2^-53, d = marginals.moment_tree_depth(rows)):
  |mean - exact| <= (d + 1) u sum|x| / n =: B,   |cov - exact| <= ((d + 4) u sum|t_k| + n B_i B_j) / (n - 1),
  t_k = (x_ki - m_i)(x_kj - m_j) with m the device mean.  Exact values: fractions.Fraction; for the 1 048 577 rows of
  test_reduce_past_one_trip the rows are integers k 2^-52, so Python's integers give sum x, sum|x| and sum x_i x_j exactly, and the
  mean of math.fsum (the exact sum rounded once, u |sum| <= u sum|x|) is held to (d + 2) u sum|x| / n beside it.  There sum|t_k| is
  computed in floating point: every |t_k| carries three roundings (within 4 u relative), math.fsum adds them exactly and rounds
  once, so the bound uses that sum times (1 + 2^-50).
"""
import ctypes as C
import fractions
import math

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model
from test_gpu_marginals import (LOGLAM, TWO_PI, U, check_counts_and_order_statistics, check_exact_region, planted, reference_counts,
                                reference_region, same_marginals)

pytestmark = pytest.mark.gpu

LDS_BYTES = 65536
REDUCE_LANES = 256
SELECT_SLOTS = 60
ADVANCE_LANES = 320
REGION_BATCH = 32768
MAX_WIDTH = 19                                   # GF_MAX_DIM + 3: a 16-column sample with its composition


def instance(W):
    return 8 if W <= 8 else 12 if W <= 12 else 19


def pairs_per_group(W, nb1, nb2):
    return (LDS_BYTES - 4 * W * nb1) // (4 * nb2 * nb2)


def columns_per_group(W, R):
    return max(1, min(W, SELECT_SLOTS // R))


def chain_capacity(nstored):
    cap = 64
    while cap < nstored:
        cap *= 2
    return cap


# nineteen ranges, no two alike; LOGLAM's and 2 pi's edges are not representable exactly
RANGES = [(0., 1.), LOGLAM, TWO_PI, (-3.7, 11.3), (0., 4.), (-2.5, 3.), (1e-3, 1e3), (-1., 1.), (990., 1010.), (0.1, 0.7), (-1e-6, 1e-6),
          (-np.pi, np.pi), (5., 6.), (-100., 0.3), (0., 1. / 3.), (2. ** -20, 2. ** 20), (-0.5, 0.25), (1., np.e), (-7.1, -2.9)]
assert len(RANGES) == MAX_WIDTH == len(set(RANGES))


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


def check_regions_without_cells(res, coverage, what):
    """thres, the levels and the mass of every marginal against `reference_region` on the returned counts (which the caller has
    compared with numpy); which of several equal cells are inside is not compared, so no tie exemption is needed"""
    for kind, counts, regs in ((1, res.counts1, res.regions1), (2, res.counts2, res.regions2)):
        assert len(regs) == len(counts), what
        for k in range(len(counts)):
            if counts[k].sum() == 0:
                continue                                          # H / np.sum(H) of nothing: the reference defines no region
            H_s, H_rs, H_crs, thres = reference_region(counts[k], coverage, 0.05)
            for t in range(len(coverage)):
                check_exact_region(regs[k][t], H_s, H_rs, H_crs, thres[t], "%s: %d-D marginal %d coverage %g" % (what, kind, k, coverage[t]),
                                   cells_too=False)


# ---- 1. widths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 8, 9, 12, 13, 15, 19])
def test_every_width_bins_and_selects_as_numpy(model, W):
    """The 19-wide instances (widths 13, 15 -- a C5 chain with its composition -- and 19, the ABI's promise: k_marg_hist<19> with
    its unrolled 171-pair loop, k_marg_sum<19>), both sides of the instance boundaries 8/9 and 12/13, and widths 1 and 2: at
    W = 1 there is no pair, counts2 and regions2 are empty and the 2-D region stage is skipped; at W = 2 there is one.  Rows as
    `planted`: on every edge, one ulp to either side, outside, +/-inf, NaN in one column; 9001 rows are two full leaves and a
    partial one.  At W = 19 also 100/50 bins: 171 pairs in groups of 5, the last group holding one."""
    assert {instance(w) for w in (1, 2, 8)} == {8} and {instance(w) for w in (9, 12)} == {12} and {instance(w) for w in (13, 15, 19)} == {19}
    ranges = RANGES[:W]
    binnings = [(20, 12)] + ([(100, 50)] if W == MAX_WIDTH else [])
    x = planted(ranges, (20, 12, 100, 50), nrows=9001, nan_col=min(1, W - 1))
    assert 2 * mg.LEAF_ROWS < len(x) < 3 * mg.LEAF_ROWS and x.shape[1] == W
    q, ranks = (2.5, 50., 99.5), (0, -1, 1, 4500, -4500, 5000000)
    npairs = W * (W - 1) // 2
    assert W > 2 or npairs == W - 1                               # no pair, one pair
    for nb1, nb2 in binnings:
        ppg = pairs_per_group(W, nb1, nb2)
        if (nb1, nb2) == (100, 50):
            assert ppg == 5 and npairs == 171 and npairs > ppg and npairs % ppg == 1      # 35 groups, a partial last one
        res = mg.chain_marginals(x, ranges, model=model, bins_1d=nb1, bins_2d=nb2, percentiles=q, ranks=ranks, cap_2d=nb2 * nb2)
        what = "width %d, bins %d/%d" % (W, nb1, nb2)
        assert res.counts2.shape == (npairs, nb2, nb2) and len(res.regions2) == npairs and len(res.pairs) == npairs, what
        check_counts_and_order_statistics(res, x, ranges, nb1, nb2, q, ranks, what)         # every pair against np.histogram2d
        assert res.counts1.sum() > 0 and (npairs == 0 or res.counts2.sum() > 0)
        check_regions_without_cells(res, (90., 99.), what)
    if W == 1:
        assert res.counts2.size == 0 and res.regions2 == [] and res.as_arrays()["r2_thres"].shape == (0, 2)


# ---- 2. pair groups at the LDS limit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,nb1,nb2,lds", [(4, 10, 100, 40160), (2, 127, 127, 65532), (3, 85, 127, 65536)])
def test_one_pair_per_group_up_to_the_largest_binning(model, W, nb1, nb2, lds):
    """Pair groups at their limits: one pair per group needs nb2 >= 91 (4 x 10 / 100: six groups of one pair); the largest accepted
    binnings, 4 W nb1 + 4 nb2^2 = 65532 (2 x 127 / 127, one pair) and 65536 exactly, every byte of the workgroup's LDS (3 x 85 / 127,
    three groups).  gf_region_check_args refuses none of them (its limit is 1024 bins), so these are the marginals' own limit."""
    npairs = W * (W - 1) // 2
    assert 4 * W * nb1 + 4 * nb2 * nb2 == lds <= LDS_BYTES and nb2 >= 91 and pairs_per_group(W, nb1, nb2) == 1 and npairs >= 1
    assert lds != 65532 or 4 * W * nb1 + 4 * (nb2 + 1) ** 2 > LDS_BYTES
    ranges = RANGES[:W]
    x = planted(ranges, (nb1, nb2), nrows=5003, nan_col=1)
    q, ranks = (16., 84.), (0, -1)
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=nb1, bins_2d=nb2, percentiles=q, ranks=ranks)
    check_counts_and_order_statistics(res, x, ranges, nb1, nb2, q, ranks, "%d x %d / %d" % (W, nb1, nb2))
    assert all(res.counts2[p].sum() > 0 for p in range(npairs))
    check_regions_without_cells(res, (90., 99.), "%d x %d / %d" % (W, nb1, nb2))


def test_smallest_refused_binning_leaves_the_model_usable(model):
    """The smallest refused binning: 4 W nb1 + 4 nb2^2 = 65540 (2 x 128 / 127), four bytes past the LDS of a workgroup, is
    GF_ERR_UNSUPPORTED, as are its neighbours 3 x 86 / 127 and 1 x 1 / 128; the model computes the same marginals afterwards."""
    rng = np.random.default_rng(2)
    for W, nb1, nb2 in ((2, 128, 127), (3, 86, 127), (1, 1, 128)):
        assert 4 * W * nb1 + 4 * nb2 * nb2 > LDS_BYTES
        x = rng.random((100, W))
        with pytest.raises(_lib.GolemHipError) as err:
            mg.chain_marginals(x, [(0., 1.)] * W, model=model, bins_1d=nb1, bins_2d=nb2)
        assert err.value.code == _lib.GF_ERR_UNSUPPORTED, (W, nb1, nb2)
    assert 4 * 2 * 128 + 4 * 127 * 127 == LDS_BYTES + 4           # a multiple of four cannot exceed it by less
    x = rng.random((3000, 2))
    res = mg.chain_marginals(x, [(0., 1.)] * 2, model=model, bins_1d=127, bins_2d=127, ranks=(0,))
    check_counts_and_order_statistics(res, x, [(0., 1.)] * 2, 127, 127, (5., 50., 95.), (0,), "after the refusals")


# ---- 3. moments ------------------------------------------------------------------------------------------------------------------
def check_moments(res, x, entries, what):
    """every mean and the covariance entries `entries` against exact rational arithmetic, within the derived bounds (printed)"""
    W = x.shape[1]
    v = x[~np.isnan(x).any(axis=1)]
    n = len(v)
    assert res.nvalid == n and n > 1, what
    d = mg.moment_tree_depth(len(x))
    F = [[fractions.Fraction(t) for t in v[:, c].tolist()] for c in range(W)]
    mu = [sum(col) / n for col in F]
    B = [(d + 1) * U * float(sum(abs(t) for t in col)) / n for col in F]
    worst = 0.0
    for c in range(W):
        err = abs(fractions.Fraction(float(res.mean[c])) - mu[c])
        worst = max(worst, float(err) / B[c])
        assert err <= B[c], (what, c, float(err), B[c])
    print("%s: mean, d = %d, largest error / bound %.3f" % (what, d, worst))
    m = [fractions.Fraction(float(t)) for t in res.mean]
    for i, j in entries:
        exact = sum((a - mu[i]) * (b - mu[j]) for a, b in zip(F[i], F[j])) / (n - 1)
        sabs = float(sum(abs((a - m[i]) * (b - m[j])) for a, b in zip(F[i], F[j])))
        bound = ((d + 4) * U * sabs + n * B[i] * B[j]) / (n - 1)
        err = abs(fractions.Fraction(float(res.cov[i, j])) - exact)
        print("%s: cov[%d,%d] error %.3e bound %.3e" % (what, i, j, float(err), bound))
        assert err <= bound, (what, i, j, float(err), bound)
    assert np.array_equal(res.cov, res.cov.T), what


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_moments_at_the_leaf_edges(model, n):
    """Leaf edges: 4095, 4096 and 4097 rows -- a leaf one row short, a full one, and a second leaf of a single row -- for nvalid,
    mean and covariance; the last row is far from the others, so leaving it out or adding it twice is 10^10 bounds away."""
    rng = np.random.default_rng(n)
    x = np.stack([rng.normal(1e3, 1., n), rng.uniform(0., 1., n), rng.normal(0., 5., n)], axis=1)
    x[-1] = (1017., 3., -40.)
    assert -(-n // mg.LEAF_ROWS) == (1 if n <= 4096 else 2) and mg.moment_tree_depth(n) == 35
    ranges = [(990., 1020.), (0., 1.), (-30., 30.)]
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=10, ranks=(0, -1))
    check_moments(res, x, [(i, j) for i in range(3) for j in range(3)], "%d rows" % n)
    check_counts_and_order_statistics(res, x, ranges, 10, 10, (5., 50., 95.), (0, -1), "%d rows" % n)
    assert res.order_stats[0, 1] == 1017.


def test_reduce_past_one_trip(model):
    """k_marg_reduce past one trip: 256 x 4096 + 1 rows are 257 leaves, so lane 0 adds leaf 256 to leaf 0 in a second trip; the
    last row, the whole of that leaf, is far from the others.  Rows k 2^-52 with integer k: exact sums from Python's integers."""
    n = REDUCE_LANES * mg.LEAF_ROWS + 1
    leaves = -(-n // mg.LEAF_ROWS)
    assert leaves == 257 > REDUCE_LANES and n > 2 ** 20
    d = mg.moment_tree_depth(n)
    assert d == 16 + 6 + 3 + 2 + 6 + 3
    rng = np.random.default_rng(41)
    k = np.stack([rng.integers(-2 ** 52, 2 ** 52, n), rng.integers(0, 2 ** 52, n)], axis=1)
    k[-1] = (2 ** 52 - 1, 3)
    x = np.ascontiguousarray(k * 2. ** -52)
    assert np.array_equal(x * 2. ** 52, k)                       # every row is its integer exactly
    ranges = [(-1., 1.), (0., 1.)]
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=10, percentiles=(50.,), ranks=(0, -1))
    check_counts_and_order_statistics(res, x, ranges, 10, 10, (50.,), (0, -1), "257 leaves")
    cols = [k[:, c].tolist() for c in range(2)]
    S = [sum(col) for col in cols]
    A = [sum(abs(t) for t in col) for col in cols]
    one = fractions.Fraction(1, 2 ** 52)
    B = []
    for c in range(2):
        exact = fractions.Fraction(S[c], n) * one
        B.append((d + 1) * U * float(A[c] * one) / n)
        err = abs(fractions.Fraction(float(res.mean[c])) - exact)
        print("257 leaves: mean[%d] error %.3e bound %.3e" % (c, float(err), B[c]))
        assert err <= B[c], c
        assert math.fsum(x[:, c]) == float(S[c] * one)           # fsum is the exact sum rounded once
        assert abs(fractions.Fraction(float(res.mean[c])) - fractions.Fraction(math.fsum(x[:, c])) / n) <= (d + 2) * U * float(A[c] * one) / n
    for i, j in ((0, 0), (0, 1), (1, 1), (1, 0)):
        sxy = sum(a * b for a, b in zip(cols[i], cols[j]))
        exact = (sxy - fractions.Fraction(S[i] * S[j], n)) * one * one / (n - 1)
        sabs = math.fsum(np.abs((x[:, i] - res.mean[i]) * (x[:, j] - res.mean[j]))) * (1 + 2. ** -50)
        bound = ((d + 4) * U * sabs + n * B[i] * B[j]) / (n - 1)
        err = abs(fractions.Fraction(float(res.cov[i, j])) - exact)
        print("257 leaves: cov[%d,%d] error %.3e bound %.3e" % (i, j, float(err), bound))
        assert err <= bound, (i, j)
    assert res.cov[0, 1] == res.cov[1, 0] and res.nvalid == n


def test_moments_of_nineteen_columns(model):
    """k_marg_sum<19> and k_marg_cov<19>: 19 correlated columns of different scales, 9001 rows (three leaves), NaN in 50 rows.
    Every mean; the covariance's corners, an inner pair and its mirror image exactly; symmetry of all 361 entries."""
    rng = np.random.default_rng(19)
    n, W = 9001, MAX_WIDTH
    a = rng.normal(0., 1., n)
    x = np.stack([(0.3 * c - 2.) * a * 10. ** (c % 5 - 2) + rng.normal(3. * c, 1. + c, n) for c in range(W)], axis=1)
    x[rng.permutation(n)[:30], 4] = np.nan
    x[rng.permutation(n)[:20], 18] = np.nan
    assert instance(W) == 19 and 2 * mg.LEAF_ROWS < n < 3 * mg.LEAF_ROWS
    ranges = [(-500., 500.)] * W
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=4, percentiles=(50.,))
    assert res.mean.shape == (W,) and res.cov.shape == (W, W) and np.all(np.isfinite(res.cov))
    check_moments(res, x, [(0, 0), (0, 18), (18, 18), (7, 12), (12, 7), (18, 0)], "19 columns")


def nothing_prep(W):
    return mg.prepare(W, [(0., 1.)] * W, bins_1d=10, bins_2d=5, percentiles=(5., 50.), ranks=(0, -1, 3))


def test_degenerate_moments(model):
    """Degenerate moments: a chain whose rows all hold a NaN (nvalid = 0: mean and cov NaN, the columns still have counts and order
    statistics), a column of NaN alone, a chain with exactly one valid row (the mean is that row, cov is NaN under ddof 1), and
    nrows = 0 through gf_marginals: GF_OK, zero counts, nvalid = 0, NaN moments, no order statistic."""
    rng = np.random.default_rng(23)
    n, W = 5000, 4
    ranges, q, ranks = [(0., 1.)] * W, (5., 50.), (0, -1, 3)
    x = rng.random((n, W))
    x[np.arange(n), np.arange(n) % W] = np.nan                   # every row holds one
    assert np.isnan(x).any(axis=1).all() and not np.isnan(x).all(axis=0).any()
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=5, percentiles=q, ranks=ranks)
    check_counts_and_order_statistics(res, x, ranges, 10, 5, q, ranks, "NaN in every row")
    assert res.nvalid == 0 and np.all(res.ncol == n - n // W) and np.isnan(res.mean).all() and np.isnan(res.cov).all()

    x = rng.random((n, W))
    x[:, 2] = np.nan                                             # a column of NaN alone
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=5, percentiles=q, ranks=ranks)
    check_counts_and_order_statistics(res, x, ranges, 10, 5, q, ranks, "a column of NaN")
    assert res.nvalid == 0 and res.ncol[2] == 0 and res.counts1[2].sum() == 0 and np.isnan(res.mean).all() and np.isnan(res.cov).all()

    x = rng.random((n, W))
    x[np.arange(n), np.arange(n) % W] = np.nan
    x[4097] = (0.25, -0.0, 0.7, 1. / 3.)                         # the one valid row, alone in the second leaf's second row
    assert np.count_nonzero(~np.isnan(x).any(axis=1)) == 1
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=10, bins_2d=5, percentiles=q, ranks=ranks)
    check_counts_and_order_statistics(res, x, ranges, 10, 5, q, ranks, "one valid row")
    assert res.nvalid == 1 and np.array_equal(res.mean, x[4097]) and np.isnan(res.cov).all()

    def call(spec, out):
        return model._L.gf_marginals(model._h, None, 0, W, spec, out)
    res = mg.run_marginal_call(call, "gf_marginals of no rows", 1, nothing_prep(W), cap_2d=25)[0]      # raises unless GF_OK
    assert res.nvalid == 0 and not res.counts1.any() and not res.counts2.any() and not res.ncol.any()
    assert res.counts1.shape == (W, 10) and res.counts2.shape == (6, 5, 5)
    assert np.isnan(res.mean).all() and np.isnan(res.cov).all() and res.cov.shape == (W, W)
    assert np.all(res.order_ranks == -1) and np.isnan(res.order_stats).all() and res.order_stats.shape == (W, 7)
    assert np.isnan(res.percentiles).all()


# ---- 4. several chains with NaN ----------------------------------------------------------------------------------------------------
def test_stacked_chains_with_nan_rows(model):
    """Several chains with NaN rows: nvalid[ch], ncol[ch][c], the negative ranks n + k and the percentile ranks are per chain and
    per column.  Three chains of 5000 rows x 5: chain 0 has NaN in two columns, chain 1 none, chain 2 enough that rank 2500 is
    the last value of one column (n = 2501) and past the end of another (n = 2400)."""
    rng = np.random.default_rng(31)
    n, W = 5000, 5
    ranges = [(0., 1.), LOGLAM, TWO_PI, (-3.7, 11.3), (-2.5, 3.)]
    x = np.stack([np.stack([rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), n) for lo, hi in ranges], axis=1) for _ in range(3)])
    for ch, c, count in ((0, 1, 37), (0, 3, 400), (2, 0, 2499), (2, 4, 2600), (2, 2, 1)):
        x[ch, rng.permutation(n)[:count], c] = np.nan
    nnan = np.isnan(x).sum(axis=1)
    assert not nnan[1].any() and nnan[0].tolist() == [0, 37, 0, 400, 0] and nnan[2].tolist() == [2499, 0, 1, 0, 2600]
    q, ranks = (2.5, 50., 97.5), (0, -1, 1, 2500, -2500)
    got = mg.chain_marginals(x, ranges, model=model, bins_1d=20, bins_2d=12, percentiles=q, ranks=ranks)
    assert len(got) == 3
    for ch in range(3):
        check_counts_and_order_statistics(got[ch], x[ch], ranges, 20, 12, q, ranks, "stacked chain %d" % ch)
        assert same_marginals(got[ch], mg.chain_marginals(x[ch], ranges, model=model, bins_1d=20, bins_2d=12, percentiles=q, ranks=ranks))
    assert got[2].order_ranks[0, 3] == 2500 and got[2].order_ranks[0, 4] == 1 and np.all(got[2].order_ranks[4, 3:5] == -1)
    assert len({r.nvalid for r in got}) == 3 and got[1].nvalid == n


# ---- 5. select at full load --------------------------------------------------------------------------------------------------------
def sort_key(v):
    """the order-preserving unsigned key of a double, as np.sort orders the non-NaN values (-0.0 just below +0.0)"""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def select_rows(nchains, n, W, seed):
    """column 0: 1 + k 2^-52, k < 256 (every key equal but for its last digit); 1: both signs over twelve decades; 2: constant;
    3: +/-0 and denormals; 4: a normal with +/-inf; 5: half NaN; the rest continuous, each with a scale of its own"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nchains, n, W)) * 10. ** rng.integers(-3, 4, (1, 1, W))
    x[:, :, 0] = 1.0 + rng.integers(0, 256, (nchains, n)) * 2. ** -52
    if W > 1:
        x[:, :, 1] = np.where(rng.random((nchains, n)) < 0.5, -1., 1.) * 10. ** rng.uniform(-6., 6., (nchains, n))
    if W > 2:
        x[:, :, 2] = 0.3
    if W > 3:
        pick = rng.integers(0, 4, (nchains, n))
        den = 5e-324 * rng.integers(1, 1000, (nchains, n))
        x[:, :, 3] = np.choose(pick, [0.0, -0.0, den, -den])
    if W > 4:
        x[:, :, 4][rng.random((nchains, n)) < 0.002] = np.inf
        x[:, :, 4][rng.random((nchains, n)) < 0.002] = -np.inf
    if W > 5:
        x[:, :, 5][rng.random((nchains, n)) < 0.5] = np.nan
    return np.ascontiguousarray(x)


SELECT_RANKS = (0, -1, 1, -2, 2500, -2500, 17, 4999, -5000, 7000)
SELECT_Q = (2.5, 50., 97.5)


def test_select_with_every_slot_in_use(model):
    """The select kernels at full load: R = 16 = GF_MARGINAL_MAX_RANKS rank slots on W = 19 columns is cpg = 3, seven column groups,
    the last one holding one column, and 304 of k_marg_select_advance's 320 lanes; two chains.  Column 0's ranks share their prefix
    until the last pass, column 1's lowest and highest part in pass 0."""
    W, n = MAX_WIDTH, 5000
    R = len(SELECT_RANKS) + 2 * len(SELECT_Q)
    assert R == 16 == mg.GF_MARGINAL_MAX_RANKS and W * R == 304 <= ADVANCE_LANES
    cpg = columns_per_group(W, R)
    assert cpg == 3 and -(-W // cpg) == 7 and W - 6 * cpg == 1
    x = select_rows(2, n, W, 61)
    for ch in range(2):
        k0, k1 = sort_key(x[ch, :, 0]), sort_key(x[ch, :, 1])
        assert len(np.unique(k0 >> np.uint64(8))) == 1 and len(np.unique(k0)) == 256          # seven digits shared, the eighth decides
        assert (k1.min() >> np.uint64(56)) != (k1.max() >> np.uint64(56))                  # parted by the first digit
        assert np.isinf(x[ch, :, 4]).sum() > 4 and 2000 < np.isnan(x[ch, :, 5]).sum() < 3000
    ranges = [(-1., 2.)] * W
    got = mg.chain_marginals(x, ranges, model=model, bins_1d=4, bins_2d=2, percentiles=SELECT_Q, ranks=SELECT_RANKS)
    for ch in range(2):
        check_counts_and_order_statistics(got[ch], x[ch], ranges, 4, 2, SELECT_Q, SELECT_RANKS, "full load, chain %d" % ch)
        assert got[ch].order_stats.shape == (W, R) and np.all(got[ch].order_stats[2, :9] == 0.3)
        assert np.all(got[ch].order_ranks[:5, 7] == n - 1) and got[ch].order_ranks[5, 7] == -1 and np.all(got[ch].order_ranks[:, 9] == -1)
        assert same_marginals(got[ch], mg.chain_marginals(x[ch], ranges, model=model, bins_1d=4, bins_2d=2, percentiles=SELECT_Q, ranks=SELECT_RANKS))


def test_select_with_a_partial_second_group_and_with_one_rank(model):
    """Several column groups with R > 6: W = 4, R = 16 is cpg = 3 and a second group of one column; W = 19, R = 1 is one group of
    19 columns with one slot each."""
    n = 5000
    assert columns_per_group(4, 16) == 3 and columns_per_group(MAX_WIDTH, 1) == MAX_WIDTH
    x = select_rows(1, n, 4, 62)[0]
    ranges = [(-1., 2.)] * 4
    res = mg.chain_marginals(x, ranges, model=model, bins_1d=4, bins_2d=2, percentiles=SELECT_Q, ranks=SELECT_RANKS)
    check_counts_and_order_statistics(res, x, ranges, 4, 2, SELECT_Q, SELECT_RANKS, "4 columns, 16 slots")
    x = select_rows(1, n, MAX_WIDTH, 63)[0]
    ranges = [(-1., 2.)] * MAX_WIDTH
    for ranks in ((n // 3,), (-1,)):
        res = mg.chain_marginals(x, ranges, model=model, bins_1d=4, bins_2d=2, percentiles=(), ranks=ranks)
        assert res.order_stats.shape == (MAX_WIDTH, 1)
        check_counts_and_order_statistics(res, x, ranges, 4, 2, (), ranks, "19 columns, one slot")


# ---- 6. regions past one batch -----------------------------------------------------------------------------------------------------
def test_regions_of_the_second_batch(model):
    """The second batch of regions: 200 chains x 171 pairs are 34 200 2-D marginals, 1432 more than a batch; the second batch begins
    inside chain 191 (b0 > 0 on every region output: thres, saturated, the levels, the mass, cells, density)."""
    nchains, n, W = 200, 64, MAX_WIDTH
    npairs = W * (W - 1) // 2
    assert nchains * npairs == 34200 > REGION_BATCH and 191 * npairs < REGION_BATCH < 192 * npairs and nchains * W < REGION_BATCH
    rng = np.random.default_rng(71)
    x = np.ascontiguousarray(rng.beta(2., 3., (nchains, n, W)) * rng.uniform(0.7, 1.1, (nchains, 1, W)))
    ranges = [(0., 1.)] * W
    kw = dict(model=model, bins_1d=8, bins_2d=4, cap_2d=16, percentiles=(50.,), coverage=(90., 99.))
    got = mg.chain_marginals(x, ranges, **kw)
    assert len(got) == nchains
    parts = mg.chain_marginals(x[:100], ranges, **kw) + mg.chain_marginals(x[100:], ranges, **kw)
    for ch in range(nchains):
        assert same_marginals(got[ch], parts[ch]), ch
    for ch in (0, 191, 192, 199):
        check_counts_and_order_statistics(got[ch], x[ch], ranges, 8, 4, (50.,), (), "chain %d of 200" % ch)
        check_regions_without_cells(got[ch], (90., 99.), "chain %d of 200" % ch)
        assert all(len(r[1].flat_cells) == min(r[1].thres, 16) > 0 for r in got[ch].regions2)


# ---- 7. capacity is not length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchains", [1, 3])
def test_chain_whose_capacity_is_not_its_length(model, nchains):
    """A chain whose capacity is not its length: the notebook posterior, 128 walkers, 60 steps, then 90 more with thin = 3: 90 stored
    steps in a chain with room for 128, so chain_stride is not nrows x W.  One chain as the scans have it, and three, where the
    stride places chains 1 and 2."""
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02))
    np.random.seed(4)
    p0 = np.stack([mcmc_utils.flat_seed(ps, 128) for _ in range(nchains)])
    s = (mcmc_utils.DeviceEnsembleSampler(128, 6, m, seed=8) if nchains == 1 else
         mcmc_utils.DeviceEnsembleSampler(128, 6, m, nchains=3, seed=8, stream_ids=[5, 0, 9]))
    try:
        s.run_mcmc(p0[0] if nchains == 1 else p0, 60)
        s.run_mcmc(None, 90, thin=3)
        assert s.nstored == 60 + 90 // 3 == 90 < chain_capacity(90) == 128 and chain_capacity(60) == 64
        x = s.flat_steps().reshape(nchains, -1, 6)
        assert x.shape == (nchains, 90 * 128, 6)
        ranges = [(m.desc.lo[c], m.desc.hi[c]) for c in range(6)]
        q, ranks = (5., 50., 95.), (0, -1)
        got = s.marginals(percentiles=q, ranks=ranks)
        got = [got] if nchains == 1 else got
        assert len(got) == nchains
        for ch in range(nchains):
            check_counts_and_order_statistics(got[ch], x[ch], ranges, 100, 50, q, ranks, "chain %d of %d" % (ch, nchains))
            want = mg.chain_marginals(x[ch], ranges, model=model, names=got[ch].names, percentiles=q, ranks=ranks)
            assert same_marginals(got[ch], want), ch
        assert nchains == 1 or not np.array_equal(x[0], x[1])
    finally:
        s.close()
        m.close()


# ---- 8. edges that are not uniform ---------------------------------------------------------------------------------------------------
def test_edges_that_are_not_uniform(model):
    """Edges that are not uniform, which the C API takes and Python never sends: log-spaced over nine decades and hand-made
    irregular ones; mg_bin's multiplicative guess is then bins off and its two loops do the work.  Against np.histogram and
    np.histogram2d with the same edges; values on every edge and one ulp to either side."""
    rng = np.random.default_rng(83)
    W, nb1, nb2, n = 3, 4, 40, 6000
    e1 = np.array([np.geomspace(1e-6, 1e3, nb1 + 1), [0., 1e-9, 0.5, 0.5000001, 1.], [-3., -2.999, 0., 10., 1e6]])
    e2 = np.array([np.geomspace(1e-6, 1e3, nb2 + 1), np.sort(np.concatenate(([0., 1e-9, 0.5, 0.5000001, 1.], rng.random(nb2 - 4) ** 3))),
                   -5. + np.cumsum(np.concatenate(([0.], rng.lognormal(0., 2., nb2))))])
    assert e1.shape == (W, nb1 + 1) and e2.shape == (W, nb2 + 1) and np.all(np.diff(e1) > 0) and np.all(np.diff(e2) > 0)
    for e in (e1, e2):                                           # not uniform: the widest bin is many times the narrowest
        assert np.all(np.diff(e).max(axis=1) > 100 * np.diff(e).min(axis=1))
    x = np.stack([10. ** rng.uniform(-6.5, 3.5, n), rng.random(n) ** 3 * 1.02 - 0.01, -5. + rng.random(n) ** 4 * (e2[2, -1] + 6.)], axis=1)
    for c in range(W):
        vals = np.concatenate([e1[c], e2[c]])
        vals = np.concatenate([vals, np.nextafter(vals, -np.inf), np.nextafter(vals, np.inf), [np.inf, -np.inf, np.nan]])
        x[rng.permutation(n)[:len(vals)], c] = vals
    ranges = [(e[0], e[-1]) for e in e1]
    prep = mg.prepare(W, ranges, bins_1d=nb1, bins_2d=nb2, percentiles=(50.,))
    prep["edges1"], prep["edges2"] = np.ascontiguousarray(e1), np.ascontiguousarray(e2)

    def call(spec, out):
        return model._L.gf_marginals(model._h, x.ctypes.data_as(_lib._dp), n, W, spec, out)
    res = mg.run_marginal_call(call, "gf_marginals", 1, prep)[0]
    for c in range(W):
        assert np.array_equal(res.counts1[c], np.histogram(x[:, c], bins=e1[c])[0]), c
        assert res.counts1[c].min() > 0, c
    for p, (i, j) in enumerate(mg.pair_list(W)):
        assert np.array_equal(res.counts2[p], np.histogram2d(x[:, i], x[:, j], bins=[e2[i], e2[j]])[0]), (i, j)
        assert res.counts2[p].sum() > n // 2
    # the same rows and edges, one column's edges sent uniform: what Python's own entry point computes
    uni = mg.chain_marginals(x, ranges, model=model, bins_1d=nb1, bins_2d=nb2, percentiles=(50.,))
    assert not np.array_equal(uni.counts1, res.counts1) and np.array_equal(uni.order_stats, res.order_stats, equal_nan=True)
