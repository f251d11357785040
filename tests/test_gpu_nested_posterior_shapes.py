"""The nested sampler's posterior on the GPU (gf_nested_post.hip) at the shapes where its launch structure does something: runs of one,
two and three leaves of 4096 points in one launch, twelve columns with a fixed one over three leaves, and weights down to the
subnormal range, to exactly 0 and lnw = -inf.  The reference throughout is the host build of gf_nested_post.hpp
(tests/nested_post_harness.py) fed with dead()'s arrays, bit for bit; mean and cov are also held to numpy's definitions in long double
within H.bounds.  test_gpu_nested_posterior.py has the same comparison below one leaf.

Measured (MI355X; the runs are deterministic, and the conditions the tests need are asserted in them from npoints and dead() alone):
  MIXED, tutorial posterior, nlive 700, batch 87, seed 5         smearing  run id  niter  npoints  leaves  lnw = -inf  subnormal e  finite lnw, e = 0
                                                                    1.0      22     37     3919      1         0           0             0
                                                                    0.12      8     57     5659      2         0           0             0
                                                                    0.02     13     83     7921      2       159          29             0
                                                                    0.01     35     91     8617      3       520          39             5
  WIDE, sens-shaped (12 columns, logLam fixed), nlive 500, batch 62, seed 7: npoints 11102 and 12094 (3 leaves each); about 1200 and 1350
  points of finite lnw and weight exactly 0, about 30 subnormal weights each.
So the deep-range test meets weights of exactly 0 from a finite lnw in the smearing-0.01 run (and the WIDE test in both of its runs),
none in the smearing-0.02 run."""
import math

import numpy as np
import pytest

import nested_post_harness as H
import test_gpu_nested as TN
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import nested

pytestmark = pytest.mark.gpu

SEED, NLIVE = 5, 700
SMEAR, IDS = [1.0, 0.12, 0.02, 0.01], [22, 8, 13, 35]
SHORT, LONG, DEEP = 0, 3, (2, 3)                 # the one-leaf run, the longest one, the runs of the deep-range test
NROWS = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 16384, 20001)          # the last one beyond every run's n
WIDE_SEED, WIDE_NLIVE, WIDE_IDS, WIDE_NROWS = 7, 500, [1, 4], (500, 4097)
SUBNORMAL = 2.0 ** -1022


def _tutorial(smearing):
    asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=smearing)
    return llh_utils.tutorial_ln_prob(asimov, ps)


def _host(s, r, fixed):
    """dead(r) and the host build's posterior of it: the reference, computed once per run"""
    d = s.dead(r)
    return d, H.host_posterior(d["lnw"], d["theta"], fixed)


@pytest.fixture(scope="module")
def mixed():
    """four tutorial runs of different smearing in one sampler: (sampler, models, per run (dead, host posterior))"""
    fs = [_tutorial(sm) for sm in SMEAR]
    s = nested.NestedSampler(fs, [0, 1], np.zeros(2), nlive=NLIVE, seed=SEED, run_ids=IDS)
    s.run()
    yield s, fs, [_host(s, r, [0, 0]) for r in range(len(SMEAR))]
    s.close()
    for f in fs:
        f.close()


@pytest.fixture(scope="module")
def alone(mixed):
    """the one-leaf run and the longest run of `mixed`, each alone in a sampler of its own with its run id"""
    s, fs, ref = mixed
    out = [nested.NestedSampler([fs[r]], [0, 1], np.zeros(2), nlive=NLIVE, seed=SEED, run_ids=[IDS[r]]) for r in (SHORT, LONG)]
    for a in out:
        a.run()
    yield out
    for a in out:
        a.close()


@pytest.fixture(scope="module")
def wide():
    """Cf.sens_paramsets(6, (1, 1, 1)), two scales, nlive 500, non-unitary points outside the support"""
    args = TN.sens_args()
    asimov, ps = TN.sens_sets()
    scales = nested.sens_scales(6, 10)[[1, 4]]
    res = nested.evidence_scan(args, asimov, ps, scales, run_ids=WIDE_IDS, nlive=WIDE_NLIVE, walks=10, seed=WIDE_SEED, on_nonunitary="-inf",
                               return_sampler=True)
    s = res["sampler"]
    fixed = [0 if c in s.cols else 1 for c in range(s.ndim)]
    yield s, fixed, [_host(s, r, fixed) for r in range(2)]
    s.close()
    for m in res["models"]:
        m.close()


def _leaves(n):
    return -(-n // H.LEAF)


def _check_moments(post, r, d, h):
    """ess, mean, cov and lnz_check of run r bit for bit against the host build"""
    n = len(d["lnw"])
    assert post["npoints"][r] == n
    assert H.same_bits(post["ess"][r], h["ess"]), (r, post["ess"][r], h["ess"])
    assert H.same_bits(post["mean"][r], h["mean"]), (r, post["mean"][r] - h["mean"])
    assert H.same_bits(post["cov"][r], h["cov"]), (r, np.abs(post["cov"][r] - h["cov"]).max())
    assert post["lnz_check"][r] == h["m"] + math.log(h["S"]), r
    assert 1.0 < post["ess"][r] <= np.isfinite(d["lnw"]).sum() * (1 + 1e-12)


def _check_rows(rows, index, r, d, h, N, seed, run_id):
    """the N rows of run r: index equal to the host build's resampling of its own prefix, non-decreasing, inside the run, never at a
    point of zero weight; the rows the points' theta"""
    n = len(d["lnw"])
    assert rows.shape[1:] == (N, d["theta"].shape[1]) and index.shape[1:] == (N,)
    ref = H.host_resample(h["C"], N, H.host_offset(seed, run_id))
    assert np.array_equal(index[r], ref), (r, N, int((index[r] != ref).sum()))
    assert index[r].min() >= 0 and index[r].max() < n and np.all(np.diff(index[r]) >= 0), (r, N)
    assert not np.any(h["p"][index[r]] == 0.0), (r, N)
    assert H.same_bits(rows[r], d["theta"][index[r]]), (r, N)


def test_mixed_leaf_counts_equal_the_host_build(mixed):
    """One launch over runs of one, two and three leaves: every number of every run bit for bit, and mean and cov within H.bounds of
    numpy's definitions in long double (a subnormal weight's absolute error, below 2^-1074, is far below the bounds' smallest term)."""
    s, fs, ref = mixed
    post = s.posterior()
    ns = [len(d["lnw"]) for d, h in ref]
    print("npoints %r leaves %r" % (ns, [_leaves(n) for n in ns]))
    assert post["npoints"].tolist() == ns
    assert any(n <= H.LEAF for n in ns) and any(H.LEAF < n <= 2 * H.LEAF for n in ns) and any(n > 2 * H.LEAF for n in ns)
    assert ns[SHORT] <= H.LEAF and ns[LONG] == max(ns) and all(n % H.SCAN_BLOCK for n in ns)
    for r, (d, h) in enumerate(ref):
        _check_moments(post, r, d, h)
        ex = H.exact_posterior(d["lnw"], d["theta"])
        b = H.bounds(ns[r], ex)
        dm, dc = np.abs(post["mean"][r] - ex["mean"]).astype(np.float64), np.abs(post["cov"][r] - ex["cov"]).astype(np.float64)
        print("run %d: largest error / bound: mean %.2e cov %.2e" % (r, (dm / b["mean"]).max(), (dc / b["cov"]).max()))
        assert np.all(dm <= b["mean"]), (r, dm, b["mean"])
        assert np.all(dc <= b["cov"]), (r, dc, b["cov"])
    assert max(NROWS) > max(ns)
    for N in NROWS:
        rows, index = s.posterior_rows(N, return_index=True)
        assert rows.shape[0] == len(ns)
        for r, (d, h) in enumerate(ref):
            _check_rows(rows, index, r, d, h, N, SEED, IDS[r])


def _snapshot(s, Ns):
    post = s.posterior()
    return post, [s.posterior_rows(N, return_index=True) for N in Ns]


def _same_snapshot(a, ra, b, rb):
    """run ra of snapshot a and run rb of snapshot b, bit for bit"""
    (pa, rowsa), (pb, rowsb) = a, b
    for k in ("npoints", "ess", "lnz_check", "mean", "cov"):
        assert H.same_bits(np.asarray(pa[k][ra], np.float64), np.asarray(pb[k][rb], np.float64)), k
    for (xa, ia), (xb, ib) in zip(rowsa, rowsb):
        assert np.array_equal(ia[ra], ib[rb]) and H.same_bits(xa[ra], xb[rb])


def test_stacking_and_call_order_change_no_bit(mixed, alone):
    """The one-leaf run and the three-leaf run alone give what they give stacked with runs of other leaf counts; and neither sampler's
    result depends on whose scratch (one leaf per run, or three) the device cache last held."""
    s, fs, ref = mixed
    short, long_ = alone
    Ns = (1000, 4097, 20001)
    stacked = _snapshot(s, Ns)
    first_long, first_short = _snapshot(long_, Ns), _snapshot(short, Ns)
    assert first_short[0]["npoints"][0] <= H.LEAF and first_long[0]["npoints"][0] > 2 * H.LEAF
    _same_snapshot(first_short, 0, stacked, SHORT)
    _same_snapshot(first_long, 0, stacked, LONG)
    for r, one in ((SHORT, first_short), (LONG, first_long)):          # and against the reference itself
        d, h = ref[r]
        _check_moments({k: v[r:r + 1] for k, v in stacked[0].items()}, 0, d, h)
        _check_moments(one[0], 0, d, h)
        for N, (rows, index) in zip(Ns, one[1]):
            _check_rows(rows, index, 0, d, h, N, SEED, IDS[r])
    for sampler, first in ((long_, first_long), (short, first_short), (long_, first_long), (s, stacked), (short, first_short)):
        again = _snapshot(sampler, Ns)
        for r in range(sampler.nruns):
            _same_snapshot(again, r, first, r)


def test_twelve_columns_one_fixed_over_three_leaves(wide):
    """sens.py's width: the fixed column's rule (mean = the run's base, covariances exactly 0) and STAGE_COV's leaf / column split
    beyond the first leaf, against the host build told which column is fixed"""
    s, fixed, ref = wide
    post = s.posterior()
    fx = [c for c in range(s.ndim) if fixed[c]]
    assert s.ndim == 12 and len(fx) == 1 and sorted(s.cols.tolist() + fx) == list(range(12))
    for r, (d, h) in enumerate(ref):
        n = len(d["lnw"])
        print("run %d: npoints %d, %d points of finite lnw and weight 0, %d subnormal weights" % (
            r, n, int((np.isfinite(d["lnw"]) & (h["e"] == 0)).sum()), int(((h["e"] > 0) & (h["e"] < SUBNORMAL)).sum())))
        assert n > 2 * H.LEAF and n % H.SCAN_BLOCK
        _check_moments(post, r, d, h)
        c = fx[0]
        assert post["mean"][r][c] == s.bases[r][c] and np.all(d["theta"][:, c] == s.bases[r][c])
        for v in (post["cov"][r][c], post["cov"][r][:, c]):
            assert np.all(v == 0.0) and not np.signbit(v).any()
        assert np.all(np.diag(post["cov"][r])[s.cols] > 0)
        assert H.same_bits(post["cov"][r], post["cov"][r].T)
    assert post["mean"][0][fx[0]] != post["mean"][1][fx[0]]            # the two scales
    for N in WIDE_NROWS:
        rows, index = s.posterior_rows(N, return_index=True)
        for r, (d, h) in enumerate(ref):
            _check_rows(rows, index, r, d, h, N, WIDE_SEED, WIDE_IDS[r])


def test_deep_weight_range(mixed):
    """Runs whose weights reach the subnormal range and whose prior holds points of zero likelihood: first the conditions on the input,
    from dead() and the host build alone, then every number bit for bit and no point of zero weight among the rows of any N."""
    s, fs, ref = mixed
    for r in DEEP:
        d, h = ref[r]
        e, lnw = h["e"], d["lnw"]
        ninf, nsub = int(np.isneginf(lnw).sum()), int(((e > 0) & (e < SUBNORMAL)).sum())
        print("run %d (smearing %g): %d points, %d with lnw = -inf, %d subnormal weights, %d of finite lnw and weight 0, %d of p = 0" % (
            r, SMEAR[r], len(lnw), ninf, nsub, int((np.isfinite(lnw) & (e == 0)).sum()), int((h["p"] == 0).sum())))
        assert ninf >= 64 and nsub >= 16
        assert np.all(e[np.isneginf(lnw)] == 0.0) and np.all(h["p"][e == 0] == 0.0)
    post = s.posterior()
    for r in DEEP:
        _check_moments(post, r, *ref[r])
    for N in NROWS:
        rows, index = s.posterior_rows(N, return_index=True)
        for r in DEEP:
            d, h = ref[r]
            _check_rows(rows, index, r, d, h, N, SEED, IDS[r])
            assert np.all(h["p"][index[r]] > 0.0) and np.all(np.isfinite(d["lnw"][index[r]]))
