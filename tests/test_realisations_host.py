"""Realisation ensembles, the parts that need no device: the host build of csrc/gf_toys.hpp (tests/toys/toys_host.cpp)
against np.lexsort on crafted seed sets, draw_realisations, sensitivity_band and ts_quantiles on synthetic arrays, and the binding of
the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import toys_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import realisations as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return H.build()


def check_case(host, lp, fr, status, bf, sm, offset, K):
    meas = H.measurements(bf, sm, offset)
    scores = H.host_scores(lp, fr, status, meas, host)
    assert not np.isnan(scores).any() and not np.any(scores == np.inf)
    want = H.lexsort_select(scores, K)
    got = H.host_select(lp, fr, status, meas, K, host)
    for g, w, name in zip(got, want, ("index", "score", "count")):
        assert H.same_bits(g, w), name
    return scores, got


@pytest.mark.parametrize("K", [1, 3, 4, 5, 16])
def test_selection_is_lexsort_on_crafted_seeds(host, K):
    # duplicated rows (ties between indices), -inf, NaN and non-unitary rows, Gaussians at -inf; 130 realisations of 700 seeds
    lp, fr, status, bf, sm, off = H.crafted(700, 130, seed=3)
    scores, (index, score, count) = check_case(host, lp, fr, status, bf, sm, off, K)
    assert np.all(count == K)
    # the case has what it is for: ties among the selected, and rows of every excluded kind
    fin = scores[0] > -np.inf
    assert len(np.unique(scores[0][fin])) < fin.sum()
    assert np.all(scores[:, status == H.NON_UNITARY] == -np.inf) and (status == H.NON_UNITARY).sum() > 20
    assert np.all(scores[:, np.isnan(lp)] == -np.inf) and np.isnan(lp).sum() > 5
    assert np.all(scores[:, np.isnan(fr).any(axis=1)] == -np.inf) and np.isnan(fr).any(axis=1).sum() > 5
    far = np.isfinite(lp) & (status == 0) & (np.abs(np.nan_to_num(fr)).max(axis=1) > 1.5)
    assert far.sum() > 10 and np.all(scores[:, far] == -np.inf)


def test_score_is_the_two_operations(host):
    """score = lp + (fma(mh, r2, k) + offset) with r2 = fma(d2, d2, fma(d1, d1, d0 d0)), restated with exact rationals"""
    from fractions import Fraction as F
    lp, fr, status, bf, sm, off = H.crafted(60, 3, seed=11)
    meas = H.measurements(bf, sm, off)
    scores = H.host_scores(lp, fr, status, meas, host)

    def rnd(x):
        return float(x)                                          # Fraction -> nearest double

    def fma(a, b, c):
        return rnd(F(a) * F(b) + F(c))
    checked = 0
    for t in range(3):
        m, mh, k, o = meas[t, :3], meas[t, 3], meas[t, 4], meas[t, 5]
        for i in range(60):
            if status[i] == H.NON_UNITARY or not np.isfinite(lp[i]) or not np.isfinite(fr[i]).all():
                assert scores[t, i] == -np.inf
                continue
            d = [fr[i, j] - m[j] for j in range(3)]
            r2 = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))
            e = fma(mh, r2, k)
            want = lp[i] + (e + o) if e >= -708.3964185322641 else -np.inf
            assert H.same_bits([scores[t, i]], [want]), (t, i)
            checked += 1
    assert checked > 100


def test_ties_all_neginf_and_short_seed_sets(host):
    # every row the same: the K lowest indices
    lp, fr, status, bf, sm, off = H.crafted(40, 5, seed=4, kind="ties")
    _, (index, score, count) = check_case(host, lp, fr, status, bf, sm, off, 16)
    assert np.all(index == np.arange(16)) and np.all(count == 16)
    # nothing finite: no starts
    lp, fr, status, bf, sm, off = H.crafted(50, 4, seed=5, kind="neginf")
    _, (index, score, count) = check_case(host, lp, fr, status, bf, sm, off, 4)
    assert np.all(count == 0) and np.all(index == -1) and np.all(score == -np.inf)
    # fewer seeds than K, and fewer finite seeds than K
    for nseed, K in ((1, 1), (1, 4), (3, 4), (15, 16), (16, 16), (9, 16)):
        lp, fr, status, bf, sm, off = H.crafted(nseed, 7, seed=20 + nseed)
        _, (index, score, count) = check_case(host, lp, fr, status, bf, sm, off, K)
        assert np.all(count <= min(nseed, K))
    assert host.toyh_select(None, None, None, 0, None, 0, 17, None, None, None) == 1      # K beyond the limit
    assert host.toyh_max_starts() == _lib.GF_TOY_MAX_STARTS == R.MAX_TOY_STARTS == 16


def test_draw_realisations_is_deterministic_and_the_stated_throw():
    bf = np.array([0.3, 0.36, 0.34])
    a, b = R.draw_realisations(bf, 0.02, 1000, seed=7), R.draw_realisations(bf, 0.02, 1000, seed=7)
    assert a.shape == (1000, 3) and np.array_equal(a, b)
    assert np.array_equal(a, bf + 0.02 * np.random.default_rng(7).standard_normal((1000, 3)))
    assert not np.array_equal(a, R.draw_realisations(bf, 0.02, 1000, seed=8))
    assert np.array_equal(a[:10], R.draw_realisations(bf, 0.02, 10, seed=7))               # a longer throw extends a shorter one
    # not projected onto the simplex; the moments of the isotropic Gaussian (five standard errors)
    assert np.abs(a.sum(axis=1) - 1.0).max() > 0.01
    assert np.all(np.abs(a.mean(axis=0) - bf) < 5 * 0.02 / np.sqrt(1000))
    assert np.all(np.abs(a.std(axis=0) / 0.02 - 1.0) < 5 / np.sqrt(2 * 1000))
    for bad in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError):
            R.draw_realisations(bf, bad, 3)


def test_sensitivity_band():
    rng = np.random.default_rng(1)
    lim = rng.normal(-40.0, 1.0, 501)
    band = R.sensitivity_band(lim)
    assert band["quantiles"].tolist() == [2.5, 16., 50., 84., 97.5]
    assert np.array_equal(band["limits"], np.percentile(lim, [2.5, 16., 50., 84., 97.5]))
    assert band["limits"][2] == np.median(lim) and band["n"] == 501 and band["n_without_limit"] == 0
    # realisations without a limit (NaN, or profile_likelihood_limit's None) are counted and left out
    holes = lim.copy()
    holes[::10] = np.nan
    band = R.sensitivity_band(holes, quantiles=(16, 50, 84))
    assert np.array_equal(band["limits"], np.percentile(lim[np.isfinite(holes)], [16, 50, 84]))
    assert band["n_without_limit"] == 51 and band["n"] == 501
    mixed = R.sensitivity_band([None, -41.0, None, -39.0], quantiles=(50,))
    assert mixed["limits"].tolist() == [-40.0] and mixed["n_without_limit"] == 2
    for none in ([None] * 4, np.full(4, np.nan), []):
        band = R.sensitivity_band(none)
        assert np.isnan(band["limits"]).all() and len(band["limits"]) == 5 and band["n_without_limit"] == band["n"] == len(none)


def test_ts_quantiles():
    from scipy.stats import chi2
    rng = np.random.default_rng(2)
    ts = rng.chisquare(1, size=(20000, 3))
    ts[:, 0] = 0.0                                                # the null column
    ts[::7, 2] = np.nan                                           # realisations without a finite statistic there
    ts[3::7, 2] = np.inf
    q = R.ts_quantiles(ts)
    assert q.shape == (3,) and q[0] == 0.0
    assert q[1] == np.percentile(ts[:, 1], 95.)
    assert q[2] == np.percentile(ts[np.isfinite(ts[:, 2]), 2], 95.)
    assert abs(q[1] - chi2.ppf(0.95, 1)) < 0.15                   # a chi2(1) sample gives Wilks' threshold back (3.84 +- 0.04)
    q2 = R.ts_quantiles(ts, q=[68., 95.])
    assert q2.shape == (2, 3) and np.array_equal(q2[1], q)
    empty = R.ts_quantiles(np.full((5, 2), np.nan))
    assert empty.shape == (2,) and np.isnan(empty).all()


NEW = ["gf_toys_set_measurements", "gf_toys_set_start_counts", "gf_toys_create", "gf_toys_destroy", "gf_toys_set_run_ids", "gf_toys_seed", "gf_toys_get_seeds",
       "gf_toys_select", "gf_toys_scores", "gf_toy_select"]


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^(?:int|void) %s\(" % name, hdr, re.M), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"#define GF_TOY_MAX_STARTS 16\b", hdr)
    assert re.search(r"#define GF_ABI_VERSION 5\b", hdr) and _lib.GF_ABI_VERSION == 5 and L.gf_abi_version() == 5
    assert _lib.SIGNATURES["gf_toys_set_measurements"] == (C.c_int, [C.c_void_p, _lib._dp, _lib._dp])
    # NULL handles are refused before any device is touched
    assert L.gf_toys_set_measurements(None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_set_start_counts(None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_seed(None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toy_select(0, None, None, None, 0, None, None, 0.0, 0, 0, None, None, None) == _lib.GF_ERR_INVALID_ARG
