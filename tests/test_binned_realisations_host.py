"""Realisation ensembles of the energy-resolved likelihood, the parts that need no device: the host build of
csrc/gf_toys_binned.hpp (tests/toys/toys_binned_host.cpp) against np.lexsort on crafted seed sets and against exact rationals,
draw_binned_realisations, the binding of the new entry points and the parser."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import toys_binned_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import realisations as R
from golemflavor_amd import sens
from golemflavor_amd.llh import BinnedMeasurement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL = -708.3964185322641


@pytest.fixture(scope="module")
def host():
    return H.build()


def check_case(host, lp, frb, status, meas, sigma, offset, K):
    tab = H.table(meas, sigma)
    scores = H.host_scores(lp, frb, status, tab, offset, host)
    assert not np.isnan(scores).any() and not np.any(scores == np.inf)
    want = H.lexsort_select(scores, K)
    got = H.host_select(lp, frb, status, tab, offset, K, host)
    for g, w, name in zip(got, want, ("index", "score", "count")):
        assert H.same_bits(g, w), name
    return scores, got


@pytest.mark.parametrize("K", [1, 3, 4, 5, 16])
def test_selection_is_lexsort_on_crafted_seeds(host, K):
    # 130 realisations of 700 seeds at 5 bins, widths per realisation
    lp, frb, status, meas, sigma, off = H.crafted(700, 130, 5, seed=3, per_toy_sigma=True)
    assert sigma.shape == (130, 5)
    scores, (index, score, count) = check_case(host, lp, frb, status, meas, sigma, off, K)
    assert np.all(count == K)
    # the case has what it is for: ties among the selected, and rows of every excluded kind
    fin = scores[0] > -np.inf
    assert len(np.unique(scores[0][fin])) < fin.sum()
    assert np.all(scores[:, status == H.NON_UNITARY] == -np.inf) and (status == H.NON_UNITARY).sum() > 20
    assert np.all(scores[:, np.isnan(lp)] == -np.inf) and np.isnan(lp).sum() > 5
    assert np.all(scores[:, lp == -np.inf] == -np.inf) and (lp == -np.inf).sum() > 5
    one_nan = np.isnan(frb).any(axis=2).sum(axis=1) == 1                       # NaN in a single bin
    assert one_nan.sum() > 5 and np.all(scores[:, one_nan] == -np.inf)
    # a single bin at the underflow wall makes the whole score -inf
    e = H.exponents(np.nan_to_num(frb), H.table(meas, sigma))                  # [T][M][nb]
    walled = (e < -746.5).sum(axis=2)
    one_wall = np.isfinite(lp) & (status == 0) & np.isfinite(frb).all(axis=(1, 2)) & np.all(walled == 1, axis=0)
    assert one_wall.sum() > 10 and np.all(scores[:, one_wall] == -np.inf)
    assert H.band_free(frb[np.isfinite(frb).all(axis=(1, 2))], H.table(meas, sigma))


def rnd(x):
    return float(x)                                              # Fraction -> nearest double


def fma(a, b, c):
    return rnd(F(a) * F(b) + F(c))


def exact_terms(fr, tab, t):
    """every bin's term of one seed, operation by operation with exact rationals: None for a bin below the wall"""
    out = []
    for k in range(tab.shape[0]):
        m, mh, kk = tab[k, :3, t], tab[k, 3, t], tab[k, 4, t]
        d = [rnd(F(fr[k, j]) - F(m[j])) for j in range(3)]
        r2 = fma(d[2], d[2], fma(d[1], d[1], rnd(F(d[0]) * F(d[0]))))
        e = fma(mh, r2, kk)
        out.append(e if e >= WALL else None)
    return out


@pytest.mark.parametrize("nb", [1, 3, 20])
def test_score_is_the_stated_operations(host, nb):
    """score = lp + (sum_k fma(mh_k, r2_k, k_k) + offset), the sum ascending in k from 0.0 with one rounding per add, r2 =
    fma(d2, d2, fma(d1, d1, d0 d0)): restated with exact rationals"""
    lp, frb, status, meas, sigma, off = H.crafted(60, 3, nb, seed=11 + nb, smearing=0.1)
    tab = H.table(meas, sigma)
    scores = H.host_scores(lp, frb, status, tab, off, host)
    checked = 0
    for t in range(3):
        for i in range(60):
            if status[i] == H.NON_UNITARY or not np.isfinite(lp[i]) or not np.isfinite(frb[i]).all():
                assert scores[t, i] == -np.inf
                continue
            terms = exact_terms(frb[i], tab, t)
            if any(e is None for e in terms):
                assert scores[t, i] == -np.inf
                continue
            acc = 0.0
            for e in terms:
                acc = rnd(F(acc) + F(e))
            want = rnd(F(lp[i]) + F(rnd(F(acc) + F(off))))
            assert H.same_bits([scores[t, i]], [want]), (t, i)
            checked += 1
    assert checked > 60


def test_the_order_of_the_sum_matters(host):
    """A seed whose terms summed in descending k give another double: the host build gives the ascending one."""
    nb = 20
    lp, frb, status, meas, sigma, off = H.crafted(200, 2, nb, seed=5, smearing=0.1)
    tab = H.table(meas, sigma)
    scores = H.host_scores(lp, frb, status, tab, off, host)
    differ = final = 0
    for i in range(200):
        if status[i] == H.NON_UNITARY or not np.isfinite(lp[i]) or not np.isfinite(frb[i]).all():
            continue
        terms = exact_terms(frb[i], tab, 0)
        if any(e is None for e in terms):
            continue
        up = down = 0.0
        for e in terms:
            up = up + e
        for e in terms[::-1]:
            down = down + e
        assert H.same_bits([scores[0, i]], [lp[i] + (up + off)]), i
        differ += up != down
        final += lp[i] + (down + off) != scores[0, i]
    # the case has seeds whose sum, and whose score, depend on the order: the descending sum is another double
    assert differ > 10 and final > 5, (differ, final)


def test_ties_all_neginf_and_short_seed_sets(host):
    lp, frb, status, meas, sigma, off = H.crafted(40, 5, 4, seed=4, kind="ties")
    _, (index, score, count) = check_case(host, lp, frb, status, meas, sigma, off, 16)
    assert np.all(index == np.arange(16)) and np.all(count == 16)
    lp, frb, status, meas, sigma, off = H.crafted(50, 4, 4, seed=5, kind="neginf")
    _, (index, score, count) = check_case(host, lp, frb, status, meas, sigma, off, 4)
    assert np.all(count == 0) and np.all(index == -1) and np.all(score == -np.inf)
    for nseed, K in ((1, 1), (1, 4), (3, 4), (15, 16), (16, 16), (9, 16)):
        lp, frb, status, meas, sigma, off = H.crafted(nseed, 7, 3, seed=20 + nseed)
        _, (index, score, count) = check_case(host, lp, frb, status, meas, sigma, off, K)
        assert np.all(count <= min(nseed, K))
    assert host.toybh_select(None, None, None, 0, 0, None, 0, 0.0, 17, None, None, None) == 1      # K beyond the limit
    assert host.toybh_max_starts() == _lib.GF_TOY_MAX_STARTS == R.MAX_TOY_STARTS == 16
    assert host.toybh_nconst() == 5


def test_draw_binned_realisations_is_deterministic_and_the_stated_throw():
    edges = np.logspace(4, 7, 21)
    b = BinnedMeasurement.constant((0.3, 0.36, 0.34), 0.02, edges)
    a, a2 = R.draw_binned_realisations(b, 500, seed=7), R.draw_binned_realisations(b, 500, seed=7)
    assert a.shape == (500, 20, 3) and np.array_equal(a, a2)
    z = np.random.default_rng(7).standard_normal((500, 20, 3))
    assert np.array_equal(a, b.fr_bins[None] + b.sigma[None, :, None] * z)
    assert not np.array_equal(a, R.draw_binned_realisations(b, 500, seed=8))
    # not projected onto the simplex, every bin with its own width (five standard errors)
    assert np.abs(a.sum(axis=2) - 1.0).max() > 0.01
    assert np.all(np.abs((a - b.fr_bins[None]).std(axis=(0, 2)) / b.sigma - 1.0) < 5 / np.sqrt(2 * 1500))
    assert len(np.unique(b.sigma)) > 1
    one = BinnedMeasurement([[0.3, 0.3, 0.4]], [0.05])
    assert R.draw_binned_realisations(one, 4).shape == (4, 1, 3)


NEW = ["gf_toys_create_binned", "gf_toys_destroy_binned", "gf_toys_set_run_ids_binned", "gf_toys_seed_binned", "gf_toys_get_seeds_binned",
       "gf_toys_select_binned", "gf_toys_scores_binned", "gf_toy_select_binned", "gf_toys_set_binned_measurements"]


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^(?:int|void) %s\(" % name, hdr, re.M), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert not name.startswith("gf_simplex_")
    assert re.search(r"#define GF_ABI_VERSION 5\b", hdr) and _lib.GF_ABI_VERSION == 5 and L.gf_abi_version() == 5
    assert _lib.SIGNATURES["gf_toys_set_binned_measurements"] == (C.c_int, [C.c_void_p, C.c_int, _lib._dp, _lib._dp])
    for name in ("draw_binned_realisations", "BinnedToySeeds", "toy_select_binned", "binned_realisation_scan"):
        assert name in R.__all__ and hasattr(R, name)
    # NULL handles are refused before any device is touched
    assert L.gf_toys_set_binned_measurements(None, 0, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_create_binned(None, 0, 0, None, None, 0, 0, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_seed_binned(None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_set_run_ids_binned(None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_get_seeds_binned(None, 0, None, None, None, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_select_binned(None, None, 0, None, 0, 0, 0, None, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toys_scores_binned(None, None, 0, None, 0, 0, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_toy_select_binned(0, None, None, None, 0, 0, None, None, 0, 0.0, 0, 0, None, None, None) == _lib.GF_ERR_INVALID_ARG
    L.gf_toys_destroy_binned(None)


def test_parser_takes_realisations_of_the_energy_resolved_likelihood(tmp_path, capsys):
    base = ["--stat-method", "frequentist", "--datadir", str(tmp_path)]
    args = sens.parse_args(base + ["--realisations", "3", "--energy-resolved"])
    assert args.realisations == 3 and args.energy_resolved
    assert sens.realisations_path(args).endswith("_ebins.npz") and os.path.basename(sens.realisations_path(args)).startswith("fr_realisations")
    args = sens.parse_args(base + ["--realisations", "3", "--energy-resolved", "--binned-smearing", "0.2"])
    assert args.binned_smearing == [0.2]
    # without --energy-resolved the path is the flux-averaged one
    assert not sens.realisations_path(sens.parse_args(base + ["--realisations", "3"])).endswith("_ebins.npz")
    # the Bayesian ensemble keeps its refusal
    with pytest.raises(SystemExit):
        sens.parse_args(["--evidence-realisations", "3", "--energy-resolved", "--datadir", str(tmp_path)])
    assert "flux-averaged likelihood" in capsys.readouterr().err
