"""Host side of the nested sampler's posterior (csrc/gf_nested_post.hpp through tests/nested_post_harness.py, golemflavor_amd.sens):
the header's exp against mpmath, the weights and moments against numpy in long double within bounds derived from the summation
tree, the prefix and the resampled indices against np.cumsum / np.searchsorted, the systematic-resampling property, the C
declarations and the driver's refusals.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nested_post_harness as H
from golemflavor_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gf_nested_posterior", "gf_nested_posterior_rows_device", "gf_nested_posterior_rows", "gf_nested_marginals",
       "gf_nested_element_marginals", "gf_nested_regions")
# (profile, n) -> seed: 1, or the first seed after it with which no t_k of any N and offset lies within n 2^-50 of a C_i (H.separation;
# asserted below on the numpy side alone, for every case)
SEED = {(k, n): 1 for k in H.PROFILES for n in H.NS}
SEED.update({("generic", 65537): 2, ("plateau", 65537): 2, ("span600", 4095): 2, ("span600", 4096): 2, ("span600", 4097): 2, ("span600", 65537): 3})


def _offsets(n):
    return [H.U_MIN, H.U_MAX, H.host_offset(25, n)]


@pytest.fixture(scope="module")
def runs():
    """(profile, n) -> (lnw, theta, fixed, host result, long-double result), computed once"""
    out = {}
    for kind in H.PROFILES:
        for n in H.NS:
            lnw, theta, fixed = H.profile(kind, n, SEED[kind, n])
            out[kind, n] = (lnw, theta, fixed, H.host_posterior(lnw, theta, fixed), H.exact_posterior(lnw, theta))
    return out


def test_exp_against_mpmath():
    x = H.exp_grid()
    assert x.min() < -745.19 and x.max() == 0.0 and len(x) > 30000
    got = H.host_exp(x)
    err = H.exact_exp_error_ulp(x, got)
    i = int(np.argmax(err))
    print("exp: largest error %.4f ulp at x = %r over %d arguments (%d subnormal results)" % (err[i], x[i], len(x), int((got < 2.0 ** -1022).sum())))
    assert (got < 2.0 ** -1022).sum() > 4000
    assert err[i] <= 2 * H.EXP_MEASURED_ULP, (err[i], x[i])
    assert err[i] >= 0.5 * H.EXP_MEASURED_ULP                      # the figure in DESIGN.md 6e is the one this grid gives
    sp = H.host_exp(np.array([0.0, -np.inf, np.nan, -1e300, -0.0]))
    assert sp[0] == 1.0 and sp[1] == 0.0 and not np.signbit(sp[1]) and np.isnan(sp[2]) and sp[3] == 0.0 and sp[4] == 1.0


def test_philox_known_answers_and_offset_range():
    """Random123's known-answer vectors of philox4x32-10, and the offset as the 53-bit uniform of the first two words"""
    kat = [([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, out in kat:
        assert H.host_philox(ctr, key).tolist() == out
    seed, rid = 0x1234567800000019, (7 << 32) | 5
    q = H.host_philox([rid & 0xFFFFFFFF, 0xFFFFFFFE, 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) ^ (rid >> 32)])
    u = ((int(q[0]) >> 5) * 67108864 + (int(q[1]) >> 6)) / 9007199254740992.0
    assert H.host_offset(seed, rid) == u and 0.0 <= u < 1.0


@pytest.mark.parametrize("kind", H.PROFILES)
def test_weights_ess_mean_cov_within_derived_bounds(runs, kind):
    """Against numpy's definitions in long double; the bounds are H.bounds' (its docstring is the derivation): the tree's depth,
    the measured exp error and one rounding per operation.  A fixed column has its value as mean and zero covariances exactly."""
    for n in H.NS:
        lnw, theta, fixed, h, ex = runs[kind, n]
        b = H.bounds(n, ex)
        assert np.all(h["e"][np.isneginf(lnw)] == 0.0) and h["e"].max() == 1.0
        assert np.all(np.abs(h["p"] - ex["p"]) <= b["p"] * ex["p"]), (kind, n)
        assert abs(h["ess"] - ex["ess"]) <= b["ess"], (kind, n, h["ess"], ex["ess"])
        assert h["ess"] <= (np.isfinite(lnw).sum()) * (1 + 1e-12)
        assert np.all(np.abs(h["mean"] - ex["mean"]) <= b["mean"]), (kind, n, h["mean"] - ex["mean"], b["mean"])
        assert h["mean"][1] == 0.625 and np.all(h["cov"][1] == 0.0) and np.all(h["cov"][:, 1] == 0.0)
        if "cov" in b:
            assert np.all(np.abs(h["cov"] - ex["cov"]) <= b["cov"]), (kind, n, np.abs(h["cov"] - ex["cov"]).max(), b["cov"].max())
            assert np.array_equal(h["cov"], h["cov"].T)
        else:                                                           # one point carries all the weight: np.cov divides by zero too
            assert not np.isfinite(h["cov"][0, 0])


@pytest.mark.parametrize("n", (4097, 9001, 65537))
@pytest.mark.parametrize("kind", ("generic", "plateau", "span600"))
def test_twelve_columns_two_fixed_within_derived_bounds(kind, n):
    """sens.py's width beyond one leaf (2, 3 and 17 leaves), H.profile_wide: the scanned columns within H.bounds of numpy's
    definitions in long double; the fixed columns' means their values and their covariances zero, exactly; cov symmetric bit for bit.
    This is the width and the length at which the GPU tests take the host build as their reference."""
    lnw, theta, fixed = H.profile_wide(kind, n, 1)
    h, ex = H.host_posterior(lnw, theta, fixed), H.exact_posterior(lnw, theta)
    b = H.bounds(n, ex)
    sc, fx = np.flatnonzero(fixed == 0), np.flatnonzero(fixed)
    assert fx.tolist() == sorted(H.WIDE_FIXED) and all(c % 2 for c in fx) and len(sc) == 10
    dm, dc = np.abs(h["mean"] - ex["mean"])[sc], np.abs(h["cov"] - ex["cov"])[np.ix_(sc, sc)]
    print("%s n %d: largest error / bound: mean %.2e cov %.2e ess %.2e" % (kind, n, (dm / b["mean"][sc]).max(), (dc / b["cov"][np.ix_(sc, sc)]).max(),
                                                                         abs(h["ess"] - ex["ess"]) / b["ess"]))
    assert abs(h["ess"] - ex["ess"]) <= b["ess"]
    assert np.all(dm <= b["mean"][sc]), (dm, b["mean"][sc])
    assert np.all(dc <= b["cov"][np.ix_(sc, sc)]), (dc.max(), b["cov"].max())
    assert np.all(np.diag(h["cov"])[sc] > 0)
    for c in fx:
        assert h["mean"][c] == H.WIDE_FIXED[c]
        assert np.all(h["cov"][c] == 0.0) and np.all(h["cov"][:, c] == 0.0) and not np.signbit(h["cov"][c]).any() and not np.signbit(h["cov"][:, c]).any()
    assert H.same_bits(h["cov"], h["cov"].T)


@pytest.mark.parametrize("kind", H.PROFILES)
def test_prefix_and_index_equal_numpy(runs, kind):
    """C bit for bit against the header's blocked order restated with np.cumsum, and within its bound of np.cumsum in long double;
    the indices equal to np.searchsorted on that C and on np.cumsum(p) itself -- after checking, on the numpy side alone, that no t_k
    lies within n 2^-50 of a C_i, so that the two prefix orders cannot disagree about any row."""
    for n in H.NS:
        lnw, theta, fixed, h, ex = runs[kind, n]
        assert H.same_bits(h["C"], H.prefix_numpy(h["p"])), (kind, n)
        assert np.all(np.abs(h["C"] - ex["C"]) <= H.bounds(n, ex)["C"]), (kind, n)
        cs = np.cumsum(h["p"])
        for N in H.NROWS:
            for u in _offsets(n):
                t, ref = H.resample_numpy(cs, N, u)
                assert H.separation(cs, t) > n * 2.0 ** -50, (kind, n, N, u, H.separation(cs, t))
                idx = H.host_resample(h["C"], N, u)
                assert np.array_equal(idx, H.resample_numpy(h["C"], N, u)[1]), (kind, n, N, u)
                assert np.array_equal(idx, ref), (kind, n, N, u)


@pytest.mark.parametrize("kind", H.PROFILES)
def test_systematic_resampling_property(runs, kind):
    """|count_i - N p_i| < 1 for every point, p in long double, widened only by what the rounding of C can move: a row's t_k lies
    in [C_{i-1}, C_i), an interval whose ends each carry bounds()['C'].  A point of zero weight is never taken."""
    for n in H.NS:
        lnw, theta, fixed, h, ex = runs[kind, n]
        dC = H.bounds(n, ex)["C"]
        for N in H.NROWS:
            for u in _offsets(n):
                idx = H.host_resample(h["C"], N, u)
                assert idx.min() >= 0 and idx.max() < n and np.all(np.diff(idx) >= 0)
                count = np.bincount(idx, minlength=n)
                dev = np.abs(count - N * ex["p"]).astype(np.float64)
                assert dev.max() < 1 + 2 * N * dC, (kind, n, N, u, dev.max())
                assert count[h["p"] == 0].sum() == 0, (kind, n, N, u)


def test_posterior_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert "#define GF_ABI_VERSION 5" in hdr and _lib.GF_ABI_VERSION == 5
    L = _lib.lib()
    assert L.gf_abi_version() == 5
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(L, name), name
    # the new file's internal interface: the one accessor, declared in gf_internal.h
    internal = open(os.path.join(ROOT, "golemflavor_amd", "csrc", "gf_internal.h")).read()
    post = open(os.path.join(ROOT, "golemflavor_amd", "csrc", "gf_nested_post.hip")).read()
    used = set(re.findall(r"\b(gf_internal_\w+)\(", post))
    assert "gf_internal_nested_view" in used
    for name in used:
        assert re.search(r"\b%s\(" % name, internal), name
    assert hasattr(L, "gf_internal_nested_view")


def test_posterior_entry_points_validate_before_touching_the_device():
    L = _lib.lib()
    assert L.gf_nested_posterior(None, None, None, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_posterior_rows(None, 8, 0, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_posterior_rows_device(None, 8, 0, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_marginals(None, 8, 0, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_element_marginals(None, 8, None, None, None) == _lib.GF_ERR_INVALID_ARG
    assert L.gf_nested_regions(None, 8, 10, 0, None, None, 1, 0, *[None] * 7) == _lib.GF_ERR_INVALID_ARG


def test_sens_posterior_is_refused_without_datadir_and_with_frequentist():
    run = lambda *a: subprocess.run([sys.executable, "-m", "golemflavor_amd.sens", *a], cwd=ROOT, capture_output=True, text=True, timeout=120)
    out = run("--posterior")
    assert out.returncode == 2 and "--posterior needs --datadir" in out.stderr
    out = run("--posterior", "--datadir", "/nonexistent", "--stat-method", "frequentist")
    assert out.returncode == 2 and "frequentist" in out.stderr
    out = run("--posterior-elements", "--datadir", "/nonexistent")
    assert out.returncode == 2 and "--posterior-elements needs --posterior" in out.stderr
    out = run("--help")
    assert out.returncode == 0 and "--posterior-rows" in out.stdout and "16384" in out.stdout
