"""Chain diagnostics without a device: the host build of csrc/gf_diag.hpp (tests/diag/diag_host.cpp) pinned bit for bit to a numpy
restatement of its summation orders, held to a np.longdouble evaluation of the definitions within the bounds those orders give, and
the interface around it.

Inputs (tests/diag_harness.py): AR(1) chains x_i = phi x_{i-1} + sqrt(1 - phi^2) e_i, phi cycling over (0, 0.5, 0.9, 0.7) per
column, default_rng(seed) with seed k for the k-th shape (six shapes: seeds 1 .. 6).

Bounds, with u = 2^-53 (diag_harness.exact_diag):
  |delta A_w(t)|   <= (256 + ceil(n / 256) + 3) u sum_i |y_i y_{i+t}|       blocks of 256 products in order, the blocks in order;
                                                                             3 = the two centring subtractions and the product
  |delta rho_w(t)| <= (dA(t) + |rho_w(t)| dA(0)) / A(0) + u |rho_w(t)|
  |delta rho(t)|   <= mean_w |delta rho_w(t)| + (32 + ceil(nwalkers / 32) + 1) u mean_w |rho_w(t)|
  |delta tau|      <= 2 sum_{t <= window} |delta rho(t)|
and split R-hat's in diag_harness.exact_rhat.  None of them is a measured number.

Measured with the host build on these inputs: the largest |error| / bound of rho is 0.006 (walker-averaged) and 0.039 (ensemble
mean); the window margin min_{M <= window} |M - c taus(M)| is 2.2e-3 or more."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diag_harness as H
from golemflavor_amd import _lib, diagnostics as dg, mcmc as mcmc_utils, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FFT_TOL = H.FFT_TOL

CASES = H.cases()
IDS = ["%dx%dx%d" % s for s, _ in CASES]


@pytest.fixture(scope="module")
def host():
    return {s: H.host_diag(x) for s, x in CASES}


@pytest.mark.parametrize("shape,x", CASES, ids=IDS)
def test_host_build_equals_the_numpy_restatement_bit_for_bit(host, shape, x):
    H.assert_same_bits(host[shape], H.numpy_diag(x), str(shape))


@pytest.mark.parametrize("shape,x", CASES, ids=IDS)
def test_host_build_within_the_derived_bounds_of_the_longdouble_definitions(host, shape, x):
    got, ref = host[shape], H.exact_diag(x)
    for tag in ("", "_mean"):
        # on the reference alone: the window is not decided by rounding
        assert ref["margin" + tag].min() > 1e-6, (tag, ref["margin" + tag])
        assert np.array_equal(got["window" + tag], ref["window" + tag]), tag
        err = np.abs(got["rho" + tag].astype(np.longdouble) - ref["rho" + tag]).astype(np.float64)
        print("%s rho%s: max error / bound %.3e" % (shape, tag, float((err / ref["drho" + tag]).max())))
        assert np.all(err <= ref["drho" + tag]), tag
        terr = np.abs(got["tau" + tag].astype(np.longdouble) - ref["tau" + tag]).astype(np.float64)
        print("%s tau%s: max error %.3e, smallest bound %.3e" % (shape, tag, terr.max(), ref["dtau" + tag].min()))
        assert np.all(terr <= ref["dtau" + tag]), tag
    assert np.all(got["nexcluded"] == 0)


@pytest.mark.parametrize("shape,x", CASES + [((2, 6, 3), H.ar1_chain((2, 6, 3), 11)), ((67, 10, 5), H.ar1_chain((67, 10, 5), 12))],
                         ids=IDS + ["2x6x3", "67x10x5"])
def test_rhat_within_its_bound_odd_lengths_drop_the_middle_step(shape, x):
    got = H.host_diag(x, maxlag=1)["rhat"]
    ref, bound = H.exact_rhat(x)
    n = shape[0]
    if n < 4:
        assert np.all(np.isnan(got)) and np.all(np.isnan(ref))       # halves of one step have no variance
        return
    assert np.all(np.abs(got.astype(np.longdouble) - ref) <= bound), (got, ref, bound)
    if n % 2:
        # the middle step is in neither half: changing it moves nothing
        y = x.copy()
        y[n // 2] += 3.0
        assert np.array_equal(H.host_diag(y, maxlag=1)["rhat"], got)
        y = x.copy()
        y[n // 2 - 1] += 3.0
        assert not np.array_equal(H.host_diag(y, maxlag=1)["rhat"], got)


def test_tau_mean_agrees_with_the_fft_path(host):
    worst = (0.0, None)
    for shape, x in CASES:
        series = H.walker_mean(x)
        want = mcmc_utils.integrated_time(series, c=5, tol=0)
        for d in range(shape[2]):
            rho = mcmc_utils._autocorr_1d(series[:, d])
            assert dg.sokal_window(2.0 * np.cumsum(rho) - 1.0, 5) == host[shape]["window_mean"][d], (shape, d)
        diff = float(np.abs(host[shape]["tau_mean"] - want).max())
        if diff > worst[0]:
            worst = (diff, shape)
        assert diff <= FFT_TOL, (shape, diff)
    print("largest |tau_mean - FFT path| %.3e at %s" % worst)


def test_excluded_series():
    shape, x = CASES[3]
    n, nw, nd = shape
    full = H.host_diag(x)
    y = x.copy()
    y[:, 5, 2] = 0.25                                            # one walker constant in one column
    got = H.host_diag(y)
    assert list(got["nexcluded"]) == [0, 0, 1, 0]
    others = np.delete(y, 5, axis=1)
    assert np.array_equal(got["rho"][2], H.numpy_diag(others)["rho"][2])
    for d in (0, 1, 3):
        assert np.array_equal(got["rho"][d], full["rho"][d]) and got["tau"][d] == full["tau"][d]
    H.assert_same_bits(got, H.numpy_diag(y), "one constant walker")
    y = x.copy()
    y[:, :, 1] = np.arange(nw)[None, :]                          # all walkers constant
    got = H.host_diag(y)
    assert got["nexcluded"][1] == nw and np.isnan(got["tau"][1]) and np.all(np.isnan(got["rho"][1])) and np.isnan(got["rhat"][1])
    assert np.isnan(got["tau_mean"][1]) and np.all(np.isnan(got["rho_mean"][1]))
    assert np.array_equal(got["tau"][[0, 2, 3]], full["tau"][[0, 2, 3]])
    y = x.copy()
    y[17, 3, 0] = np.nan                                         # one NaN sample: its own series only
    got = H.host_diag(y)
    assert list(got["nexcluded"]) == [1, 0, 0, 0]
    assert np.array_equal(got["rho"][0], H.numpy_diag(np.delete(y, 3, axis=1))["rho"][0])
    assert np.array_equal(got["rho"][1:], full["rho"][1:]) and np.array_equal(got["rhat"][1:], full["rhat"][1:])
    assert np.all(np.isnan(got["rho_mean"][0])) and np.array_equal(got["rho_mean"][1:], full["rho_mean"][1:])


@pytest.mark.parametrize("maxlag", [1, 63, 64, 65, 192])
def test_maxlag_gives_the_prefix_of_the_full_run(host, maxlag):
    shape, x = CASES[3]
    full, got = host[shape], H.host_diag(x, maxlag=maxlag)
    for f in ("rho", "rho_mean"):
        assert got[f].shape == (4, maxlag + 1)
        assert np.array_equal(got[f].view(np.uint64), full[f][:, :maxlag + 1].view(np.uint64))
    assert np.array_equal(got["rhat"], full["rhat"])
    for tag in ("", "_mean"):
        for d in range(4):
            if full["window" + tag][d] <= maxlag:
                assert got["window" + tag][d] == full["window" + tag][d] and got["tau" + tag][d] == full["tau" + tag][d]
            else:                                                # Sokal's condition is not met within maxlag
                assert got["window" + tag][d] == maxlag
                assert got["tau" + tag][d] == (2.0 * np.cumsum(full["rho" + tag][d, :maxlag + 1]) - 1.0)[-1]
    if maxlag == 1:
        assert np.all(got["window"] == 1)


def test_host_build_refuses_what_the_library_refuses():
    L = H.build()
    x = np.zeros((4, 2, 2))
    args = lambda n, c, ml: (x.ctypes.data, n, 2, 2, c, ml) + (None,) * 8 + (1,)   # noqa: E731
    assert L.dgh_chain(*args(1, 5.0, -1)) == -1 and L.dgh_chain(*args(4, 0.0, -1)) == -1 and L.dgh_chain(*args(4, 5.0, 4)) == -1
    assert L.dgh_chain(*args(16385, 5.0, -1)) == -2


def test_interface_declared_bound_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    for name in ("gf_chain_diagnostics_device", "gf_chain_diagnostics", "gf_sampler_diagnostics"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.GfDiagSpec) == 16 and C.sizeof(_lib.GfDiagOut) == 64
    assert [f for f, _ in _lib.GfDiagOut._fields_] == ["tau", "tau_mean", "rhat", "window", "window_mean", "nexcluded", "rho", "rho_mean"]


def test_sokal_window_states_integrated_times_rule():
    rng = np.random.default_rng(3)
    for n, phi in ((50, 0.0), (400, 0.5), (2000, 0.9), (300, 0.99)):
        e = rng.standard_normal(n)
        x = np.empty(n)
        x[0] = e[0]
        for i in range(1, n):
            x[i] = phi * x[i - 1] + e[i]
        for c in (1, 5, 10):
            rho = mcmc_utils._autocorr_1d(x)
            taus = 2.0 * np.cumsum(rho) - 1.0
            m = np.arange(len(taus)) < c * taus                     # integrated_time's lines before the rule was factored out
            window = int(np.argmin(m)) if not m.all() else len(taus) - 1
            assert dg.sokal_window(taus, c) == window
            assert mcmc_utils.integrated_time(x, c=c, tol=0)[0] == taus[window]
    assert dg.sokal_window(np.full(7, 100.0), 5) == 6               # never met: the last lag
    with pytest.raises(mcmc_utils.AutocorrError):
        mcmc_utils.integrated_time(x, c=5, tol=50)


def test_chain_diagnostics_object_round_trips(tmp_path):
    o = H.host_diag(CASES[2][1])
    r = dg.ChainDiagnostics(nsteps=65, nwalkers=8, c=5.0, **o)
    assert np.array_equal(r.ess, 8 * 65 / o["tau"])
    assert r.converged(1) and not r.converged(50)
    assert not dg.ChainDiagnostics(nsteps=65, nwalkers=8, c=5.0, **dict(o, tau=np.array([1., np.nan, 1., 1.]))).converged(1)
    p = str(tmp_path / "d.npz")
    r.save(p)
    z = np.load(p)
    want = r.as_arrays()
    assert set(z.files) == set(want) and {"tau", "window", "tau_mean", "window_mean", "rhat", "nexcluded", "ess", "rho", "rho_mean"} <= set(z.files)
    for k in want:
        assert np.array_equal(z[k], want[k], equal_nan=True) and z[k].dtype == np.asarray(want[k]).dtype, k
    with pytest.raises(ValueError, match="thin"):
        dg.run_diag_call(None, "x", 1, 16385, 4, 2)


def test_scan_diagnostics_needs_datadir(capsys):
    with pytest.raises(SystemExit) as e:
        scan.main(["--config", "C4", "--diagnostics"])
    assert e.value.code == 2 and "--diagnostics needs --datadir" in capsys.readouterr().err
