"""The shortest interval around the mode without a device: the host build of csrc/gf_interval.hpp (tests/interval/interval_host.cpp)
and the numpy restatement `intervals.interval_host` held to the reference's own results (tests/golden/golden_interval.npz, written by
tests/golden/make_golden_interval.py from golemflavor/misc.py:174-213) exactly as numbers, to each other on seeded random columns,
and the interface around them.

A case the reference raised on carries the exception's name: IndexError (its walk indexed s[n]) is status 3, anything else (raised
before the walk: ValueError for a NaN bin count or an empty histogram, OverflowError for an infinite one) is status 2."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import interval_harness as H
from golemflavor_amd import _lib, intervals as iv, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = H.goldens()
IDS = [g[0] for g in GOLDENS]
ENTRY_POINTS = ("gf_sort_columns_device", "gf_column_intervals_device", "gf_column_intervals", "gf_sampler_intervals",
                "gf_sampler_element_intervals", "gf_nested_intervals")


def test_goldens_hold_every_case_of_the_issue():
    assert IDS == ["normal", "uniform", "bimodal", "rounded", "zeros_uniform", "negative", "mixed", "magnitudes", "constant", "n1", "n2", "n3"]
    for name, x, pct, low, center, up, status, nbins in GOLDENS:
        assert len(x) <= 4096 and list(pct) == [68., 90., 99., 100.]
        assert np.all(np.isfinite(low[status == 0])) and np.all(np.isnan(low[status != 0]))
    by = {g[0]: g for g in GOLDENS}
    assert list(by["constant"][6]) == [2] * 4 and list(by["n1"][6]) == [2] * 4 and list(by["n2"][6]) == [3] * 4 and list(by["n3"][6]) == [3] * 4
    assert all(list(by[k][6]) == [0, 0, 0, 3] for k in IDS[:8])
    # the bimodal walk reaches the upper end and goes on downward; the zero block starts the window at index 0
    assert by["bimodal"][5][0] == by["bimodal"][1].max() and by["bimodal"][3][0] < 3. and by["zeros_uniform"][3][0] == 0.0


def _check(name, x, pct, low, center, up, status, nbins, got):
    assert np.array_equal(got["status"], status), (name, got["status"], status)
    assert H.same_numbers(got["low"], low) and H.same_numbers(got["up"], up), (name, got["low"], low, got["up"], up)
    if np.any(status == 0):
        assert got["center"] == center[status == 0][0], (name, got["center"], center)
    assert got["nbins"] == (-1 if np.isnan(nbins) else int(nbins)), (name, got["nbins"], nbins)
    assert got["nunique"] == len(np.unique(x)), name


@pytest.mark.parametrize("g", GOLDENS, ids=IDS)
def test_host_build_equals_the_reference(g):
    _check(*g, H.host_column(g[1], g[2]))
    # one walk serves every percentile: any order and any subset give the same numbers
    rev = H.host_column(g[1], g[2][::-1])
    assert H.same_numbers(rev["low"][::-1], g[3]) and H.same_numbers(rev["up"][::-1], g[5]) and np.array_equal(rev["status"][::-1], g[6])


@pytest.mark.parametrize("g", GOLDENS, ids=IDS)
def test_numpy_restatement_equals_the_reference(g):
    name, x, pct = g[:3]
    r = [iv.interval_host(x, p) for p in pct]
    got = dict(low=np.array([q[0] for q in r]), up=np.array([q[2] for q in r]), status=np.array([q[3] for q in r], np.int32),
               center=r[0][1], nbins=iv.most_likely_host(x)[1], nunique=iv.nunique_host(x))
    _check(*g, got)
    if g[6][0] == 0:
        assert iv.most_likely_host(x)[0] == g[4][0]


def test_host_build_equals_the_restatement_on_200_random_columns():
    pct = (68., 90., 100.)
    nties = 0
    for seed in range(200):
        x = H.random_column(seed)
        want = iv.rows_intervals_host(x[:, None], pct)
        got = H.host_column(x, pct)
        nties += got["nunique"] < len(x)
        H.assert_same_result({k: (np.asarray(v)[None] if k in ("low", "up", "status") else np.asarray([v])) for k, v in got.items()},
                             {k: want[k] for k in got}, "seed %d n %d" % (seed, len(x)))
    assert nties >= 50


def test_status_rules_of_both_statements():
    for x, want in (([1., np.nan, 2., 3.], 1), ([1., np.inf, 2., 3.], 1), ([2.] * 7, 2), ([0., 1., 1., 1., 1., 1., 1., 5.], 2), ([3.], 2)):
        assert iv.interval_host(x, 68.)[3] == want, x
        h = H.host_column(x, (68., 90.))
        assert list(h["status"]) == [want] * 2 and np.all(np.isnan(h["low"])) and np.all(np.isnan(h["up"])), x
        assert h["nunique"] == iv.nunique_host(x) and (want != 1 or (h["nunique"] == -1 and h["nbins"] == -1))
    # a bin count above 2^20: a far outlier next to a narrow bulk
    x = np.concatenate([np.linspace(0., 1e-3, 999), [1e6]])
    assert iv.interval_host(x, 68.)[3] == 4 and list(H.host_column(x, (68.,))["status"]) == [4]
    assert H.host_column(x, (68.,))["nbins"] == iv.most_likely_host(x)[1] > iv.GF_INTERVAL_MAX_BINS
    # status 3 keeps the centre
    lo, c, up, st = iv.interval_host(np.arange(50.), 100.)
    assert st == 3 and np.isfinite(c) and H.host_column(np.arange(50.), (100.,))["center"] == c


def test_host_build_refuses_what_the_library_refuses():
    L = H.build()
    x, p = np.zeros(4), np.array([68., 0., 101.])
    o = [np.zeros(8) for _ in range(6)]
    args = lambda n, pp, k: (x.ctypes.data, n, pp, k) + tuple(a.ctypes.data for a in o)   # noqa: E731
    assert L.ivh_column(*args(0, p.ctypes.data, 1)) == -1 and L.ivh_column(*args(4, p.ctypes.data, 0)) == -1
    assert L.ivh_column(*args(4, p.ctypes.data, 9)) == -1 and L.ivh_column(*args(4, p.ctypes.data, 2)) == -1
    assert L.ivh_column(*args(4, p[2:].ctypes.data, 1)) == -1
    for bad in ((), (0.,), (101.,), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            iv._percentiles(bad)


def test_interface_declared_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
    assert re.search(r"#define\s+GF_INTERVAL_MAX_BINS\s+\(1 << 20\)", hdr) and _lib.GF_INTERVAL_MAX_BINS == 1 << 20
    assert re.search(r"#define\s+GF_INTERVAL_MAX_PERCENTILES\s+8\b", hdr) and _lib.GF_INTERVAL_MAX_PERCENTILES == 8


def test_library_exports_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


def test_binding_covers_the_entry_points():
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.GfIntervalSpec) == 16 and C.sizeof(_lib.GfIntervalOut) == 48
    assert [f for f, _ in _lib.GfIntervalOut._fields_] == ["low", "up", "status", "center", "nbins", "nunique"]
    assert _lib.lib().gf_nested_intervals.argtypes == _lib.SIGNATURES["gf_nested_intervals"][1]


def test_scan_intervals_needs_datadir(capsys):
    with pytest.raises(SystemExit) as e:
        scan.main(["--config", "C4", "--intervals"])
    assert e.value.code == 2 and "--intervals needs --datadir" in capsys.readouterr().err
