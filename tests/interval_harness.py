"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_interval.hpp (tests/interval/interval_host.cpp,
g++ with contraction off), the reference's goldens (tests/golden/golden_interval.npz, written by tests/golden/make_golden_interval.py)
and the seeded columns and rows the CPU and the GPU interval tests share.

Used by tests/test_intervals_host.py (CPU) and tests/test_gpu_intervals.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "interval", "interval_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_interval.npz")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]

ST_OK, ST_NONFINITE, ST_NBINS, ST_INDEX, ST_TOO_MANY_BINS = range(5)

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="ivhost")
    out = os.path.join(d, "libintervalhost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.ivh_column.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    _CACHE[out_dir] = L
    return L


def host_column(x, percentiles, L=None):
    """The host build's result for one column: dict(low, up, status (npct,), center, nbins, nunique)."""
    L = L or build()
    x = np.ascontiguousarray(x, dtype=np.float64)
    p = np.ascontiguousarray(np.atleast_1d(percentiles), dtype=np.float64)
    low, up, st = np.full(len(p), np.nan), np.full(len(p), np.nan), np.full(len(p), -1, np.int32)
    center, nb, nu = np.full(1, np.nan), np.full(1, -9, np.int64), np.full(1, -9, np.int64)
    rc = L.ivh_column(x.ctypes.data, len(x), p.ctypes.data, len(p), low.ctypes.data, up.ctypes.data, st.ctypes.data, center.ctypes.data,
                      nb.ctypes.data, nu.ctypes.data)
    assert rc >= 0, rc
    return dict(low=low, up=up, status=st, center=center[0], nbins=int(nb[0]), nunique=int(nu[0]))


def goldens():
    """[(name, x, pct, low, center, up, status, nbins)]: the reference's results; status from the exception it raised (IndexError: the
    walk indexed s[n], 3; anything else was raised before the walk, 2)."""
    z = np.load(GOLDEN, allow_pickle=False)
    out = []
    for name in z["cases"]:
        name = str(name)
        exc = [str(e) for e in z[name + "_exc"]]
        status = np.array([ST_OK if not e else ST_INDEX if e == "IndexError" else ST_NBINS for e in exc], np.int32)
        out.append((name, z[name + "_x"], z[name + "_pct"], z[name + "_low"], z[name + "_center"], z[name + "_up"], status, float(z[name + "_nbins"])))
    return out


def same_numbers(a, b):
    """equal as numbers, NaN equal to NaN (+0.0 and -0.0 are the same number)"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def random_column(seed):
    """A seeded column, n in [4, 5000]; every third one rounded (ties, runs of duplicates), every fifth one skewed."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(4, 5001))
    x = rng.standard_normal(n) * 10. ** rng.integers(-3, 4) + rng.integers(-5, 6)
    if seed % 5 == 0:
        x = np.exp(x / np.abs(x).max() * 3.)
    if seed % 3 == 0:
        x = np.round(x, int(rng.integers(0, 3)))
    return x


def ar1_rows(n, width, nchains, seed):
    """(nchains, n, width) AR(1)-like rows: phi cycling over (0, 0.5, 0.9, 0.99) per column, every fourth column rounded to two
    decimals (ties), columns of different scales and offsets."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((nchains, n, width))
    phi = np.array([(0.0, 0.5, 0.9, 0.99)[c % 4] for c in range(width)])
    x = np.empty_like(e)
    x[:, 0] = e[:, 0]
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + np.sqrt(1 - phi * phi) * e[:, i]
    x = x * (10. ** (np.arange(width) % 5 - 2)) + (np.arange(width) - 3.)
    x[:, :, 3::4] = np.round(x[:, :, 3::4], 2)
    return np.ascontiguousarray(x)


def assert_same_result(got, want, label=""):
    """two dicts of low, up, status, center, nbins, nunique: equal as numbers"""
    for f in ("status", "nbins", "nunique", "center", "low", "up"):
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (label, f, g.shape, w.shape)
        assert same_numbers(g, w), "%s: %s differs at %s: %s != %s" % (
            label, f, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:3].tolist(), g[~((g == w) | ((g != g) & (w != w)))][:3], w[~((g == w) | ((g != g) & (w != w)))][:3])
