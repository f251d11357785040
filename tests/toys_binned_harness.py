"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_toys_binned.hpp (tests/toys/toys_binned_host.cpp,
g++ with contraction off) and the crafted seed sets both the CPU and the GPU tests of the energy-resolved realisation ensembles use
(DESIGN.md 6l).  The selection restated with np.lexsort, the Gaussian's constants and the comparison of bits are toys_harness's.

Used by tests/test_binned_realisations_host.py (CPU) and tests/test_gpu_binned_realisations.py.

As in toys_harness, the crafted inputs keep every bin's Gaussian exponent outside the subnormal band (-745.14, -708.39), where the
host's and the device's exp and log may round differently (`band_free` checks a case, bin by bin); the band is covered on the device
alone: the scores against Model.lnprob."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from toys_harness import FLAGS, NON_UNITARY, gauss_consts, lexsort_select, same_bits  # noqa: F401  (re-exported to the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "toys", "toys_binned_host.cpp")

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="toybhost")
    out = os.path.join(d, "libtoybhost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.toybh_scores.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.toybh_scores.restype = None
    L.toybh_select.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 3
    _CACHE[out_dir] = L
    return L


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def table(meas, sigma):
    """[nb][5][T] = {m[3], mh, k} of every bin of every realisation: the host build's (and the device's) view.  meas [T][nb][3], sigma
    [nb] or [T][nb]."""
    meas = np.asarray(meas, dtype=np.float64)
    T, nb = meas.shape[:2]
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (T, nb))
    tab = np.empty((nb, 5, T))
    tab[:, :3, :] = meas.transpose(1, 2, 0)
    for t in range(T):
        for k in range(nb):
            tab[k, 3, t], tab[k, 4, t] = gauss_consts(sg[t, k])
    return tab


def host_scores(lp, frb, status, tab, offset, L=None):
    L = L or build()
    lp, frb, status, tab = _c(lp), _c(frb), _c(status, np.int32), _c(tab)
    nb, _, T = tab.shape
    assert frb.shape == (len(lp), nb, 3)
    out = np.empty((T, len(lp)))
    L.toybh_scores(lp.ctypes.data, frb.ctypes.data, status.ctypes.data, len(lp), nb, tab.ctypes.data, T, float(offset), out.ctypes.data)
    return out


def host_select(lp, frb, status, tab, offset, K, L=None):
    """The host build's selection: (index [T][K], score [T][K], count [T])"""
    L = L or build()
    lp, frb, status, tab = _c(lp), _c(frb), _c(status, np.int32), _c(tab)
    nb, _, T = tab.shape
    assert frb.shape == (len(lp), nb, 3)
    index, score, count = np.empty((T, K), np.int32), np.empty((T, K)), np.empty(T, np.int32)
    rc = L.toybh_select(lp.ctypes.data, frb.ctypes.data, status.ctypes.data, len(lp), nb, tab.ctypes.data, T, float(offset), int(K),
                        index.ctypes.data, score.ctypes.data, count.ctypes.data)
    assert rc == 0, rc
    return index, score, count


def exponents(frb, tab):
    """the Gaussian exponent of every (realisation, seed, bin): [T][M][nb] (plain numpy: for the conditions on a case, not for bits)"""
    frb = np.asarray(frb, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = frb[None] - tab[:, :3, :].transpose(2, 0, 1)[:, None]           # [T][M][nb][3]
        return tab[:, 3, :].T[:, None] * np.sum(d * d, axis=-1) + tab[:, 4, :].T[:, None]


def band_free(frb, tab):
    """No Gaussian exponent of any bin of the case inside the subnormal band (toys_harness.band_free's rule and margin, per bin)."""
    e = exponents(frb, tab)
    return not np.any((e > -746.5) & (e < -707.5))


def crafted(nseed, ntoys, nb, seed, kind="mixed", smearing=0.05, offset=-320.0, per_toy_sigma=False):
    """A seed set and its realisations: (lp, frb [nseed][nb][3], status, meas [ntoys][nb][3], sigma ([nb], or [ntoys][nb]), offset).
    kind: "mixed"   compositions near (1/3, 1/3, 1/3) in every bin, a fifth of the rows duplicated (ties between different indices), some lp
                    -inf (outside the box), some NaN (in lp, and in ONE bin of fr), some non-unitary, some with ONE bin far enough for that
                    bin's Gaussian to be -inf -- the underflow wall, which makes the whole score -inf
          "neginf"  every score -inf
          "ties"    every row the same"""
    rng = np.random.default_rng(seed)
    centre = np.array([1 / 3, 1 / 3, 1 / 3])
    meas = centre + smearing * rng.standard_normal((ntoys, nb, 3))
    sigma = smearing * (1.0 + 0.25 * rng.random((ntoys, nb) if per_toy_sigma else nb))
    frb = centre + 2.0 * smearing * rng.standard_normal((nseed, nb, 3))
    lp = rng.normal(-5.0, 3.0, nseed)
    status = np.zeros(nseed, np.int32)
    if kind == "ties":
        frb[:], lp[:] = frb[0], lp[0]
    else:
        dup = rng.random(nseed) < 0.2
        src = rng.integers(0, nseed, nseed)
        frb[dup], lp[dup] = frb[src[dup]], lp[src[dup]]
        pick = rng.random(nseed)
        bin_of = rng.integers(0, nb, nseed)
        lp[pick < 0.05] = -np.inf
        status[pick < 0.05] = 1
        lp[(pick >= 0.05) & (pick < 0.08)] = np.nan
        rows = np.flatnonzero((pick >= 0.08) & (pick < 0.11))
        frb[rows, bin_of[rows], 1] = np.nan                               # NaN in a single bin
        status[(pick >= 0.11) & (pick < 0.2)] = NON_UNITARY
        rows = np.flatnonzero((pick >= 0.2) & (pick < 0.25))
        frb[rows, bin_of[rows]] += 2.0                                    # that bin's exponent is below -745.14 by far: its term is -inf
        if kind == "neginf":
            third = np.arange(nseed) % 3
            lp[third == 0] = -np.inf
            status[third == 1] = NON_UNITARY
            lp[third == 2] = np.nan
    assert band_free(frb[np.isfinite(frb).all(axis=(1, 2))], table(meas, sigma))
    return lp, frb, status, meas, sigma, offset
