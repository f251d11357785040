"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_toys.hpp (tests/toys/toys_host.cpp, g++ with
contraction off), the crafted seed sets both the CPU and the GPU tests of the realisation ensembles use, and the selection restated
with np.lexsort.

Used by tests/test_realisations_host.py (CPU) and tests/test_gpu_realisations.py.

The crafted inputs keep every Gaussian exponent outside the subnormal band (-745.14, -708.39): there log(exp(.)) goes through exp and
log, which the host's and the device's libraries may round differently in the last place; above the band it is the identity and below
it -inf on both (`band_free` checks a case).  The band itself is covered on the device alone: the scores against Model.lnprob."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from golemflavor_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "toys", "toys_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]
NON_UNITARY = _lib.GF_ST_NON_UNITARY

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="toyhost")
    out = os.path.join(d, "libtoyhost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.toyh_scores.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.toyh_scores.restype = None
    L.toyh_select.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
    _CACHE[out_dir] = L
    return L


def gauss_consts(smearing):
    """(mh, k) of a smearing by the library's own host function (gf_internal.h; not part of the public header): the bits a model of
    that smearing holds.  Needs no device."""
    fn = _lib.lib().gf_internal_gauss_consts
    fn.restype, fn.argtypes = None, [C.c_double] + [_lib._dp] * 4
    v = [C.c_double() for _ in range(4)]
    fn(float(smearing), *[C.byref(x) for x in v])
    return v[2].value, v[3].value


def measurements(bf, smearing, offset):
    """[ntoys][6] = {m[3], mh, k, offset}: the host build's view of the realisations"""
    bf = np.asarray(bf, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(bf), 6))
    out[:, :3] = bf
    for t, sm in enumerate(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (len(bf),))):
        out[t, 3], out[t, 4] = gauss_consts(sm)
    out[:, 5] = offset
    return out


def host_scores(lp, fr, status, meas, L=None):
    L = L or build()
    lp, fr, status, meas = _c(lp), _c(fr), _c(status, np.int32), _c(meas)
    out = np.empty((len(meas), len(lp)))
    L.toyh_scores(lp.ctypes.data, fr.ctypes.data, status.ctypes.data, len(lp), meas.ctypes.data, len(meas), out.ctypes.data)
    return out


def host_select(lp, fr, status, meas, K, L=None):
    """The host build's selection: (index [ntoys][K], score [ntoys][K], count [ntoys])"""
    L = L or build()
    lp, fr, status, meas = _c(lp), _c(fr), _c(status, np.int32), _c(meas)
    T = len(meas)
    index, score, count = np.empty((T, K), np.int32), np.empty((T, K)), np.empty(T, np.int32)
    rc = L.toyh_select(lp.ctypes.data, fr.ctypes.data, status.ctypes.data, len(lp), meas.ctypes.data, T, int(K), index.ctypes.data,
                       score.ctypes.data, count.ctypes.data)
    assert rc == 0, rc
    return index, score, count


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def lexsort_select(scores, K):
    """The definition: per realisation the K first of np.lexsort((index, -score)) whose score is above -inf; -1 / -inf behind them."""
    scores = np.asarray(scores, dtype=np.float64)
    T, M = scores.shape
    index, score, count = np.full((T, K), -1, np.int32), np.full((T, K), -np.inf), np.zeros(T, np.int32)
    for t in range(T):
        order = np.lexsort((np.arange(M), -scores[t]))
        order = order[scores[t][order] > -np.inf][:K]
        count[t] = len(order)
        index[t, :len(order)] = order
        score[t, :len(order)] = scores[t][order]
    return index, score, count


def band_free(fr, meas):
    """No Gaussian exponent of the case inside the subnormal band (a margin of 1 on either side)."""
    fr = np.asarray(fr, dtype=np.float64)
    ok = True
    with np.errstate(invalid="ignore", over="ignore"):
        for q in meas:
            e = q[3] * np.sum((fr - q[:3]) ** 2, axis=1) + q[4]
            ok = ok and not np.any((e > -746.5) & (e < -707.5))
    return ok


def crafted(nseed, ntoys, seed, kind="mixed", smearing=0.05, offset=-320.0):
    """A seed set and its realisations: (lp, fr, status, bf, smearing [ntoys], offset).
    kind: "mixed"   seeded compositions near (1/3, 1/3, 1/3), a fifth of the rows duplicated (ties between different indices), some lp
                    -inf (outside the box), some NaN (in lp and in fr), some non-unitary, some far enough for the Gaussian to be -inf
          "neginf"  every score -inf (lp -inf, non-unitary or NaN)
          "ties"    every row the same"""
    rng = np.random.default_rng(seed)
    bf = np.array([1 / 3, 1 / 3, 1 / 3]) + smearing * rng.standard_normal((ntoys, 3))
    sm = np.full(ntoys, smearing)
    fr = np.array([1 / 3, 1 / 3, 1 / 3]) + 2.0 * smearing * rng.standard_normal((nseed, 3))
    lp = rng.normal(-5.0, 3.0, nseed)
    status = np.zeros(nseed, np.int32)
    if kind == "ties":
        fr[:], lp[:] = fr[0], lp[0]
    else:
        dup = rng.random(nseed) < 0.2
        src = rng.integers(0, nseed, nseed)
        fr[dup], lp[dup] = fr[src[dup]], lp[src[dup]]
        pick = rng.random(nseed)
        lp[pick < 0.05] = -np.inf
        status[pick < 0.05] = 1
        lp[(pick >= 0.05) & (pick < 0.08)] = np.nan
        fr[(pick >= 0.08) & (pick < 0.11), 1] = np.nan
        status[(pick >= 0.11) & (pick < 0.2)] = NON_UNITARY
        fr[(pick >= 0.2) & (pick < 0.25)] += 2.0                          # exponent below -745.14 by far: the Gaussian is -inf
        if kind == "neginf":
            third = np.arange(nseed) % 3
            lp[third == 0] = -np.inf
            status[third == 1] = NON_UNITARY
            lp[third == 2] = np.nan
    meas = measurements(bf, sm, offset)
    assert band_free(fr[np.isfinite(fr).all(axis=1)], meas)
    return lp, fr, status, bf, sm, offset


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64:
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))
