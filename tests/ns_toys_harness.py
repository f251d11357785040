"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_ns_toys.hpp (tests/ns_toys/ns_toys_host.cpp, g++
with contraction off): the evidence of a nested run's points under other Gaussian measurements, summed along gf_nested_post.hpp's tree.

Used by tests/test_evidence_realisations_host.py (CPU) and tests/test_gpu_evidence_realisations.py.

The bit-for-bit comparisons keep every Gaussian exponent outside the subnormal band (-745.14, -708.39): there log(exp(.)) goes through
exp and log, which the host's and the device's libraries may round differently in the last place; above the band it is the identity
and below it -inf on both.  `host_evidence` asserts it for every (point, realisation) it is given, the run's own measurement included."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import toys_harness as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ns_toys", "ns_toys_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]
LANES, LEAF = 256, 4096
U = 2.0 ** -53

_CACHE = {}
same_bits = TH.same_bits


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="nthost")
    out = os.path.join(d, "libnthost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.nth_evidence.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.nth_evidence.restype = None
    L.nth_gauss.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]
    L.nth_gauss.restype = None
    L.nth_x.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int32]
    L.nth_x.restype = C.c_double
    L.nth_tree_sum.argtypes = [C.c_void_p, C.c_int64]
    L.nth_tree_sum.restype = C.c_double
    L.nth_ess.argtypes = [C.c_double, C.c_double, C.c_int64]
    L.nth_ess.restype = C.c_double
    _CACHE[out_dir] = L
    return L


def consts(bf, smearing):
    """[T][5] = {m[3], mh, k}: the host build's view of measurements bf [T][3] of smearing [T] (or one value), the constants by the
    library's own host function (toys_harness.gauss_consts: the bits a model of that smearing holds)."""
    bf = np.asarray(bf, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(bf), 5))
    out[:, :3] = bf
    for t, sm in enumerate(np.broadcast_to(np.asarray(smearing, dtype=np.float64), (len(bf),))):
        out[t, 3], out[t, 4] = TH.gauss_consts(sm)
    return out


def band_free(fr, meas):
    """No Gaussian exponent of (fr [n][3], meas [T][5]) inside the subnormal band, a margin of 1 on either side (toys_harness.band_free)."""
    fr = np.asarray(fr, dtype=np.float64)
    fr = fr[np.isfinite(fr).all(axis=1)]
    return TH.band_free(fr, np.concatenate([meas, np.zeros((len(meas), 1))], axis=1))


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def host_evidence(lnw, fr, status, own, meas, offset, want_x=False, check_band=True):
    """The host build's evidence of one run (lnw [n], fr [n][3], status [n]; own [5] its measurement, meas [T][5]) under every
    realisation: dict(m, s, s2, ess, kept [T], x [T][n] with want_x)."""
    lnw, fr, status, own, meas = _c(lnw), _c(fr).reshape(-1, 3), _c(status, np.int32), _c(own).reshape(5), _c(meas).reshape(-1, 5)
    n, T = len(lnw), len(meas)
    if check_band:
        assert band_free(fr, np.concatenate([own[None], meas])), "a Gaussian exponent lies in the subnormal band"
    out = dict(m=np.empty(T), s=np.empty(T), s2=np.empty(T), ess=np.empty(T), kept=np.empty(T, np.int64))
    x = np.empty((T, n)) if want_x else None
    build().nth_evidence(lnw.ctypes.data, fr.ctypes.data, status.ctypes.data, n, own.ctypes.data, float(offset), meas.ctypes.data, T,
                         *[out[k].ctypes.data for k in ("m", "s", "s2", "ess", "kept")], x.ctypes.data if want_x else None)
    if want_x:
        out["x"] = x
    return out


def host_gauss(fr, meas, offset):
    fr, meas = _c(fr).reshape(-1, 3), _c(meas).reshape(5)
    out = np.empty(len(fr))
    build().nth_gauss(fr.ctypes.data, len(fr), meas.ctypes.data, float(offset), out.ctypes.data)
    return out


def host_tree_sum(e):
    e = _c(e)
    return float(build().nth_tree_sum(e.ctypes.data, len(e)))


def tree_depth(n):
    """additions on the longest path of the tree sum of n terms (gf_nested_post.hpp's count)"""
    leaves = max(1, -(-n // LEAF))
    return 16 + 6 + 3 + -(-leaves // LANES) + 6 + 3
