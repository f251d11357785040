"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_temper.hpp (tests/temper/temper_host.cpp, g++ with
contraction off) and numpy restatements of what the tempered sampler defines for itself: the walker's scalar, the draw
and the accept rule of a replica-exchange round.

Used by tests/test_temper_host.py (CPU) and tests/test_gpu_temper.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "temper", "temper_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="tphost")
    out = os.path.join(d, "libtphost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.tph_temper.argtypes, L.tph_temper.restype = [C.c_double] * 3, C.c_double
    L.tph_swap_step_word.argtypes, L.tph_swap_step_word.restype = [C.c_uint64, C.c_int], C.c_uint64
    L.tph_swap_walker_word.argtypes, L.tph_swap_walker_word.restype = [C.c_uint64, C.c_int, C.c_int], C.c_uint64
    L.tph_stretch_step_word.argtypes, L.tph_stretch_step_word.restype = [C.c_uint64, C.c_int], C.c_uint64
    L.tph_swap_uniform.argtypes, L.tph_swap_uniform.restype = [C.c_uint64] * 3, C.c_double
    L.tph_swap_log_ratio.argtypes, L.tph_swap_log_ratio.restype = [C.c_double] * 4, C.c_double
    L.tph_max_temps.restype = C.c_int
    L.tph_series.argtypes, L.tph_series.restype = [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_void_p], None
    _CACHE[out_dir] = L
    return L


def host_series(lnl, d_up, d_dn):
    """lnl (nsteps, nwalkers) -> (nsteps, 5) by the host build."""
    lnl = np.ascontiguousarray(lnl, dtype=np.float64)
    out = np.empty((lnl.shape[0], 5))
    build().tph_series(lnl.ctypes.data, lnl.shape[0], lnl.shape[1], float(d_up), float(d_dn), out.ctypes.data)
    return out


# ---- the definitions, restated ---------------------------------------------------------------------------------------------------------

SWAP_BIT, RUNG_SHIFT = 1 << 63, 56


def temper(lp, lnl, beta):
    """T = lp + beta * lnl, the product rounded, then the sum; beta == 0: lp, no product."""
    lp, lnl = np.asarray(lp, dtype=np.float64), np.asarray(lnl, dtype=np.float64)
    if beta == 0.0:
        return lp.copy()
    with np.errstate(invalid="ignore"):
        return lp + np.float64(beta) * lnl


def fma(x, y, z):
    """x * y + z rounded once: what T must NOT be"""
    from fractions import Fraction
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def swap_step_word(rnd, t):
    return SWAP_BIT | (t << RUNG_SHIFT) | (rnd & ((1 << RUNG_SHIFT) - 1))


def swap_uniform(oracle, seed, gsid, nwalkers, w, rnd, t):
    """The round's uniform of walker w of the pair (t, t + 1) of the group whose rung-0 chain has stream id gsid."""
    g = (gsid * nwalkers + w) & 0xFFFFFFFFFFFFFFFF
    s = swap_step_word(rnd, t)
    r = oracle.philox4x32_10((g & 0xffffffff, g >> 32, s & 0xffffffff, s >> 32), (seed & 0xffffffff, seed >> 32))
    return (r[0] + 0.5) / 4294967296.0


def swap_round(oracle, seed, rnd, betas, pos, T, lp, lnl, counts, stream_ids=None):
    """One round in place on pos (nchains, nwalkers, ndim) and T (nchains, nwalkers), given (lp, lnl) of the current walkers; counts
    (nchains, 2) += pairs proposed / accepted at the entry of the pair's colder chain.  nchains = ngroups * len(betas)."""
    K = len(betas)
    nchains, nw = T.shape
    for g in range(nchains // K):
        gsid = g * K if stream_ids is None else int(stream_ids[g * K])
        for t in range(rnd % 2, K - 1, 2):
            a, b = g * K + t, g * K + t + 1
            for w in range(nw):
                if not (T[a, w] > -np.inf) or not (T[b, w] > -np.inf):
                    continue
                counts[a, 0] += 1
                u = swap_uniform(oracle, seed, gsid, nw, w, rnd, t)
                with np.errstate(invalid="ignore"):
                    ok = np.log(u) < (np.float64(betas[t]) - np.float64(betas[t + 1])) * (lnl[b, w] - lnl[a, w])
                if not ok:
                    continue
                counts[a, 1] += 1
                pos[[a, b], w] = pos[[b, a], w]
                T[a, w] = temper(lp[b, w], lnl[b, w], betas[t])
                T[b, w] = temper(lp[a, w], lnl[a, w], betas[t + 1])
