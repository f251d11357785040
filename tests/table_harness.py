"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_table.hpp (tests/table/table_host.cpp, g++ with
contraction off), which both the CPU and the GPU tests of the tabulated flavour-plane likelihood hold the package to.

Used by tests/test_table_host.py (CPU) and tests/test_gpu_table.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "table", "table_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="tabhost")
    out = os.path.join(d, "libtabhost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.tabh_node_count.argtypes = [C.c_int]
    L.tabh_node_count.restype = C.c_int64
    L.tabh_node_at.argtypes = [C.c_int] * 3
    L.tabh_node_at.restype = C.c_int64
    L.tabh_locate.argtypes = [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 7
    L.tabh_locate.restype = None
    L.tabh_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.tabh_lookup.restype = None
    _CACHE[out_dir] = L
    return L


def _fr(fr):
    fr = np.ascontiguousarray(np.atleast_2d(np.asarray(fr, dtype=np.float64)))
    assert fr.ndim == 2 and fr.shape[1] == 3
    return fr


def host_lookup(values, nside, fr, L=None):
    """the header's ln L of every composition fr [n][3]"""
    L = L or build()
    values = np.ascontiguousarray(values, dtype=np.float64)
    assert values.shape == (int(L.tabh_node_count(int(nside))),)
    fr = _fr(fr)
    out = np.empty(len(fr))
    L.tabh_lookup(values.ctypes.data, int(nside), fr.ctypes.data, len(fr), out.ctypes.data)
    return out


def host_locate(nside, fr, L=None):
    """the header's own cell of every composition: dict(i, j, fu, fv, up, ok, at [n][3]); rows with ok == 0 (NaN) hold zeros"""
    L = L or build()
    fr = _fr(fr)
    n = len(fr)
    r = dict(i=np.zeros(n, np.int32), j=np.zeros(n, np.int32), fu=np.zeros(n), fv=np.zeros(n), up=np.zeros(n, np.int32),
             ok=np.zeros(n, np.int32), at=np.zeros((n, 3), np.int64))
    L.tabh_locate(fr.ctypes.data, n, int(nside), *(r[k].ctypes.data for k in ("i", "j", "fu", "fv", "up", "ok", "at")))
    return r


def same_bits(a, b):
    """equal as bit patterns (NaN equals NaN of the same payload, -0.0 differs from 0.0)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_values(a, b):
    """same_bits, except that any NaN equals any NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))
