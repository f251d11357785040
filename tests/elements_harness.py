"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_elements.hpp and gf_elements_exact.hpp
(tests/elements/elements_host.cpp,
g++ with contraction off), the seeded input both the CPU and the GPU element tests use, and the oracle's side of the comparison.

Used by tests/test_elements_host.py (CPU) and tests/test_gpu_elements.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "elements", "elements_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-mfma", "-fPIC", "-shared", "-ffp-contract=off"]

# The absolute tolerance of every modulus and fraction against the oracle: four times the maximum measured over mixing_input(SEED,
# NRAND) and source_input(SEED, NRAND) with the host build (profiles/elements/README.txt has the figure and the row that attains it).
MEASURED_MAX = 2.2205510052351563e-15
TOL = 4.0 * MEASURED_MAX
SEED = 20260117
NRAND = 1 << 22
F32_EXCLUDED_CAP = 1e-3

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    from golemflavor_amd.elements import GfElementPlan
    d = out_dir or tempfile.mkdtemp(prefix="elhost")
    out = os.path.join(d, "libelementshost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.elh_plan_width.argtypes = [C.POINTER(GfElementPlan), C.c_int]
    L.elh_rows.argtypes = [C.POINTER(GfElementPlan), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    _CACHE[out_dir] = L
    return L


def host_rows(L, plan, rows):
    """The host build's element rows of `rows` (n, width_in)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    w = L.elh_plan_width(C.byref(plan), rows.shape[1])
    assert w > 0
    out = np.empty((rows.shape[0], w))
    assert L.elh_rows(C.byref(plan), rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data) == 0
    return out


def _edges01():
    """0, 1, 2^-k and 1 - 2^-k for k = 1 .. 52"""
    k = np.arange(1, 53, dtype=np.float64)
    return np.concatenate([[0.0, 1.0], 2.0 ** -k, 1.0 - 2.0 ** -k])


def mixing_edge_rows(seed=SEED):
    """The explicit edge sets of (s12^2, c13^4, s23^2, delta): every edge value of each of the three with the others random, with the
    others at their own corners, and all three at an edge at once (a seeded sample of the cube of edges); delta at the multiples
    of pi/2 and random."""
    rng = np.random.default_rng(seed + 1)
    e = _edges01()
    quarter = np.arange(5) * (np.pi / 2)
    out = []
    for col in range(3):
        for d in list(quarter) + [None] * 3:
            r = rng.uniform(0, 1, size=(len(e), 4))
            r[:, 3] = rng.uniform(0, 2 * np.pi, len(e)) if d is None else d
            r[:, col] = e
            out.append(r)
        for corner in range(4):                                  # the other two at 0 / 1
            others = [c for c in range(3) if c != col]
            r = np.zeros((len(e), 4))
            r[:, col] = e
            r[:, others[0]] = corner & 1
            r[:, others[1]] = corner >> 1
            r[:, 3] = quarter[(np.arange(len(e)) + corner) % 5]
            out.append(r)
    n = 8000
    r = np.column_stack([rng.choice(e, n), rng.choice(e, n), rng.choice(e, n), rng.choice(quarter, n)])
    r[n // 2:, 3] = rng.uniform(0, 2 * np.pi, n - n // 2)
    out.append(r)
    return np.concatenate(out)


def mixing_input(seed=SEED, nrand=NRAND):
    """Edge rows first, then `nrand` rows uniform over the box [0, 1]^3 x [0, 2 pi]."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0, 1, size=(nrand, 4))
    r[:, 3] *= 2 * np.pi
    return np.concatenate([mixing_edge_rows(seed), r])


def source_edge_rows(seed=SEED):
    rng = np.random.default_rng(seed + 2)
    e = _edges01()
    c = np.concatenate([e, -e, 2 * e - 1])                       # cos 2psi over [-1, 1]
    a = np.column_stack([e, rng.uniform(-1, 1, len(e))])
    b = np.column_stack([rng.uniform(0, 1, len(c)), c])
    g = np.column_stack([np.repeat(e, len(c)), np.tile(c, len(e))])
    return np.concatenate([a, b, g])


def source_input(seed=SEED, nrand=NRAND):
    """Edge rows first, then `nrand` rows uniform over [0, 1] x [-1, 1]."""
    rng = np.random.default_rng(seed + 3)
    r = rng.uniform(0, 1, size=(nrand, 2))
    r[:, 1] = 2 * r[:, 1] - 1
    return np.concatenate([source_edge_rows(seed), r])


def oracle_absu(rows):
    """|U_ij| of every row (n, 4) -> (n, 9) np.longdouble: hypot of the long-double parts orc_angles_to_u_ldout hands back."""
    from oracle import oracle as O
    O.lib()
    L = C.CDLL(O.LIB_PATH)                                       # a handle of its own: integer addresses instead of typed pointers
    f = L.orc_angles_to_u_ldout
    f.argtypes = [C.c_void_p, C.c_void_p]
    f.restype = None
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = rows.shape[0]
    parts = np.zeros((n, 18), dtype=np.longdouble)
    a0, p0, sp = rows.ctypes.data, parts.ctypes.data, parts.strides[0]
    for i in range(n):
        f(a0 + 32 * i, p0 + sp * i)
    return np.hypot(parts[:, 0::2], parts[:, 1::2])


def oracle_fr(rows):
    """oracle.angles_to_fr of every row (n, 2) -> (n, 3)"""
    from oracle import oracle as O
    O.lib()
    L = C.CDLL(O.LIB_PATH)
    f = L.orc_angles_to_fr
    f.argtypes = [C.c_void_p, C.c_void_p]
    f.restype = None
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n = rows.shape[0]
    out = np.zeros((n, 3))
    a0, p0 = rows.ctypes.data, out.ctypes.data
    for i in range(n):
        f(a0 + 16 * i, p0 + 24 * i)
    return out


def f32_boundary_distance(v):
    """The distance of every value of `v` (np.longdouble, in [0, 1]) from the nearest float32 rounding boundary: a midpoint between
    neighbouring floats."""
    f = v.astype(np.float32)
    up = np.nextafter(f, np.float32(2)).astype(np.longdouble)
    dn = np.nextafter(f, np.float32(-1)).astype(np.longdouble)
    fl = f.astype(np.longdouble)
    return np.minimum(np.abs(v - (fl + up) / 2), np.abs(v - (fl + dn) / 2))


def check_moduli(got64, ref, label=""):
    """`got64` (round32 off) within TOL of the oracle's moduli `ref` (longdouble).  Returns (max error, its row)."""
    err = np.abs(got64.astype(np.longdouble) - ref)
    worst = int(np.argmax(err.max(axis=1)))
    print("%s moduli: max abs err %.3e at row %d" % (label, float(err.max()), worst))
    assert float(err.max()) <= TOL, (float(err.max()), worst)
    return float(err.max()), worst


def float32_steps(got32, ref, label=""):
    """The float32 column against np.float32 of the oracle's moduli: (near, steps) -- `near` marks the entries whose oracle value
    lies within TOL of a float32 rounding boundary, `steps` is the distance in float32 steps (0 = equal)."""
    g32 = got32.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), got32), "round32 output is not a float32 value"
    r32 = ref.astype(np.float32)
    near = f32_boundary_distance(ref) <= TOL
    steps = np.abs(g32.view(np.int32).astype(np.int64) - r32.view(np.int32).astype(np.int64))
    print("%s float32: %d of %d entries within TOL of a rounding boundary (%.2e); away from them %d differ; on them %d differ, %d by "
          "more than one step (largest oracle value among those %.3e)"
          % (label, near.sum(), near.size, near.mean(), (steps[~near] != 0).sum(), (steps[near] != 0).sum(), (steps[near] > 1).sum(),
             float(ref[near & (steps > 1)].max()) if (near & (steps > 1)).any() else 0.0))
    return near, steps
