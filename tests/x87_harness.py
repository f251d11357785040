"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_x87.hpp (tests/x87/x87_host.cpp, g++ with
contraction off, as the header is meant to be read) and numpy faces of its entry points, plus the two test-only device accessors
that hand the same operations and the model's own chain inputs to it (gf_internal_x87_eval, gf_internal_bsm_tables).

Used by tests/test_x87_emulation.py (CPU), tests/test_gpu_x87_device.py, tests/test_gpu_fuzz.py and tests/test_gpu_sampler.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "x87", "x87_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-mfma", "-fPIC", "-shared", "-ffp-contract=off"]

OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "sqrt": 4, "sincos": 5, "asin": 6, "acos": 7, "hypot": 8, "pow10": 9, "angles_to_u": 10}
BINARY = ("add", "sub", "mul", "div", "hypot")
VALUES_OUT = {"sincos": 2, "angles_to_u": 18}          # pairs out per operand (else 1)
THRESHOLD = 1e-7                                       # fr.py:493-494

_CACHE = {}
_D = C.POINTER(C.c_double)


def build(out_dir=None, defines=()):
    """Compile the host build (optionally with -D defines) and return the loaded library, with every entry point typed."""
    key = (out_dir, tuple(defines))
    if key in _CACHE:
        return _CACHE[key]
    d = out_dir or tempfile.mkdtemp(prefix="x87host")
    out = os.path.join(d, "libx87host%s.so" % "".join("_" + x.lower() for x in defines))
    subprocess.check_call(["g++"] + FLAGS + ["-D" + x for x in defines] + ["-o", out, SRC])
    L = C.CDLL(out)
    L.x87t_bin_residual.restype = C.c_double
    L.x87t_bin_residual.argtypes = [_D] * 2 + [C.c_double] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    L.x87t_pow10.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_double]
    L.x87t_operands.restype = C.c_int64
    L.x87t_operands.argtypes = [C.c_uint64, C.c_int64] + [C.c_void_p] * 4
    L.x87t_apply.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 8
    L.x87t_walker_residuals.argtypes = ([C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_double] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3)
    _CACHE[key] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def operands(L, seed, n):
    """x87t_arith's operand stream of n pairs from `seed`, then the structured extras: (ahi, alo, bhi, blo)."""
    tot = L.x87t_operands(seed, n, None, None, None, None)
    arr = [np.zeros(tot) for _ in range(4)]
    assert L.x87t_operands(seed, n, *[_p(a) for a in arr]) == tot
    return tuple(arr)


def apply(L, op, ahi, alo=None, bhi=None, blo=None, want_x87=False):
    """The host build's result of `op` (a name of OPS): (ohi, olo), or ohi alone for pow10; with want_x87 (+ - * / sqrt) also the
    x87 unit's result on the same operands as (xhi, xlo)."""
    code = OPS[op]
    n = len(ahi) // 4 if op == "angles_to_u" else len(ahi)
    k = VALUES_OUT.get(op, 1)
    ohi, olo = np.zeros(n * k), np.zeros(n * k)
    xhi = np.zeros(n) if want_x87 else None
    xlo = np.zeros(n) if want_x87 else None
    ahi = np.ascontiguousarray(ahi, dtype=np.float64)
    alo = None if alo is None else np.ascontiguousarray(alo, dtype=np.float64)
    bhi = None if bhi is None else np.ascontiguousarray(bhi, dtype=np.float64)
    blo = None if blo is None else np.ascontiguousarray(blo, dtype=np.float64)
    assert L.x87t_apply(code, n, _p(ahi), _p(alo), _p(bhi), _p(blo), _p(ohi), _p(olo), _p(xhi), _p(xlo)) == 0
    res = ohi if op == "pow10" else (ohi, olo)
    return (res, (xhi, xlo)) if want_x87 else res


def device_apply(model, op, ahi, alo=None, bhi=None, blo=None):
    """gf_internal_x87_eval: the same operation by the device build (k_x87_eval, compiled in the library's own unitarity translation
    unit) on `model`'s device; same shapes as apply()."""
    from golemflavor_amd import _lib
    Lg = _lib.lib()
    Lg.gf_internal_x87_eval.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 6
    n = len(ahi) // 4 if op == "angles_to_u" else len(ahi)
    k = VALUES_OUT.get(op, 1)
    bufs = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        d = model.alloc(max(a.nbytes, 8)).upload(a)
        bufs.append(d)
        return d.ptr
    d_in = [up(a) for a in (ahi, alo, bhi, blo)]
    d_ohi, d_olo = model.alloc(8 * max(n * k, 1)), model.alloc(8 * max(n * k, 1))
    bufs += [d_ohi, d_olo]
    _lib.check(Lg.gf_internal_x87_eval(model.device, OPS[op], n, *d_in, d_ohi.ptr, d_olo.ptr), "x87 eval")
    ohi, olo = d_ohi.download((n * k,)), d_olo.download((n * k,))
    for d in bufs:
        d.free()
    return ohi if op == "pow10" else (ohi, olo)


def model_tables(model):
    """gf_internal_bsm_tables: the model's smu / npu (hi, lo), inv2e and epow exactly as the device kernels read them."""
    from golemflavor_amd import _lib
    Lg = _lib.lib()
    Lg.gf_internal_bsm_tables.argtypes = [C.c_void_p] * 7 + [C.POINTER(C.c_int)]
    t = {k: np.zeros(18) for k in ("smu_hi", "smu_lo", "npu_hi", "npu_lo")}
    t["inv2e"], t["epow"] = np.zeros(64), np.zeros(64)
    nb = C.c_int(-1)
    _lib.check(Lg.gf_internal_bsm_tables(model._h, *[_p(t[k]) for k in ("smu_hi", "smu_lo", "npu_hi", "npu_lo", "inv2e", "epow")],
                                         C.byref(nb)), "bsm tables")
    t["inv2e"], t["epow"] = t["inv2e"][:nb.value].copy(), t["epow"][:nb.value].copy()
    return t


def walker_residuals(L, desc, tables, theta):
    """x87t_walker_residuals: every bin's residual of every row of `theta` (AoS, the model's columns) -> (n, nbins), from the
    descriptor's column indices and fixed values and the model's own tables (model_tables)."""
    from golemflavor_amd.enums import Texture
    th = np.ascontiguousarray(theta, dtype=np.float64)
    n, nd = th.shape
    nb = len(tables["inv2e"])
    out = np.zeros((n, nb))
    i32 = lambda v: np.ascontiguousarray(list(v), dtype=np.int32)
    f64 = lambda v: np.ascontiguousarray(list(v), dtype=np.float64)
    idx_sm, idx_mass, idx_mm = i32(desc.idx_sm[:4]), i32(desc.idx_mass[:2]), i32(desc.idx_mm[:4])
    mass_fixed = f64(desc.mass_fixed[:2])
    tb = {k: np.ascontiguousarray(v) for k, v in tables.items()}
    assert L.x87t_walker_residuals(n, nd, _p(th), _p(idx_sm), _p(idx_mass), _p(mass_fixed), _p(idx_mm),
                                   int(desc.texture == Texture.NONE.value), int(desc.idx_scale), float(desc.scale_fixed),
                                   _p(tb["smu_hi"]), _p(tb["smu_lo"]), _p(tb["npu_hi"]), _p(tb["npu_lo"]), nb, _p(tb["inv2e"]),
                                   _p(tb["epow"]), _p(out)) == 0
    return out


def non_unitary(res):
    """The reference's verdict from per-bin residuals (n, nbins): raised iff some bin is not (r < 1e-7) -- NaN raises too."""
    return ~(res < THRESHOLD).all(axis=1)


def same_bits(a, b):
    """Elementwise: the same double bit for bit, or both NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
