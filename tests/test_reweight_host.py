"""Reweighting a stored chain, the parts that need no device: the log-weight rules of csrc/gf_reweight.hpp (host build, g++ with
contraction off) against numpy, `reweight.reweight_host` against the np.longdouble definitions of tests/nested_post_harness.py, the
parsing of targets, and the binding of the new entry points."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nested_post_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import reweight as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "reweight", "reweight_host.cpp")


@pytest.fixture(scope="module")
def host():
    d = tempfile.mkdtemp(prefix="rwhost")
    out = os.path.join(d, "librwhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, SRC])
    L = C.CDLL(out)
    L.rwh_lnw.argtypes = [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3
    L.rwh_lnw.restype = None
    L.rwh_resample_id.argtypes = [C.c_uint64, C.c_int]
    L.rwh_resample_id.restype = C.c_uint64
    return L


def crafted():
    """Every pair of (finite of either sign and size, +-0, subnormal, -inf, +inf, NaN) under every status, and seeded finite pairs
    whose difference rounds."""
    special = np.array([-745.3, -3.5, -0.0, 0.0, 5e-324, 7.25, 1e308, -1e308, -np.inf, np.inf, np.nan])
    a, b, s = np.meshgrid(special, special, np.arange(4, dtype=np.int32), indexing="ij")
    rng = np.random.default_rng(5)
    lt = np.concatenate([a.ravel(), rng.normal(-20, 30, 4000)])
    l0 = np.concatenate([b.ravel(), rng.normal(-20, 30, 4000)])
    st = np.concatenate([s.ravel(), rng.integers(0, 4, 4000).astype(np.int32)])
    return np.ascontiguousarray(lt), np.ascontiguousarray(l0), np.ascontiguousarray(st, dtype=np.int32)


def test_rules_bit_for_bit(host):
    lt, l0, st = crafted()
    n = len(lt)
    lnw, kind, counts = np.empty(n), np.empty(n, np.int32), np.zeros(4, np.int64)
    host.rwh_lnw(lt.ctypes.data, l0.ctypes.data, st.ctypes.data, n, lnw.ctypes.data, kind.ctypes.data, counts.ctypes.data)
    # the rules, stated independently of reweight.lnw_host
    bad = ~np.isfinite(l0)
    nonu = ~bad & (st == _lib.GF_ST_NON_UNITARY)
    out = ~bad & ~nonu & (np.isnan(lt) | (lt == -np.inf))
    kept = ~bad & ~nonu & ~out
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(kept, np.subtract(lt, l0), -np.inf)
    assert H.same_bits(lnw, want)
    assert counts.tolist() == [int(kept.sum()), int(bad.sum()), int(nonu.sum()), int(out.sum())]
    assert min(counts) >= 48                                      # every case is there (outside: 8 finite l0 x 2 l_t x 3 statuses)
    assert np.array_equal(kind, np.select([bad, nonu, out], [1, 2, 3], 0))
    lnw2, kind2 = rw.lnw_host(lt, l0, st)
    assert H.same_bits(lnw2, want) and np.array_equal(kind2, kind)
    assert np.isposinf(lnw[kept & np.isposinf(lt)]).all()          # +inf under the target is kept as it is: the subtraction


def test_resample_id(host):
    for sid, t in ((0, 0), (7, 63), (2 ** 40 + 3, 5)):
        assert host.rwh_resample_id(sid, t) == sid * _lib.GF_REWEIGHT_MAX_TARGETS + t
    assert _lib.GF_REWEIGHT_MAX_TARGETS == 64


@pytest.mark.parametrize("n", [1, 64, 4097])
@pytest.mark.parametrize("kind", ["generic", "plateau", "span600"])
def test_reweight_host_against_exact(n, kind):
    lnw, theta, _ = H.profile(kind, n, seed=100 + n)
    rng = np.random.default_rng(n)
    l0 = rng.normal(-10, 3, n)
    lt = np.where(np.isneginf(lnw), -np.inf, lnw + l0)             # lt - l0 differs from lnw by one rounding
    r = rw.reweight_host(theta, l0, lt, nrows=65, u=0.25)
    ex = H.exact_posterior(r["lnw"], theta)
    b = H.bounds(n, ex, exp_ulp=1.0)                               # numpy's exp: below one ulp
    assert abs(r["ess"] - float(ex["ess"])) <= b["ess"]
    assert np.all(np.abs(r["mean"] - ex["mean"].astype(np.float64)) <= b["mean"] + 1e-300)
    assert np.all(np.abs(r["p"] - ex["p"].astype(np.float64)) <= b["p"] * ex["p"].astype(np.float64) + 1e-300)
    if n > 1 and "cov" in b:
        assert np.all(np.abs(r["cov"] - ex["cov"].astype(np.float64)) <= b["cov"] + 1e-300)
    assert r["outside"] == int(np.isneginf(lnw).sum()) and r["bad_base"] == 0
    assert r["index"].min() >= 0 and r["index"].max() < n and np.all(np.diff(r["index"]) >= 0)
    assert np.all(r["p"][r["index"]] > 0)                          # a row of zero weight is never taken
    assert np.array_equal(r["rows"], theta[r["index"]])


def test_reweight_host_without_posterior():
    theta = np.random.default_rng(1).uniform(size=(10, 3))
    st = np.full(10, _lib.GF_ST_NON_UNITARY, np.int32)
    r = rw.reweight_host(theta, np.zeros(10), np.zeros(10), status=st, nrows=4)
    assert r["ess"] == 0.0 and r["nonunitary"] == 10 and np.isnan(r["lnz_ratio"])
    assert np.isnan(r["mean"]).all() and np.isnan(r["cov"]).all() and np.isnan(r["rows"]).all() and (r["index"] == -1).all()
    r = rw.reweight_host(theta, np.full(10, -np.inf), np.zeros(10))
    assert r["bad_base"] == 10 and r["ess"] == 0.0


class _FakeModel:
    _h, ndim = 1, 6


def test_target_parsing():
    a, b = rw.Measurement(bestfit_fr=(0.3, 0.36, 0.34)), rw.Measurement(injected_ratio=(1, 2, 0), smearing=0.05)
    assert np.allclose(b.bestfit_fr, (1 / 3, 2 / 3, 0)) and b.smearing == 0.05 and a.smearing is None and a.offset is None
    kind, per = rw.parse_targets([a, b], 3)
    assert kind == "measurement" and len(per) == 3 and all(p == [a, b] for p in per)
    kind2, per2 = rw.parse_targets([[a, b], [a, b], [a, b]], 3)
    assert kind2 == kind and per2 == per
    kind3, per3 = rw.parse_targets([[a], [b]], 2)
    assert per3 == [[a], [b]]
    m = _FakeModel()
    assert rw.parse_targets([m], 2) == ("model", [[m], [m]])
    with pytest.raises(TypeError):
        rw.parse_targets([a, m], 1)                                 # the kinds do not mix
    with pytest.raises(TypeError):
        rw.parse_targets([a, "x"], 1)
    with pytest.raises(ValueError):
        rw.parse_targets([a] * 65, 1)                               # T > 64
    assert len(rw.parse_targets([a] * 64, 1)[1][0]) == 64
    with pytest.raises(ValueError):
        rw.parse_targets([], 1)
    with pytest.raises(ValueError):
        rw.parse_targets([[a], [a, b]], 2)                          # every chain the same T
    with pytest.raises(ValueError):
        rw.parse_targets([[a], [a]], 3)                             # one list per chain
    with pytest.raises(ValueError):
        rw.parse_targets([[a], a], 2)
    for bad in (dict(), dict(bestfit_fr=(1, 0, 0), injected_ratio=(1, 0, 0)), dict(bestfit_fr=(1, 0)), dict(bestfit_fr=(1, 0, np.nan)),
                dict(bestfit_fr=(1, 0, 0), smearing=0.0), dict(injected_ratio=(0, 0, 0)), dict(injected_ratio=(1, -1, 1))):
        with pytest.raises(ValueError):
            rw.Measurement(**bad)


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    names = set(re.findall(r"\b(gf_sampler_reweight\w*)\s*\(", hdr))
    assert names == {"gf_sampler_reweight", "gf_sampler_reweight_lnw", "gf_sampler_reweight_rows_device", "gf_sampler_reweight_rows",
                     "gf_sampler_reweight_marginals", "gf_sampler_reweight_intervals", "gf_sampler_reweight_regions"}
    for name in names:
        assert name in _lib.SIGNATURES, name
    assert "#define GF_ABI_VERSION 5" in hdr and "#define GF_REWEIGHT_MAX_TARGETS 64" in hdr
    # struct gf_reweight_spec / gf_reweight_out, field for field
    spec = re.search(r"typedef struct gf_reweight_spec \{(.*?)\} gf_reweight_spec;", hdr, re.S).group(1)
    spec = re.sub(r"/\*.*?\*/", "", spec, flags=re.S)
    fields = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in spec.split(";") if d.strip()]
    assert fields == [f for f, _ in _lib.GfReweightSpec._fields_]
    out = re.search(r"typedef struct gf_reweight_out \{(.*?)\} gf_reweight_out;", hdr, re.S).group(1)
    out = re.sub(r"/\*.*?\*/", "", out, flags=re.S)
    ofields = [n for d in out.split(";") if d.strip() for n in re.findall(r"\*\s*(\w+)", d)]
    assert ofields == [f for f, _ in _lib.GfReweightOut._fields_]
    assert C.sizeof(_lib.GfReweightSpec) == 48 and C.sizeof(_lib.GfReweightOut) == 64


def test_scan_arguments_without_a_device(capsys):
    from golemflavor_amd import scan
    tg = scan.reweight_targets([0.30, 0.36, 0.34, 1, 2, 0], [0.05, 0.01])
    assert len(tg) == 4 and [sm for _, sm in tg] == [0.05, 0.01, 0.05, 0.01]
    assert np.allclose(tg[0][0], (0.30, 0.36, 0.34))
    assert np.allclose(tg[2][0], (1 / 3, 2 / 3, 0))
    assert scan.reweight_targets([1, 1, 1], None) == [((1 / 3, 1 / 3, 1 / 3), None)]
    for bad in (([1, 1], None), ([], None), ([1, 1, 1], [0.0]), ([0, 0, 0], None), ([1, -1, 1], None), ([1, 1, 1] * 9, [0.1] * 8)):
        with pytest.raises(ValueError):
            scan.reweight_targets(*bad)
    # the checks of main come before anything touches a device
    for argv, text in ((["--config", "C5", "--reweight-injected", "1", "1", "1"], "needs --datadir"),
                       (["--config", "C4", "--datadir", "x", "--reweight-injected", "1", "1", "1"], "DeviceEnsembleSampler.reweight"),
                       (["--config", "C5", "--datadir", "x", "--reweight-injected", "1", "1"], "triples"),
                       (["--config", "C5", "--datadir", "x", "--reweight-rows", "10"], "need --reweight-injected"),
                       (["--config", "C5", "--datadir", "x", "--reweight-injected", "1", "1", "1", "--reweight-rows", "0"], "at least 1")):
        with pytest.raises(SystemExit):
            scan.main(argv)
        assert text in capsys.readouterr().err, argv
