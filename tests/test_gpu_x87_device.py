"""GPU: the DEVICE build of the emulated x87 arithmetic (gf_x87.hpp as compiled into the library, with its flags and inlining)
against the HOST build of the same header (tests/x87/x87_host.cpp, g++ with contraction off), which tests/test_x87_emulation.py
pins to the CPU's x87 unit and to mpmath.  Bit for bit: the primitives on the x87t_arith operand stream and structured extras, the
transcendentals, cr_pow10 and angles_to_u; every (walker, bin) residual of the product's own chain kernels (serial, three- and
nine-lane) against x87t_walker_residuals fed the model's own tables; and the status Model.lnprob ships for the walkers whose
verdict lies near the reference's threshold (fr.py:493-494).  A device-only difference -- a contraction the pragma fails to stop,
a device sqrt / nearbyint / ldexp that differs from glibc's, a table split differently -- fails here."""
import ctypes as C

import numpy as np
import pytest

import x87_harness as H
from common import BIN_EDGES
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import GF_LAYOUT_AOS, GF_LAYOUT_SOA, Model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hx(tmp_path_factory):
    return H.build(str(tmp_path_factory.mktemp("x87dev")))


@pytest.fixture(scope="module")
def dev_model():
    ps = Cf.texture_paramset(6)
    kw = dict(texture=Texture.OET, dimension=6, binning=BIN_EDGES, source_ratio=(0., 1., 0.), bestfit_fr=(1 / 3,) * 3, smearing=0.02)
    with Model(compile_model(ps, "BSM_GAUSS", **kw)) as m:
        yield m


def _pairs(v):
    """long doubles -> (hi, lo) as from_ld splits them"""
    hi = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    lo[~np.isfinite(hi)] = 0.0
    return hi, lo


def _random_ld(rng, n, lo, hi):
    """n long doubles uniform in [lo, hi) with full 64-bit significands"""
    m = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(np.longdouble) * np.longdouble(2.0) ** -62
    return np.longdouble(lo) + (np.longdouble(hi) - np.longdouble(lo)) * m


def _check_same(name, dev, host):
    for d, h in zip(dev if isinstance(dev, tuple) else (dev,), host if isinstance(host, tuple) else (host,)):
        ok = H.same_bits(d, h)
        assert ok.all(), "%s: %d of %d differ, first at %s" % (name, int((~ok).sum()), ok.size, np.flatnonzero(~ok)[:8])


def test_basic_operations_device_equal_host_and_x87(hx, dev_model):
    """+ - * / sqrt on the 1.6 M pairs of test_basic_operations_are_bit_exact plus the structured extras: the device's (hi, lo) is
    the host build's bit for bit (NaN == NaN), and on the random stream the value is the x87 unit's."""
    for seed in (1, 2):
        ops = H.operands(hx, seed, 800000)
        for op in ("add", "sub", "mul", "div", "sqrt"):
            args = ops if op != "sqrt" else ops[:2]
            host, x = H.apply(hx, op, *args, want_x87=True)
            dev = H.device_apply(dev_model, op, *args)
            _check_same("%s seed %d" % (op, seed), dev, host)
            with np.errstate(invalid="ignore"):
                got = dev[0][:800000].astype(np.longdouble) + dev[1][:800000].astype(np.longdouble)
                want = x[0][:800000].astype(np.longdouble) + x[1][:800000].astype(np.longdouble)
            assert np.array_equal(got, want, equal_nan=True), (op, seed)


def test_transcendentals_device_equal_host(hx, dev_model):
    """sincos, asin, acos, hypot on random 64-bit arguments and edges, cr_pow10 over every operator dimension's scale range (grid
    points, integers, the range ends and random doubles), angles_to_u on random and edge angles: device == host build, bit for bit."""
    rng = np.random.default_rng(21)
    LD = np.longdouble
    pi = LD("3.14159265358979323846264338327950288")
    t = np.concatenate([_random_ld(rng, 40000, -8, 8), _random_ld(rng, 20000, 0, 2 * pi), _random_ld(rng, 5000, -1e-3, 1e-3),
                        np.array([0, -0.0, pi / 2, pi, 2 * pi, 1e-9, -1e-9, 3.97935, 4.08, 2 * np.pi], dtype=LD)])
    ahi, alo = _pairs(t)
    _check_same("sincos", H.device_apply(dev_model, "sincos", ahi, alo), H.apply(hx, "sincos", ahi, alo))
    s = np.concatenate([_random_ld(rng, 40000, -1, 1), np.sqrt(_random_ld(rng, 20000, 0, 1)), _random_ld(rng, 5000, 0.71, 0.73),
                        np.array([0, -0.0, 1, -1, 0.72, -0.72, 1e-9, np.sqrt(1e-9), 0.5, np.sqrt(0.5)], dtype=LD)])
    shi, slo = _pairs(s)
    for op in ("asin", "acos"):
        _check_same(op, H.device_apply(dev_model, op, shi, slo), H.apply(hx, op, shi, slo))
    ops = H.operands(hx, 3, 200000)
    fin = np.isfinite(ops[0]) & np.isfinite(ops[2])
    args = tuple(a[fin] for a in ops)
    _check_same("hypot", H.device_apply(dev_model, "hypot", *args), H.apply(hx, "hypot", *args))
    x = [rng.uniform(-72.0, -20.0, 200000), np.arange(-72.0, -19.0), np.arange(-72.0, -20.0, 1 / 1024)]
    for lo, hi in Cf.SCALE_BOUNDARIES.values():
        x.append(np.array([lo, hi, np.nextafter(lo, 0), np.nextafter(hi, -100)]))
    x = np.concatenate(x)
    _check_same("pow10", H.device_apply(dev_model, "pow10", x), H.apply(hx, "pow10", x))
    n = 20000
    ang = np.column_stack([rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)])
    edge = np.array([0., 1., 1e-9, 0.5, 0.25, 0.307, 0.9565, 0.538, (1 - 0.02195) ** 2])
    grid = np.array(np.meshgrid(edge, edge, edge, [0., 1e-9, np.pi, 2 * np.pi, 4.08]), dtype=float).reshape(4, -1).T
    ang = np.ascontiguousarray(np.concatenate([ang, grid]).reshape(-1))
    _check_same("angles_to_u", H.device_apply(dev_model, "angles_to_u", ang), H.apply(hx, "angles_to_u", ang))


# ---- the chain through the product's kernels --------------------------------------------------------------------------------
# (dimension, texture, 12 columns, NP angles: None | "sampled" | "fixed", bins, layout)
CONFIGS = [
    (3, Texture.OEU, False, None, 1, GF_LAYOUT_AOS),
    (4, Texture.OET, True, None, 33, GF_LAYOUT_SOA),
    (5, Texture.OEU, True, None, 20, GF_LAYOUT_AOS),
    (6, Texture.OUT, False, None, 64, GF_LAYOUT_SOA),
    (6, Texture.OEU, False, None, 20, GF_LAYOUT_SOA),
    (7, Texture.OUT, True, None, 20, GF_LAYOUT_AOS),
    (7, Texture.OET, False, None, 1, GF_LAYOUT_SOA),
    (8, Texture.OEU, True, None, 64, GF_LAYOUT_AOS),
    (8, Texture.OUT, False, None, 33, GF_LAYOUT_SOA),
    (5, Texture.NONE, False, "sampled", 20, GF_LAYOUT_SOA),
    (6, Texture.NONE, True, "fixed", 33, GF_LAYOUT_AOS),
]


def _paramset(dim, twelve, np_mode):
    from test_oracle_golden import _mm_paramset
    if np_mode == "sampled":
        return _mm_paramset(dim, twelve)
    return Cf.fr_paramsets(dim, (0.4, 0.0))[1] if twelve else Cf.texture_paramset(dim)


def _device_residuals(m, th, layout, walkers, bins, which):
    n = th.shape[0]
    L = _lib.lib()
    L.gf_internal_uni_residuals.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                            C.c_void_p]
    arr = np.ascontiguousarray(th if layout == GF_LAYOUT_AOS else th.T)
    w = np.ascontiguousarray(walkers, dtype=np.int64)
    b = np.ascontiguousarray(bins, dtype=np.int32)
    d_th, d_w, d_b, d_o = m.alloc(arr.nbytes).upload(arr), m.alloc(w.nbytes).upload(w), m.alloc(b.nbytes).upload(b), m.alloc(8 * len(w))
    _lib.check(L.gf_internal_uni_residuals(m._h, d_th.ptr, int(layout), n, d_w.ptr, d_b.ptr, len(w), which, d_o.ptr), "uni residuals")
    out = d_o.download((len(w),))
    for d in (d_th, d_w, d_b, d_o):
        d.free()
    return out


def _shipped_status(m, th, layout):
    n = th.shape[0]
    arr = np.ascontiguousarray(th if layout == GF_LAYOUT_AOS else th.T)
    d_th, d_lp, d_st = m.alloc(arr.nbytes).upload(arr), m.alloc(8 * n), m.alloc(4 * n)
    m.lnprob_device(d_th.ptr, n, d_lp.ptr, None, d_st.ptr, layout=layout)
    m.sync()
    st = d_st.download((n,), dtype=np.int32)
    for d in (d_th, d_lp, d_st):
        d.free()
    return st


@pytest.mark.parametrize("dim,tex,twelve,np_mode,nbins,layout", CONFIGS)
def test_chain_kernels_equal_host_build(hx, oracle, dim, tex, twelve, np_mode, nbins, layout):
    """Every (walker, bin) residual of gf_internal_uni_residuals -- which = 0 (serial, walker_terms + walker_bin_residual), 1 (three
    lanes, k_uni_resolve's), 100 (nine lanes, the settle step's) -- equals x87t_walker_residuals on the model's own tables, bit for
    bit, on three walker sets: a spread over the whole scale range; every pool walker whose oracle residual lies in [10^-7.5,
    10^-6.5]; knife-edge walkers (scale nudged off band walkers) whose host residual lies within 1 % of 1e-7.  For the band and
    knife-edge walkers the status Model.lnprob ships (host entry; device entry AoS and SoA) is the harness verdict."""
    rng = np.random.default_rng(1000 * dim + 10 * nbins + int(tex.value))
    ps = _paramset(dim, twelve, np_mode)
    lo, hi = Cf.SCALE_BOUNDARIES[dim]
    edges = np.sort(10 ** rng.uniform(4.3, 7.3, nbins + 1)) if nbins > 1 else np.array([6e4, 1e7])
    kw = dict(texture=tex, dimension=dim, binning=edges, source_ratio=(0., 1., 0.), bestfit_fr=(1 / 3,) * 3, smearing=0.02)
    if np_mode == "fixed":
        kw["mm_fixed"] = (0.3, 0.7, 0.45, 2.1)

    def draw(n, slo, shi):
        if np_mode == "sampled":
            box = np.array([p.seed if p.seed is not None else p.ranges for p in ps], dtype=float)
        else:
            box = np.array(ps.seeds, dtype=float)
        th = rng.uniform(box[:, 0], box[:, 1], size=(n, len(ps)))
        th[:, -1] = rng.uniform(slo, shi, n)
        return th

    spread = draw(1500, lo, hi)
    spread[:301, -1] = np.linspace(lo, hi, 301)                     # the whole range, both ends included
    okw = dict(kw, texture=tex.name)
    om = oracle.make_model(ps, "BSM_GAUSS", **okw)
    pool = draw(12000 if nbins <= 20 else 5000, lo, hi)
    r80 = oracle.unitarity_residual_batch(om, pool)
    band = pool[(r80 >= 10 ** -7.5) & (r80 <= 10 ** -6.5)]
    with Model(compile_model(ps, "BSM_GAUSS", **kw)) as m:
        tables = H.model_tables(m)
        assert len(tables["inv2e"]) == nbins
        # knife-edge walkers: band walkers with the scale nudged by up to 1e-3 decades, kept where the host residual is 1e-7 +- 1 %
        knife = np.zeros((0, len(ps)))
        if len(band):
            cand = np.repeat(band[:80], 48, axis=0)
            cand[:, -1] += rng.uniform(-1e-3, 1e-3, len(cand))
            worst = H.walker_residuals(hx, m.desc, tables, cand).max(axis=1)
            knife = cand[np.abs(worst / 1e-7 - 1) <= 0.01]
        print("\nd=%d %s %s np=%s bins=%d layout=%d: spread %d, band %d, knife-edge %d"
              % (dim, tex.name, "12col" if twelve else "7col", np_mode, nbins, layout, len(spread), len(band), len(knife)))
        sets = {"spread": spread, "band": band, "knife": knife}
        for name, th in sets.items():
            if not len(th):
                continue
            want = H.walker_residuals(hx, m.desc, tables, th)
            n = len(th)
            walkers, bins = np.repeat(np.arange(n), nbins), np.tile(np.arange(nbins), n)
            for which in (0, 1, 100):
                got = _device_residuals(m, th, layout, walkers, bins, which).reshape(n, nbins)
                ok = H.same_bits(got, want)
                assert ok.all(), "%s which=%d: %d of %d residuals differ (walkers %s)" % (
                    name, which, int((~ok).sum()), ok.size, np.unique(np.nonzero(~ok)[0])[:8])
            if name == "spread":
                assert np.isfinite(want).mean() > 0.99
                continue
            verdict = H.non_unitary(want)
            st_host = m.lnprob(th)[1]
            assert np.array_equal(st_host == _lib.GF_ST_NON_UNITARY, verdict), (name, np.flatnonzero((st_host == 2) != verdict))
            for lay in (GF_LAYOUT_AOS, GF_LAYOUT_SOA):
                st = _shipped_status(m, th, lay)
                assert np.array_equal(st == _lib.GF_ST_NON_UNITARY, verdict), (name, lay, np.flatnonzero((st == 2) != verdict))
    if (tex == Texture.OEU and dim >= 5) or (tex == Texture.OUT and dim >= 6):
        assert len(band) > 0, "the failing region has no band walkers"
