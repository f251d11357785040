"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_nested_post.hpp (tests/nested_post/
nested_post_host.cpp, g++ with contraction off), seeded log-weight profiles, a numpy restatement of the prefix order the header fixes, a
np.longdouble evaluation of the definitions, and the error bounds that follow from the orders.

Used by tests/test_nested_posterior_host.py (CPU), tests/test_gpu_nested_posterior.py and tests/test_gpu_nested_posterior_shapes.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "nested_post", "nested_post_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"]

LANES, LEAF, SCAN_BLOCK = 256, 4096, 64
U = 2.0 ** -53
# the largest error of the header's exp against mpmath over exp_grid(), in ulp of the exact value (2^-1074 in the subnormal range):
# measured with the host build (DESIGN.md 6e has the figure and the argument that attains it); the test asserts twice this
EXP_MEASURED_ULP = 0.8368

NS = [1, 2, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, LEAF - 1, LEAF, LEAF + 1, 65537]
NROWS = [1, 2, 63, 64, 65, 4097]
PROFILES = ("generic", "first", "last", "plateau", "span600")
U_MIN, U_MAX = 0.0, 1.0 - 2.0 ** -53          # the smallest and the largest offset 53 Philox bits can give

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="nphost")
    out = os.path.join(d, "libnphost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.nph_exp.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.nph_exp.restype = None
    L.nph_philox.argtypes = [C.c_void_p] * 3
    L.nph_philox.restype = None
    L.nph_offset.argtypes = [C.c_uint64, C.c_uint64]
    L.nph_offset.restype = C.c_double
    L.nph_posterior.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 7
    L.nph_resample.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p]
    _CACHE[out_dir] = L
    return L


def host_exp(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    build().nph_exp(x.ctypes.data, x.size, out.ctypes.data)
    return out


def host_philox(ctr, key):
    c, k, o = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    build().nph_philox(c.ctypes.data, k.ctypes.data, o.ctypes.data)
    return o


def host_offset(seed, run_id):
    return float(build().nph_offset(int(seed) & 0xFFFFFFFFFFFFFFFF, int(run_id)))


def host_posterior(lnw, theta, fixed=None):
    """The host build's posterior of one run: dict(m, S, S2, ess, sp, sp2, e, p, C, mean, cov)."""
    lnw = np.ascontiguousarray(lnw, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    n, nd = theta.shape
    fx = np.ascontiguousarray(np.zeros(nd) if fixed is None else fixed, dtype=np.int32)
    stats, e, p, Cp, mean, cov = np.zeros(6), np.empty(n), np.empty(n), np.empty(n), np.empty(nd), np.empty((nd, nd))
    rc = build().nph_posterior(lnw.ctypes.data, theta.ctypes.data, n, nd, fx.ctypes.data, *[a.ctypes.data for a in (stats, e, p, Cp, mean, cov)])
    assert rc == 0, rc
    return dict(zip(("m", "S", "S2", "ess", "sp", "sp2"), stats), e=e, p=p, C=Cp, mean=mean, cov=cov)


def host_resample(Cp, nrows, u):
    Cp = np.ascontiguousarray(Cp, dtype=np.float64)
    idx = np.empty(int(nrows), np.int64)
    assert build().nph_resample(Cp.ctypes.data, Cp.size, int(nrows), float(u), idx.ctypes.data) == 0
    return idx


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def exp_grid():
    """0, -2^-k, five neighbours of every multiple of ln 2 / 2 down to -745.2, the subnormal band, and seeded uniform arguments."""
    half = np.log(2.0) / 2
    xs = [np.array([0.0]), -(2.0 ** -np.arange(0, 61))]
    m = -half * np.arange(0, int(745.2 / half) + 1)
    for _ in range(3):
        xs.append(m)
        m = np.nextafter(m, -np.inf)
    m = -half * np.arange(0, int(745.2 / half) + 1)
    for _ in range(2):
        m = np.nextafter(m, np.inf)
        xs.append(m)
    xs.append(np.linspace(-745.1999, -708.3, 4000))
    xs.append(-745.2 * np.random.default_rng(11).uniform(size=20000))
    x = np.concatenate(xs)
    return x[(x <= 0) & (x > -745.2)]


def exact_exp_error_ulp(x, got):
    """|got - exp(x)| in ulp of the exact value (the spacing of doubles at it: 2^-1074 below 2^-1022), by mpmath at 100 bits."""
    import mpmath as mp
    mp.mp.prec = 100
    err = np.empty(len(x))
    for i, (xi, gi) in enumerate(zip(x.tolist(), got.tolist())):
        ex = mp.exp(mp.mpf(xi))
        e2 = max(int(mp.floor(mp.log(ex, 2))), -1022)
        err[i] = float(abs(mp.mpf(gi) - ex) / mp.mpf(2) ** (e2 - 52))
    return err


def profile(kind, n, seed):
    """Seeded log-weights [n] of one of PROFILES and theta [n][3] whose middle column is fixed."""
    rng = np.random.default_rng(seed)
    lnw = -30.0 * rng.uniform(size=n) ** 2 - 5.0
    if kind == "first":
        lnw[:] = -np.inf
        lnw[0] = -3.0
    elif kind == "last":
        lnw[:] = -np.inf
        lnw[-1] = -3.0
    elif kind == "plateau":
        lnw[:max(1, n // 3) if n > 1 else 0] = -np.inf
    elif kind == "span600":
        lnw = -600.0 * rng.uniform(size=n)
        lnw[rng.integers(n)] = 0.0
    theta = rng.uniform(-2.0, 3.0, size=(n, 3))
    theta[:, 1] = 0.625
    return lnw, theta, np.array([0, 1, 0], np.int32)


WIDE_NDIM, WIDE_FIXED = 12, {3: -41.5, 11: 0.625}          # sens.py's width; the fixed columns at odd positions, the last one among them


def profile_wide(kind, n, seed):
    """profile()'s log-weights with theta [n][12]: ten scanned columns of different centre and width (two of them correlated), the
    columns of WIDE_FIXED fixed at its values."""
    lnw = profile(kind, n, seed)[0]
    rng = np.random.default_rng(seed + 1000)
    theta = rng.uniform(-1.0, 1.0, size=(n, WIDE_NDIM)) * (0.25 + np.arange(WIDE_NDIM)) + np.linspace(-40.0, 3.0, WIDE_NDIM)
    theta[:, 5] = 0.5 * theta[:, 4] + 0.1 * theta[:, 5]
    fixed = np.zeros(WIDE_NDIM, np.int32)
    for c, v in WIDE_FIXED.items():
        theta[:, c] = v
        fixed[c] = 1
    return lnw, theta, fixed


# ---- the prefix order of gf_nested_post.hpp in numpy (np.cumsum is strictly sequential) -------------------------------------------------

def prefix_numpy(p):
    n = len(p)
    nb = -(-n // SCAN_BLOCK)
    pad = np.zeros(nb * SCAN_BLOCK)
    pad[:n] = p
    local = np.cumsum(pad.reshape(nb, SCAN_BLOCK), axis=1)
    last = np.array([local[b, min(SCAN_BLOCK, n - b * SCAN_BLOCK) - 1] for b in range(nb)])
    before = np.concatenate([[0.0], np.cumsum(last)[:-1]])
    out = local.copy()
    out[1:] = before[1:, None] + local[1:]
    return out.reshape(-1)[:n]


def resample_numpy(Cp, nrows, u):
    """(t, index): np.minimum(np.searchsorted(C, t, side="right"), last) with t_k = (k + u) / N and last = the last point that carries
    weight (n - 1 unless the run ends in points of zero weight)"""
    t = (np.arange(nrows, dtype=np.float64) + u) / float(nrows)
    last = int(np.searchsorted(Cp, Cp[-1], side="left"))
    return t, np.minimum(np.searchsorted(Cp, t, side="right"), last)


# ---- the definitions in np.longdouble and the bounds ---------------------------------------------------------------------------------

def tree_depth(n):
    """Additions a term passes through, at most, in the header's tree sum of n terms."""
    leaves = max(1, -(-int(n) // LEAF))
    return 16 + 6 + 3 + (-(-leaves // LANES)) + 6 + 3


def exact_posterior(lnw, theta):
    """dict(p, ess, mean, cov, fact, C) in np.longdouble: numpy's definitions (np.average, np.cov with aweights)."""
    ld = np.longdouble
    lw = np.asarray(lnw, dtype=ld)
    with np.errstate(all="ignore"):
        e = np.where(np.isneginf(lw), ld(0), np.exp(lw - lw.max()))
    p = e / e.sum()
    x = np.asarray(theta, dtype=ld)
    mean = (p[:, None] * x).sum(axis=0) / p.sum()
    fact = p.sum() - (p * p).sum() / p.sum()
    d = x - mean
    with np.errstate(all="ignore"):
        cov = (p[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / fact
    return dict(p=p, ess=e.sum() ** 2 / (e * e).sum(), mean=mean, cov=cov, fact=fact, C=np.cumsum(p), absx=(p[:, None] * np.abs(x)).sum(axis=0),
                absd=(p[:, None, None] * np.abs(d[:, :, None] * d[:, None, :])).sum(axis=0))


def bounds(n, exact, exp_ulp=None):
    """First-order bounds of the fp64 results, u = 2^-53, D = tree_depth(n), E = the exp's error in ulp (1 ulp <= 2 u relative):
      e_i      relative eps_e = (2 E + 746) u: the exp, and its argument lnw - m (|.| < 746) rounded once;
      S, S2    sums of positive terms: eps_e + D u and 2 eps_e + (D + 1) u;   ess = S S / S2: 4 eps_e + (3 D + 3) u;
      p_i      e_i / S: eps_p = 2 eps_e + (D + 1) u;    C_i: eps_p + (SCAN_BLOCK + ceil(n / SCAN_BLOCK)) u, absolute (C <= 1);
      mean     sum p x over sum p, each sum eps_p + (D + 1) u of sum p |x|, and the division:  (2 eps_p + (2 D + 3) u) sum p |x| / sum p;
      cov      a term p (x_a - m_a)(x_b - m_b) carries eps_p + 4 u, the sum D u; centring on the device mean instead of the exact
               one changes the sum by dm_a dm_b sum p only (sum p (x - m) = 0); fact = sum p - sum p^2 / sum p carries
               dfact = (3 eps_p + (2 D + 3) u) (sum p + sum p^2) absolutely; the division u:
               |dcov| <= (eps_p + (D + 4) u) sum p |d_a d_b| / fact + dm_a dm_b / fact + |cov| (dfact / fact + u)."""
    E = EXP_MEASURED_ULP if exp_ulp is None else exp_ulp
    D = tree_depth(n)
    eps_e = (2 * E + 746) * U
    eps_p = 2 * eps_e + (D + 1) * U
    sp = float(exact["p"].sum())
    dmean = (2 * eps_p + (2 * D + 3) * U) * exact["absx"].astype(np.float64) / sp
    fact = float(exact["fact"])
    out = dict(ess=(4 * eps_e + (3 * D + 3) * U) * float(exact["ess"]), p=eps_p, C=eps_p + (SCAN_BLOCK + -(-n // SCAN_BLOCK)) * U, mean=dmean)
    if fact > 0:
        dfact = (3 * eps_p + (2 * D + 3) * U) * (sp + float((exact["p"] ** 2).sum()))
        out["cov"] = ((eps_p + (D + 4) * U) * exact["absd"].astype(np.float64) + np.outer(dmean, dmean)) / fact \
            + np.abs(exact["cov"]).astype(np.float64) * (dfact / fact + U)
    return out


def separation(cs, t):
    """The smallest |t_k - C_i| over the rows with t_k > 0 and the boundaries C_i before the last point that carries weight (what lies
    behind it decides no row: every t beyond goes to that point).  t_k = 0 (u = 0, k = 0) is left out: C_i > 0 holds or fails
    exactly in every summation order, a sum of non-negative terms being zero only if all of them are."""
    last = int(np.searchsorted(cs, cs[-1], side="left"))
    inner, t = cs[:last], t[t > 0]
    if len(inner) == 0 or len(t) == 0:
        return 1.0
    j = np.searchsorted(inner, t)
    lo, hi = inner[np.maximum(j - 1, 0)], inner[np.minimum(j, len(inner) - 1)]
    return float(np.minimum(np.abs(t - lo), np.abs(t - hi)).min())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and (np.array_equal(a.view(np.uint64), b.view(np.uint64)) or
                                   (np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & (a == a), np.signbit(b) & (b == b))))
