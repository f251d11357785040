"""Test infrastructure (not a test module): the host build of golemflavor_amd/csrc/gf_diag.hpp (tests/diag/diag_host.cpp, g++ with
contraction off), the seeded AR(1) chains both the CPU and the GPU diagnostics tests use, a numpy restatement of the summation
orders gf_diag.hpp fixes, a np.longdouble evaluation of the definitions, and the error bounds that follow from the orders.

Used by tests/test_diagnostics_host.py (CPU) and tests/test_gpu_diagnostics.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diag", "diag_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off"]

# (nsteps, nwalkers, ndim) and the seed of each, in order
SHAPES = [(2, 8, 4), (3, 8, 4), (65, 8, 4), (193, 14, 4), (600, 24, 7), (1000, 32, 12)]
SEEDS = [1, 2, 3, 4, 5, 6]
PHIS = (0.0, 0.5, 0.9, 0.7)
FIELDS = ("tau", "tau_mean", "rhat", "window", "window_mean", "nexcluded", "rho", "rho_mean")

# |tau_mean - mcmc.integrated_time(walker_mean, tol=0)|, the existing host FFT path: four times the largest difference measured with the
# host build over SHAPES (profiles/diagnostics/README.txt has the figure and the case that attains it); the FFT's error has no
# bound that could be derived
FFT_MEASURED_MAX = 1.4211e-14
FFT_TOL = 4.0 * FFT_MEASURED_MAX

PARTS, LAG_BLOCK, WALKER_BLOCK = 256, 256, 32
U = 2.0 ** -53

_CACHE = {}


def build(out_dir=None):
    """Compile the host build and return the loaded library."""
    if out_dir in _CACHE:
        return _CACHE[out_dir]
    d = out_dir or tempfile.mkdtemp(prefix="dghost")
    out = os.path.join(d, "libdiaghost.so")
    subprocess.check_call(["g++"] + FLAGS + ["-o", out, SRC])
    L = C.CDLL(out)
    L.dgh_chain.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int64] + [C.c_void_p] * 8 + [C.c_int]
    _CACHE[out_dir] = L
    return L


def empty_outputs(ndim, nlags):
    return dict(tau=np.full(ndim, np.nan), tau_mean=np.full(ndim, np.nan), rhat=np.full(ndim, np.nan), window=np.full(ndim, -1, np.int64),
                window_mean=np.full(ndim, -1, np.int64), nexcluded=np.full(ndim, -1, np.int32), rho=np.full((ndim, nlags), np.nan),
                rho_mean=np.full((ndim, nlags), np.nan))


def host_diag(chain, c=5.0, maxlag=None, nthreads=None, L=None):
    """The host build's diagnostics of one chain (n, nwalkers, ndim): a dict of FIELDS."""
    L = L or build()
    x = np.ascontiguousarray(chain, dtype=np.float64)
    n, nw, nd = x.shape
    nlags = (n - 1 if maxlag is None else int(maxlag)) + 1
    o = empty_outputs(nd, nlags)
    nthreads = nthreads or min(16, len(os.sched_getaffinity(0)))
    rc = L.dgh_chain(x.ctypes.data, n, nw, nd, float(c), -1 if maxlag is None else int(maxlag), *[o[f].ctypes.data for f in FIELDS], nthreads)
    assert rc == 0, rc
    return o


def ar1_chain(shape, seed, phis=PHIS):
    """x_i = phi x_{i-1} + sqrt(1 - phi^2) e_i per series, phi cycling over `phis` per column, e from default_rng(seed)."""
    n, nw, nd = shape
    e = np.random.default_rng(seed).standard_normal(shape)
    phi = np.array([phis[d % len(phis)] for d in range(nd)])
    x = np.empty(shape)
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + np.sqrt(1 - phi * phi) * e[i]
    return x


def cases():
    return [(s, ar1_chain(s, seed)) for s, seed in zip(SHAPES, SEEDS)]


# ---- the summation orders of gf_diag.hpp in numpy (np.cumsum = np.add.accumulate is strictly sequential) --------------------------

def seqsum(a, axis):
    """Sum along `axis` in index order, starting from +0.0 as the C loops do."""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    z = np.zeros(a.shape[:-1] + (1,))
    return np.cumsum(np.concatenate([z, a], axis=-1), axis=-1)[..., -1]


def _pad(a, multiple):
    """Zero-pad the last axis to a multiple (adding +0.0 to a sum that started from +0.0 changes no bit)."""
    k = (-a.shape[-1]) % multiple
    return np.concatenate([a, np.zeros(a.shape[:-1] + (k,))], axis=-1) if k else a


def series_sum(terms):
    """(S, m) -> (S,): 256 strided partials, then the halving tree."""
    t = _pad(terms, PARTS)
    part = seqsum(t.reshape(t.shape[0], -1, PARTS), axis=1)
    s = PARTS // 2
    while s:
        part = part[:, :s] + part[:, s:2 * s]
        s //= 2
    return part[:, 0]


def acov(y, nlags):
    """(S, n) centred series -> (S, nlags): blocks of 256 products in order, then the blocks in order."""
    S, n = y.shape
    npad = -(-n // LAG_BLOCK) * LAG_BLOCK
    out = np.empty((S, nlags))
    for s in range(S):
        ext = np.zeros(npad + nlags)
        ext[:n] = y[s]
        win = np.lib.stride_tricks.sliding_window_view(ext, npad)[:nlags]          # win[t, i] = ext[i + t]
        p = ext[None, :npad] * win
        out[s] = seqsum(seqsum(p.reshape(nlags, -1, LAG_BLOCK), axis=2), axis=1)
    return out


def walker_mean(chain):
    """k_walker_mean's arithmetic: (n, nw, nd) -> (n, nd)."""
    n, nw, nd = chain.shape
    stride = (256 // nd) * nd
    flat = _pad(chain.reshape(n, nw * nd), stride)
    part = seqsum(flat.reshape(n, -1, stride), axis=1)
    return seqsum(part.reshape(n, stride // nd, nd), axis=1) / float(nw)


def _series_acf(x, nlags, want_halves):
    """(S, n) series -> racf (S, nlags), excluded (S,), halves (S, 4)"""
    S, n = x.shape
    with np.errstate(all="ignore"):
        nonfinite = ~np.isfinite(x).all(axis=1)
        m = series_sum(x) / float(n)
        y = x - m[:, None]
        halves = np.full((S, 4), np.nan)
        if want_halves:
            h = n // 2
            for k, lo in enumerate((0, n - h)):
                mu = series_sum(y[:, lo:lo + h]) / float(h)
                d = y[:, lo:lo + h] - mu[:, None]
                halves[:, 2 * k] = m + mu
                halves[:, 2 * k + 1] = series_sum(d * d) / float(h - 1)
        a = acov(y, nlags)
        a0 = a[:, 0]
        excl = nonfinite | ~(a0 > 0) | ~np.isfinite(a0)
        return a / a0[:, None], excl, halves


def _sokal(rho, c):
    taus = 2.0 * np.cumsum(rho) - 1.0
    m = np.arange(len(taus)) < c * taus
    w = int(np.argmin(m)) if not m.all() else len(taus) - 1
    return taus[w], w


def numpy_diag(chain, c=5.0, maxlag=None):
    """The diagnostics of one chain restated in numpy, order for order: a dict of FIELDS."""
    x = np.asarray(chain, dtype=np.float64)
    n, nw, nd = x.shape
    nlags = (n - 1 if maxlag is None else int(maxlag)) + 1
    o = empty_outputs(nd, nlags)
    with np.errstate(all="ignore"):
        racf, excl, halves = _series_acf(np.ascontiguousarray(x.reshape(n, nw * nd).T), nlags, True)
        racf, excl, halves = racf.reshape(nw, nd, nlags), excl.reshape(nw, nd), halves.reshape(nw, nd, 4)
        rm, exm, _ = _series_acf(np.ascontiguousarray(walker_mean(x).T), nlags, False)
        rm[exm] = np.nan
        for d in range(nd):
            inc = ~excl[:, d]
            k = int(inc.sum())
            r = _pad(np.where(inc[:, None], racf[:, d], 0.0).T, WALKER_BLOCK)      # (nlags, walkers)
            tot = seqsum(seqsum(r.reshape(nlags, -1, WALKER_BLOCK), axis=2), axis=1)
            o["rho"][d] = tot / float(k) if k else np.nan
            o["rho_mean"][d] = rm[d]
            o["tau"][d], o["window"][d] = _sokal(o["rho"][d], c)
            o["tau_mean"][d], o["window_mean"][d] = _sokal(rm[d], c)
            o["nexcluded"][d] = nw - k
            h = n // 2
            if k and h >= 2:
                q = halves[inc, d]
                grand = seqsum(q[:, [0, 2]].reshape(-1), 0) / float(2 * k)
                W = seqsum(q[:, [1, 3]].reshape(-1), 0) / float(2 * k)
                dd = q[:, [0, 2]].reshape(-1) - grand
                bh = seqsum(dd * dd, 0) / float(2 * k - 1)
                o["rhat"][d] = np.sqrt((float(h - 1) / float(h) * W + bh) / W)
    return o


# ---- the definitions in np.longdouble, directly (no FFT), and the bounds --------------------------------------------------------

def _exact_series(x, nlags):
    """(S, n) float64 -> A (S, nlags) longdouble, and sum |products| (S, nlags) float64"""
    S, n = x.shape
    xl = x.astype(np.longdouble)
    y = xl - xl.mean(axis=1)[:, None]
    y64 = np.abs(y).astype(np.float64)
    A = np.empty((S, nlags), dtype=np.longdouble)
    Sabs = np.empty((S, nlags))
    for t in range(nlags):
        A[:, t] = (y[:, :n - t] * y[:, t:]).sum(axis=1)
        Sabs[:, t] = (y64[:, :n - t] * y64[:, t:]).sum(axis=1)
    return A, Sabs


def depth_acov(n):
    """additions a product passes through at most in A(t), plus k = 3: the two centring subtractions and the product"""
    return LAG_BLOCK + -(-n // LAG_BLOCK) + 3


def depth_walkers(nw):
    """additions of the walker average plus its division"""
    return WALKER_BLOCK + -(-nw // WALKER_BLOCK) + 1


def exact_diag(chain, c=5.0):
    """The definitions evaluated in np.longdouble for a chain without excluded series, with the bounds of the fp64 results:
    rho / rho_mean (nd, n), their bounds drho / drho_mean, taus / taus_mean (nd, n) = 2 cumsum - 1, window / window_mean, tau / tau_mean,
    dtau / dtau_mean = 2 sum_{t <= window} drho, margin / margin_mean = min_{M <= window} |M - c taus(M)|, rhat, drhat."""
    x = np.asarray(chain, dtype=np.float64)
    n, nw, nd = x.shape
    nlags = n
    key = (x.shape, float(c), x.tobytes())
    if key in _CACHE:
        return _CACHE[key]
    out = {}
    A, Sabs = _exact_series(np.ascontiguousarray(x.reshape(n, nw * nd).T), nlags)
    # |delta A(t)| <= (depth + k) 2^-53 sum |products|; rho_w = A(t) / A(0): delta <= (dA(t) + |rho_w| dA(0)) / A(0) + 2^-53 |rho_w|
    dA = depth_acov(n) * U * Sabs
    a0 = A[:, :1]
    rw = A / a0
    drw = ((dA + np.abs(rw) * dA[:, :1]) / a0 + U * np.abs(rw)).astype(np.float64)
    rw, drw = rw.reshape(nw, nd, nlags), drw.reshape(nw, nd, nlags)
    out["rho"] = rw.mean(axis=0)
    out["drho"] = drw.mean(axis=0) + depth_walkers(nw) * U * np.abs(rw).mean(axis=0).astype(np.float64)
    # the ensemble-mean series is DEFINED as walker_mean()'s fp64 values (k_walker_mean's order, pinned bit for bit elsewhere)
    Am, Sm = _exact_series(np.ascontiguousarray(walker_mean(x).T), nlags)
    dAm = depth_acov(n) * U * Sm
    out["rho_mean"] = Am / Am[:, :1]
    out["drho_mean"] = ((dAm + np.abs(out["rho_mean"]) * dAm[:, :1]) / Am[:, :1] + U * np.abs(out["rho_mean"])).astype(np.float64)
    for tag in ("", "_mean"):
        rho = out["rho" + tag]
        taus = 2 * np.cumsum(rho, axis=1) - 1
        win = np.empty(nd, np.int64)
        margin = np.empty(nd)
        for d in range(nd):
            m = np.arange(nlags) < c * taus[d]
            win[d] = int(np.argmin(m)) if not m.all() else nlags - 1
            margin[d] = float(np.abs(np.arange(win[d] + 1) - c * taus[d, :win[d] + 1]).min())
        out["taus" + tag], out["window" + tag], out["margin" + tag] = taus, win, margin
        out["tau" + tag] = taus[np.arange(nd), win]
        out["dtau" + tag] = np.array([2 * out["drho" + tag][d, :win[d] + 1].sum() for d in range(nd)])
    out["rhat"], out["drhat"] = exact_rhat(x)
    _CACHE[key] = out
    return out


def exact_rhat(x):
    """Split R-hat in np.longdouble over all walkers, (nd,), and the bound of the fp64 result.

    With u = 2^-53, D = ceil(h / 256) + 8 the depth of a half's series sum and k = 2 nwalkers sequences:
      a sequence mean carries at most dmu = (2 D + 6) u max|x|   (the series mean, the centring, the half's mean, their sum);
      a sequence variance is a sum of squares: relative error at most (D + 6) u, and W, summed in walker order, (D + 6 + k + 1) u;
      B/h = sum (mean - grand)^2 / (k - 1): |delta| <= 4 dmu sum|mean - grand| / (k - 1) + (k + 4) u B/h   (first order);
      rhat = sqrt(a + (B/h) / W): |delta| <= (delta(B/h) / W + (B/h) / W (relW + 2 u)) / (2 rhat) + 3 u rhat."""
    n, nw, nd = x.shape
    h = n // 2
    if h < 2:
        return np.full(nd, np.nan), np.full(nd, np.nan)
    ld = np.longdouble
    xl = x.astype(ld)
    seq = np.concatenate([xl[:h], xl[n - h:]], axis=1)                              # (h, 2 nw, nd)
    mean = seq.mean(axis=0)
    var = ((seq - mean) ** 2).sum(axis=0) / (h - 1)
    k = 2 * nw
    W = var.mean(axis=0)
    grand = mean.mean(axis=0)
    bh = ((mean - grand) ** 2).sum(axis=0) / (k - 1)
    rhat = np.sqrt((ld(h - 1) / h * W + bh) / W)
    D = -(-h // PARTS) + 8
    dmu = (2 * D + 6) * U * float(np.abs(x).max())
    relW = (D + 6 + k + 1) * U
    dbh = 4 * dmu * np.abs(mean - grand).sum(axis=0) / (k - 1) + (k + 4) * U * bh
    drhat = (dbh / W + bh / W * (relW + 2 * U)) / (2 * rhat) + 3 * U * rhat
    return rhat, drhat.astype(np.float64)


def assert_same_bits(a, b, label=""):
    """Every field of two results bit for bit (NaN equal to NaN)."""
    for f in FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert x.shape == y.shape and x.dtype == y.dtype, (label, f, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float64:
            ok = np.array_equal(x.view(np.uint64), y.view(np.uint64)) or \
                (np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x) & (x == x), np.signbit(y) & (y == y)))
        else:
            ok = np.array_equal(x, y)
        assert ok, "%s: %s differs (first at %s)" % (label, f, np.argwhere(~((x == y) | ((x != x) & (y != y))))[:1])
