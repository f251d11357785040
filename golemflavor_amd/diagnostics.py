"""Convergence diagnostics of a stored chain on the device: what a reference job prints when it ends (acceptance fraction and
`sampler.acor`, golemflavor/mcmc.py:45-51), for every chain of a stacked sampler, without the chain crossing PCIe.

emcee is not a dependency of this package, so nothing here is "equal to emcee": THE DEFINITIONS ARE THIS PACKAGE'S OWN (DESIGN.md
section 6d, include/golemflavor_hip.h).  Per chain and column, n stored steps:
  tau, window            the integrated autocorrelation time of the walker-averaged normalised autocorrelation function
                         rho(t) = mean_w A_w(t) / A_w(0), with the window rule of `mcmc.integrated_time` (`sokal_window`);
  tau_mean, window_mean  the same of the ensemble-mean series `walker_mean()` returns -- the quantity `sampler.acor` estimates;
  nexcluded              walker series left out of rho and R-hat: constant (a walker that never moved) or holding a non-finite value;
  rhat                   split R-hat over the walkers' first and second halves.  Walkers of one ensemble are NOT independent
                         sequences: a diagnostic, not a guarantee;
  ess                    nwalkers n / tau;   converged(tol) = n >= tol tau.
The kernels are in csrc/gf_diag.hip, the arithmetic and the order of every sum in csrc/gf_diag.hpp.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GF_DIAG_MAX_STEPS, check  # noqa: F401


def sokal_window(taus, c):
    """Sokal's automatic window over taus(M) = 2 sum_{t <= M} rho(t) - 1: the smallest M with M >= c taus(M), else the last lag."""
    m = np.arange(len(taus)) < c * taus
    return int(np.argmin(m)) if not m.all() else len(taus) - 1


class ChainDiagnostics:
    """One chain's diagnostics.

    nsteps, nwalkers; tau, tau_mean, rhat (ndim,); window, window_mean (ndim,) int64; nexcluded (ndim,) int32; rho, rho_mean
    (ndim, maxlag + 1) or None; acceptance_fraction (nwalkers,) or None (a host chain has no counters)."""

    ARRAYS = ("tau", "window", "tau_mean", "window_mean", "rhat", "nexcluded")

    def __init__(self, **kw):
        self.rho = self.rho_mean = self.acceptance_fraction = None
        self.__dict__.update(kw)

    @property
    def ess(self):
        """Effective sample size per column: nwalkers n / tau."""
        return self.nwalkers * self.nsteps / self.tau

    def converged(self, tol=50):
        """n >= tol tau in every column (False where tau is NaN)."""
        return bool(np.all(self.nsteps >= tol * self.tau))

    def as_arrays(self):
        """Everything as a dict of arrays: the layout of the `.npz` a scan writes."""
        out = {k: np.asarray(getattr(self, k)) for k in self.ARRAYS}
        out["ess"] = np.asarray(self.ess)
        out["nsteps"], out["nwalkers"], out["c"] = np.int64(self.nsteps), np.int64(self.nwalkers), np.float64(self.c)
        for k in ("rho", "rho_mean", "acceptance_fraction"):
            if getattr(self, k) is not None:
                out[k] = np.asarray(getattr(self, k))
        return out

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **self.as_arrays())

    def __repr__(self):
        return "ChainDiagnostics(nsteps=%d, nwalkers=%d, tau=%s, rhat=%s)" % (self.nsteps, self.nwalkers, self.tau, self.rhat)


def run_diag_call(call, what, nchains, nsteps, nwalkers, ndim, c=5, maxlag=None, want_rho=False):
    """Drive one of the C entry points: `call(spec_pointer, out_pointer)`.  Returns [chain] ChainDiagnostics."""
    nsteps = int(nsteps)
    if nsteps > GF_DIAG_MAX_STEPS:
        raise ValueError("chain diagnostics hold a whole series in LDS: %d stored steps exceed %d -- thin the chain (run_mcmc(..., thin=%d))"
                         % (nsteps, GF_DIAG_MAX_STEPS, -(-nsteps // GF_DIAG_MAX_STEPS)))
    if nsteps < 2:
        raise ValueError("chain diagnostics need at least 2 stored steps")
    if not c > 0:
        raise ValueError("c must be positive")
    if maxlag is not None and not 0 <= int(maxlag) < nsteps:
        raise ValueError("maxlag must lie in [0, nsteps)")
    nlags = (nsteps - 1 if maxlag is None else int(maxlag)) + 1
    dp, ip, lp = _lib._dp, _lib._ip, _lib._lp
    a = dict(tau=np.full((nchains, ndim), np.nan), tau_mean=np.full((nchains, ndim), np.nan), rhat=np.full((nchains, ndim), np.nan),
             window=np.zeros((nchains, ndim), np.int64), window_mean=np.zeros((nchains, ndim), np.int64),
             nexcluded=np.zeros((nchains, ndim), np.int32))
    if want_rho:
        a["rho"] = np.full((nchains, ndim, nlags), np.nan)
        a["rho_mean"] = np.full((nchains, ndim, nlags), np.nan)
    spec = _lib.GfDiagSpec(float(c), -1 if maxlag is None else int(maxlag))
    ptr = {np.dtype(np.int64): lp, np.dtype(np.int32): ip, np.dtype(np.float64): dp}
    out = _lib.GfDiagOut(**{name: a[name].ctypes.data_as(ptr[a[name].dtype]) for name, _ in _lib.GfDiagOut._fields_ if name in a})
    check(call(C.byref(spec), C.byref(out)), what)
    return [ChainDiagnostics(nsteps=nsteps, nwalkers=int(nwalkers), c=float(c), **{k: v[ch] for k, v in a.items()}) for ch in range(nchains)]


def chain_diagnostics(chain, *, model, c=5, maxlag=None, want_rho=False):
    """The diagnostics of a host chain (nsteps, nwalkers, ndim) in the device's order (`chain_to_host`, or emcee's `chain` with its
    first two axes swapped).  model: any `Model` on the device to use.  More than 16384 steps: ValueError -- thin the chain."""
    x = np.ascontiguousarray(chain, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("chain must be (nsteps, nwalkers, ndim)")
    n, nw, nd = x.shape
    model = getattr(model, "model", model)

    def call(spec, out):
        return model._L.gf_chain_diagnostics(model._h, x.ctypes.data_as(_lib._dp), n, nw, nd, spec, out)
    return run_diag_call(call, "gf_chain_diagnostics", 1, n, nw, nd, c, maxlag, want_rho)[0]
