"""The energy-resolved Gaussian likelihood restated on the host for the tests: the reference's multi_gaussian
(golemflavor/llh.py:32-54, scipy's operations in scipy's order, the C library's pow / sqrt / log / exp) per energy bin, and the sum
of the terms in ascending bin order from 0.0.  test_binned_host.py holds it to oracle.multi_gaussian bit for bit."""
import math

import numpy as np


def _log_of_exp(x):
    """log(exp(x)) as the reference forms it: the pdf in fp64 first, so -inf below the underflow wall and quantised in the
    subnormal band"""
    try:
        y = math.exp(x)
    except OverflowError:
        y = math.inf
    if y == 0.0:
        return -math.inf
    return math.log(y)


def multi_gaussian_host(fr, m, sigma):
    """multi_gaussian(fr, m, sigma, offset = 0) for one composition: the operations of oracle/golem_oracle.c orc_multi_gaussian"""
    s = math.pow(float(sigma), 2)
    scale = math.sqrt(1.0 / s)
    log_pdet = math.log(s) + math.log(s) + math.log(s)
    maha = 0.0
    for i in range(3):
        d = (float(fr[i]) - float(m[i])) * scale
        maha += d * d
    logpdf = -0.5 * (3 * math.log(2 * math.pi) + log_pdet + maha)
    if logpdf != logpdf:
        return math.nan
    return _log_of_exp(logpdf) + 0.0


def binned_terms_host(fr_bins, meas):
    """fr_bins (n, K, 3) -> the K terms of every row, (n, K)"""
    f = np.asarray(fr_bins, dtype=np.float64)
    n, K, _ = f.shape
    assert K == meas.nbins
    out = np.empty((n, K))
    for i in range(n):
        for k in range(K):
            out[i, k] = multi_gaussian_host(f[i, k], meas.fr_bins[k], meas.sigma[k])
    return out


def binned_lnl_host(fr_bins, meas, offset=-320.0, return_terms=False):
    """lnL = offset + sum_k multi_gaussian(fr_k, m_k, sigma_k, 0): ascending k from 0.0, one rounding per add, then the offset"""
    terms = binned_terms_host(fr_bins, meas)
    acc = np.zeros(terms.shape[0])
    with np.errstate(invalid="ignore"):
        for k in range(terms.shape[1]):
            acc = acc + terms[:, k]
        lnl = acc + offset
    return (lnl, terms) if return_terms else lnl


def binned_bound(terms, lnprior, offset=-320.0):
    """(K + 4) 2^-52 (sum_k |term_k| + |offset| + |lnprior|) per row; inf where a term is not finite"""
    t = np.asarray(terms, dtype=np.float64)
    K = t.shape[1]
    with np.errstate(invalid="ignore"):
        return (K + 4) * 2.0 ** -52 * (np.abs(t).sum(axis=1) + abs(offset) + np.abs(lnprior))
