"""The posterior of the flavour composition AS A FUNCTION OF ENERGY, on the device.

`flux_averaged_BSMu` (golemflavor/fr.py:441-457) evaluates `u_to_fr(source, params_to_BSMu(..., energy=E_k))` at the centre of every
energy bin and returns only the width-weighted mean; the new-physics term grows as E^(d-3), so the composition per bin shows where
in energy the texture takes over, which the mean hides.  `Model.propagate_bins` returns the per-bin terms themselves (csrc/gf_spectrum.hip,
bit for bit the terms of the average); `DeviceEnsembleSampler.spectrum` / `NestedSampler.spectrum` reduce them over a stored chain /
the posterior rows without anything but the results crossing PCIe, by the marginals' own reduction with the energy bins in place of
the chains (`marginals.py` states every definition):
  counts       np.histogram(f, bins, range=(0, 1)) per energy bin and flavour;
  percentiles  np.percentile's default `linear` rule on two exact order statistics;
  nvalid, mean, cov (ddof 1)   over the samples that have a composition.
A sample the reference would have raised on (fr.py:398-399: inside flux_averaged_BSMu at the first failing bin) has no composition
at ANY energy: NaN in every bin, left out of every reduction.  DESIGN.md 6g.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GF_MARGINAL_MAX_RANKS, check
from .marginals import percentile_from_order_statistics

FLAVOURS = ("fr_e", "fr_mu", "fr_tau")


def bin_tables(edges):
    """(energies, widths) of bin edges b: the centres sqrt(b_k b_{k+1}) (fr.py:413) and |b_{k+1} - b_k| (fr.py:414)."""
    b = np.asarray(edges, dtype=np.float64)
    if b.ndim != 1 or len(b) < 2:
        raise ValueError("edges must be a 1-D array of at least two bin edges")
    return np.sqrt(b[:-1] * b[1:]), np.abs(np.diff(b))


def model_edges(model):
    """The energy bin edges of a BSM `Model` (or of a posterior that carries one); ValueError for a model without bins."""
    m = getattr(model, "model", model)
    if int(m.mode) != _lib.GF_MODE_BSM_GAUSS or int(m.desc.nbins) < 1:
        raise ValueError("the energy-resolved composition needs a BSM model (mode BSM_GAUSS, with energy bins)")
    return np.array(m.desc.bin_edges[:int(m.desc.nbins) + 1], dtype=np.float64)


class SpectrumResult:
    """One chain's composition per energy bin.

    energies, widths (nbinsE,), edges (nbinsE + 1,); nvalid (nbinsE,) samples with a composition; mean (nbinsE, 3), cov (nbinsE, 3, 3);
    percentile_q (nq,), percentiles (nbinsE, 3, nq); hist_edges (bins + 1,) = np.linspace(0, 1, bins + 1), counts (nbinsE, 3, bins)
    uint64; order_ranks / order_stats (nbinsE, 3, 2 nq): the order statistics the percentiles were interpolated from."""

    ARRAYS = ("energies", "edges", "widths", "nvalid", "mean", "cov", "percentile_q", "percentiles", "hist_edges", "counts", "order_ranks",
              "order_stats")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def flux_average(self):
        """The flux-averaged composition of the mean spectrum, recombined as fr.py:454-457: sum over the bins of mean x width,
        times 1 / (b_N - b_0), normalised to unit sum."""
        integrated = np.sum(np.asarray(self.mean).T * self.widths, axis=1)
        averaged = (1. / (self.edges[-1] - self.edges[0])) * integrated
        return averaged / np.sum(averaged)

    def as_arrays(self):
        out = {k: np.asarray(getattr(self, k)) for k in self.ARRAYS}
        out["names"] = np.array(FLAVOURS)
        return out

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, **self.as_arrays())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(**{k: z[k] for k in cls.ARRAYS})

    def __repr__(self):
        return "SpectrumResult(nbinsE=%d, nvalid=%s, bins=%d)" % (len(self.energies), np.asarray(self.nvalid).tolist(), self.counts.shape[-1])


def prepare(edges, percentiles=(5., 16., 50., 84., 95.), bins=50):
    """Validate the arguments and build what both entry points share: a dict with the bin tables, the percentiles and the
    histogram edges."""
    b = np.array(edges, dtype=np.float64)
    if b.ndim != 1 or not 2 <= len(b) <= _lib.GF_MAX_BINS + 1:
        raise ValueError("edges must hold 2 to %d bin edges" % (_lib.GF_MAX_BINS + 1))
    if not np.all(np.isfinite(b)) or not np.all(b > 0) or not (np.all(np.diff(b) > 0) or np.all(np.diff(b) < 0)):
        raise ValueError("edges must be finite, positive and strictly monotonic")
    bins = int(bins)
    if not 1 <= bins <= 1024:
        raise ValueError("bins must lie in [1, 1024]")
    q = np.atleast_1d(np.asarray(percentiles, dtype=np.float64)).copy()
    if q.ndim != 1 or not np.all((q >= 0) & (q <= 100)):
        raise ValueError("percentiles must lie in [0, 100]")
    if 2 * len(q) > GF_MARGINAL_MAX_RANKS:
        raise ValueError("at most %d percentiles" % (GF_MARGINAL_MAX_RANKS // 2))
    energies, widths = bin_tables(b)
    return dict(edges=b, energies=energies, widths=widths, q=q, bins=bins, hist_edges=np.linspace(0., 1., bins + 1))


def run_spectrum_call(call, what, nchains, prep):
    """Drive one of the C entry points: `call(spec_pointer, out_pointer)`.  Returns [chain] SpectrumResult."""
    nE, nb, q = len(prep["energies"]), prep["bins"], prep["q"]
    R = 2 * len(q)
    a = dict(nvalid=np.zeros((nchains, nE), np.int64), mean=np.full((nchains, nE, 3), np.nan), cov=np.full((nchains, nE, 3, 3), np.nan),
             ostat=np.full((nchains, nE, 3, R), np.nan), orank=np.full((nchains, nE, 3, R), -1, np.int64),
             counts=np.zeros((nchains, nE, 3, nb), np.uint64))
    spec = _lib.GfSpectrumSpec(nb, len(q), q.ctypes.data_as(_lib._dp))
    ptr = {np.dtype(np.uint64): _lib._up, np.dtype(np.int64): _lib._lp, np.dtype(np.float64): _lib._dp}
    out = _lib.GfSpectrumOut(**{name: a[name].ctypes.data_as(ptr[a[name].dtype]) for name, _ in _lib.GfSpectrumOut._fields_})
    check(call(C.byref(spec), C.byref(out)), what)
    results = []
    for ch in range(nchains):
        pct = np.full((nE, 3, len(q)), np.nan)
        for k in range(nE):
            n = int(a["nvalid"][ch, k])
            for c in range(3):
                for j in range(len(q)):
                    pct[k, c, j] = percentile_from_order_statistics(n, q[j], a["ostat"][ch, k, c, 2 * j], a["ostat"][ch, k, c, 2 * j + 1])
        results.append(SpectrumResult(energies=prep["energies"], edges=prep["edges"], widths=prep["widths"], nvalid=a["nvalid"][ch],
                                      mean=a["mean"][ch], cov=a["cov"][ch], percentile_q=q, percentiles=pct, hist_edges=prep["hist_edges"],
                                      counts=a["counts"][ch], order_ranks=a["orank"][ch], order_stats=a["ostat"][ch]))
    return results


def rows_spectrum_host(fr_bins, edges, percentiles=(5., 16., 50., 84., 95.), bins=50):
    """`SpectrumResult` of host compositions fr_bins (n, nbinsE, 3) by numpy alone: the statement the device results are tested
    against, and the path they replace.  Rows with a NaN are left out."""
    prep = prepare(edges, percentiles, bins)
    f = np.asarray(fr_bins, dtype=np.float64)
    nE, q, nb = len(prep["energies"]), prep["q"], prep["bins"]
    if f.ndim != 3 or f.shape[1:] != (nE, 3):
        raise ValueError("fr_bins must be (n, %d, 3)" % nE)
    good = f[~np.isnan(f).any(axis=(1, 2))]
    n = len(good)
    nvalid = np.full(nE, n, np.int64)
    mean, cov = np.full((nE, 3), np.nan), np.full((nE, 3, 3), np.nan)
    pct, counts = np.full((nE, 3, len(q)), np.nan), np.zeros((nE, 3, nb), np.uint64)
    for k in range(nE):
        x = good[:, k, :]
        if n:
            mean[k] = x.mean(axis=0)
            if len(q):
                pct[k] = np.percentile(x, q, axis=0).T
        if n > 1:
            cov[k] = np.cov(x.T, ddof=1)
        for c in range(3):
            counts[k, c] = np.histogram(x[:, c], bins=nb, range=(0., 1.))[0]
    return SpectrumResult(energies=prep["energies"], edges=prep["edges"], widths=prep["widths"], nvalid=nvalid, mean=mean, cov=cov,
                          percentile_q=q, percentiles=pct, hist_edges=prep["hist_edges"], counts=counts,
                          order_ranks=np.zeros((nE, 3, 0), np.int64), order_stats=np.zeros((nE, 3, 0)))
