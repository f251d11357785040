"""What the three sources of samples share on the Python side (csrc/gf_rowsets.h is the C side): the stored chain
(`mcmc.DeviceEnsembleSampler`), the nested posterior's equal-weight rows (`nested.NestedSampler`) and a reweighted chain's
(`reweight.Reweighted`) each hold some number of row sets on the device and reduce every set in one library call.  Written once
here: a model's handle, the default column names and ranges, the element-space checks, and the bodies of `marginals`, `intervals`,
`regions` and `spectrum` over the drivers `marginals.run_marginal_call`, `intervals.run_interval_call`, `contour.run_region_call`
and `spectrum.run_spectrum_call`.  A source checks what is its own and hands over (`RowSetSource`)."""
import ctypes as C

import numpy as np


def handle(m):
    """The C handle of a `Model`, or of the model of an `LnProb`, as a c_void_p."""
    h = getattr(m, "model", m)._h
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h)


def model_handles(models, n):
    """One handle per set for the entry points that take post-processing models: None for None (the sampled posteriors)."""
    if models is None:
        return None
    models = list(models)
    if len(models) != n:
        raise ValueError("%d post-processing models for %d chains" % (len(models), n))
    return (C.c_void_p * n)(*[handle(m) for m in models])


def sample_columns(desc, ndim, with_fr):
    """(names, ranges) of the rows by default: the sampled columns over the box of the descriptor, behind the composition over
    (0, 1) with with_fr (the rows a scan saves)."""
    names = (["fr_e", "fr_mu", "fr_tau"] if with_fr else []) + ["theta%d" % c for c in range(ndim)]
    return names, ([(0., 1.)] * 3 if with_fr else []) + [(desc.lo[c], desc.hi[c]) for c in range(ndim)]


def element_space(llh_paramset, ndim, round32, with_fr=False, models=None):
    """(plan, names, ranges) of `elements.element_plan(llh_paramset, round32)` for rows of ndim columns, after the checks of
    space="elements"."""
    from . import elements as el
    if with_fr:
        raise ValueError("space='elements' does not combine with with_fr: the element-space row carries the source composition")
    if models is not None:
        raise ValueError("space='elements' propagates nothing: it takes no post-processing models")
    if llh_paramset is None:
        raise ValueError("space='elements' needs llh_paramset, the set the chain was sampled over")
    if len(llh_paramset) != ndim:
        raise ValueError("llh_paramset has %d parameters, the chain %d columns" % (len(llh_paramset), ndim))
    return el.element_plan(llh_paramset, round32)


class RowSetSource:
    """The reductions of every row set of a source.  The source supplies
        _L, _prefix     the library and what its entry points' names start with ("gf_sampler_", "gf_nested_", ...)
        _sets           what it calls its sets in a message ("chains", "runs")
        _nsets, _ncols  how many sets it holds; the columns of a sample
        _desc0()        the descriptor whose box is the default ranges
        _shape(x)       a per-set list, or an array with a leading set axis, in the layout its public methods return
    and gives every body `lead`, the arguments of its entry points in front of the ones all sources share."""

    def _entry(self, name, lead):
        fn = getattr(self._L, self._prefix + name)
        return (lambda *args: fn(*lead, *args)), self._prefix + name

    def _columns(self, with_fr, elements):
        """elements: None, or (llh_paramset, round32, models) for the sets in element space.  Returns (the argument that says
        which columns, what goes in front of the entry point's name, default names, default ranges)."""
        if elements:
            plan, names, ranges = element_space(elements[0], self._ncols, elements[1], with_fr, elements[2])
            return C.byref(plan), "element_", names, ranges
        return (int(bool(with_fr)), "") + sample_columns(self._desc0(), self._ncols, with_fr)

    def _marginals(self, lead, ranges, names, with_fr, kw, elements=None):
        from . import marginals as mg
        which, pre, dnames, dranges = self._columns(with_fr, elements)
        kw = dict(kw)
        cap_2d = kw.pop("cap_2d", None)
        prep = mg.prepare(len(dnames), dranges if ranges is None else ranges, dnames if names is None else names, **kw)
        call, what = self._entry(pre + "marginals", lead + (which,))
        return self._shape(mg.run_marginal_call(call, what, self._nsets, prep, cap_2d))

    def _intervals(self, lead, percentiles, with_fr, elements=None):
        from . import intervals as iv
        which, pre, dnames, _ = self._columns(with_fr, elements)
        call, what = self._entry(pre + "intervals", lead + (which,))
        res = iv.run_interval_call(call, what, self._nsets, len(dnames), percentiles)
        return {k: (v if k == "percentiles" else self._shape(v)) for k, v in res.items()}

    def _regions(self, lead, nbins, coverage, hist_smooth, oversample, truncate, cap):
        from . import contour
        nb = int(nbins * oversample) + 1
        scalar, _ = contour._coverages(coverage)
        call, what = self._entry("regions", lead + (nb,))
        res = contour.run_region_call(call, what, self._nsets, nb, coverage, hist_smooth, truncate, cap)
        return self._shape(contour.shape_results(res, scalar, False))

    def _spectrum(self, lead, models, percentiles, bins):
        """models: the sets' models, whose energy binning must agree"""
        from . import spectrum as sp
        edges = [sp.model_edges(m) for m in models]
        if any(not np.array_equal(e, edges[0]) for e in edges[1:]):
            raise ValueError("the %s' models differ in their energy binning" % self._sets)
        call, what = self._entry("spectrum", lead)
        return self._shape(sp.run_spectrum_call(call, what, self._nsets, sp.prepare(edges[0], percentiles, bins)))
