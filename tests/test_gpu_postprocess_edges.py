"""The sampler's chain post-processing (csrc/gf_postprocess.hip) where its eight entry points were written one after the other and
do not agree: what each does with an empty chain, and that a refused `models` argument leaves the sampler usable."""
import ctypes as C

import numpy as np
import pytest

from common import BIN_EDGES, notebook_sets, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import diagnostics as dg
from golemflavor_amd import elements as el
from golemflavor_amd import intervals as iv
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model
from golemflavor_amd import spectrum as sp
from golemflavor_amd.reweight import Measurement, Reweighted

pytestmark = pytest.mark.gpu

NCHAINS, NWALKERS, NDIM, NBINS = 3, 16, 7, 5
MARGINAL_KW = dict(bins_1d=4, bins_2d=3, coverage=(90.,), percentiles=(50.,))
MARGINAL_OUTPUTS = ("counts1", "counts2", "nvalid", "mean", "cov", "ncol", "order_ranks", "order_stats", "percentiles", "r1_thres",
                    "r1_saturated", "r1_level_in", "r1_level_out", "r1_mass", "r1_cells", "r1_density", "r2_thres", "r2_saturated",
                    "r2_level_in", "r2_level_out", "r2_mass", "r2_cells", "r2_density")


@pytest.fixture(scope="module")
def bsm7():
    """(paramset, posterior) of the 7-dimensional BSM model: mc_texture.py's columns with the scale sampled"""
    ps = Cf.texture_paramset(6)
    desc = compile_model(ps, "BSM_GAUSS", texture=Texture.OET, dimension=6, binning=BIN_EDGES, source_ratio=(0., 1., 0.),
                         bestfit_fr=(1 / 3,) * 3, smearing=0.02)
    f = llh_utils.LnProb(desc, device=0, on_nonunitary="-inf")
    yield ps, f
    f.close()


def digest(a):
    """an array as plain Python that == compares exactly, NaN included: [shape, the one value every element has] or
    [shape, every element]"""
    a = np.asarray(a)
    vals = [repr(x) for x in a.reshape(-1).tolist()]
    return [list(a.shape), vals[0] if vals and all(v == vals[0] for v in vals) else vals]


def rc_of(call):
    """(return code, result) of a wrapper that raises GolemHipError on a non-zero code"""
    try:
        return _lib.GF_OK, call()
    except _lib.GolemHipError as exc:
        return exc.code, None


def region_digest(res):
    return {f: digest([[getattr(r, f) for r in row] for row in res]) for f in ("thres", "saturated", "level_in", "level_out", "mass")} | {
        "cells": digest([[len(r.flat_cells) for r in row] for row in res])}


def marginal_digest(res):
    per_chain = [r.as_arrays() for r in res]
    same_shape = {k: len({a[k].shape for a in per_chain}) == 1 for k in MARGINAL_OUTPUTS}          # r2_cells: as wide as the largest region
    return {k: digest(np.stack([a[k] for a in per_chain])) if same_shape[k] else [digest(a[k]) for a in per_chain] for k in MARGINAL_OUTPUTS}


def handles_of(models):
    return (C.c_void_p * len(models))(*[m._h.value for m in models])


def observe(s, f, ps, models):
    """every entry point once on sampler s: {name: [return code, what it returned]}.  models: a list of Models or None"""
    L, h, m = _lib.lib(), s._h, f.model
    dp, ip, up = _lib._dp, _lib._ip, C.POINTER(C.c_uint64)
    hm = handles_of(models) if models is not None else None
    ns = s.nstored
    n = NCHAINS * ns * NWALKERS
    out = {}
    d_fr, d_st, d_rows = m.alloc(max(n, 1) * 24), m.alloc(max(n, 1) * 4), m.alloc(max(n, 1) * 8 * (3 + NDIM))
    for name in ("gf_sampler_postprocess", "gf_sampler_postprocess_with"):
        if name == "gf_sampler_postprocess" and models is not None:
            continue
        fr, st = np.full((NCHAINS, ns, NWALKERS, 3), -7.0), np.full((NCHAINS, ns, NWALKERS), -7, np.int32)
        counts = np.full((NCHAINS, NBINS, NBINS, NBINS), 77, np.uint64)
        args = (fr.ctypes.data_as(dp), st.ctypes.data_as(ip), NBINS, counts.ctypes.data_as(up))
        rc = L.gf_sampler_postprocess(h, *args) if name == "gf_sampler_postprocess" else L.gf_sampler_postprocess_with(h, hm, *args)
        out[name] = [rc, {"counts": digest(counts)}]
    out["gf_sampler_postprocess_device"] = [L.gf_sampler_postprocess_device(h, hm, d_fr.ptr, d_st.ptr), None]
    out["gf_sampler_postprocess_rows_device"] = [L.gf_sampler_postprocess_rows_device(h, hm, d_rows.ptr), None]
    rows = np.full((NCHAINS, ns * NWALKERS, 3 + NDIM), -7.0)
    out["gf_sampler_postprocess_rows"] = [L.gf_sampler_postprocess_rows(h, hm, rows.ctypes.data_as(dp)), None]
    rc, res = rc_of(lambda: s.regions(NBINS - 1, [90., 99.], models=models))
    out["gf_sampler_regions"] = [rc, region_digest(res) if res is not None else None]
    for with_fr in (False, True):
        rc, res = rc_of(lambda: s.marginals(with_fr=with_fr, models=models, **MARGINAL_KW))
        out["gf_sampler_marginals with_fr=%d" % with_fr] = [rc, marginal_digest(res) if res is not None else None]
    if models is None:
        rc, res = rc_of(lambda: s.marginals(space="elements", llh_paramset=ps, **MARGINAL_KW))
        out["gf_sampler_element_marginals"] = [rc, marginal_digest(res) if res is not None else None]
    for d in (d_fr, d_st, d_rows):
        d.free()
    return out


def interval_digest(res):
    return {k: digest(res[k]) for k in iv.FIELDS}


class _NoSummary(Reweighted):
    """a Reweighted whose making calls nothing: the entry points are called one by one below"""

    def _run_summary(self):
        return {"nonunitary": np.zeros((self.nchains, self.ntargets), np.int64)}


def observe_more(s, f, ps):
    """the entry points added since `observe` was written, once each on sampler s with the sampling models: {name: [return code, what
    it returned]}.  They are called below the wrappers that refuse an empty chain in Python."""
    L, h, m = _lib.lib(), s._h, f.model
    ns = s.nstored
    out = {}
    for with_fr in (0, 1):
        rc, res = rc_of(lambda: iv.run_interval_call(lambda spec, o: L.gf_sampler_intervals(h, None, with_fr, spec, o), "gf_sampler_intervals",
                                                     NCHAINS, 3 * with_fr + NDIM, (68., 90.)))
        out["gf_sampler_intervals with_fr=%d" % with_fr] = [rc, interval_digest(res) if res is not None else None]
    plan, pnames, _ = el.element_plan(ps)
    rc, res = rc_of(lambda: iv.run_interval_call(lambda spec, o: L.gf_sampler_element_intervals(h, C.byref(plan), spec, o),
                                                 "gf_sampler_element_intervals", NCHAINS, len(pnames), (68., 90.)))
    out["gf_sampler_element_intervals"] = [rc, interval_digest(res) if res is not None else None]
    prep = sp.prepare(sp.model_edges(m), (16., 84.), 4)
    rc, res = rc_of(lambda: sp.run_spectrum_call(lambda spec, o: L.gf_sampler_spectrum(h, None, spec, o), "gf_sampler_spectrum", NCHAINS, prep))
    out["gf_sampler_spectrum"] = [rc, {k: digest(np.stack([getattr(r, k) for r in res])) for k in ("nvalid", "mean", "cov", "order_ranks",
                                                                                                  "order_stats", "counts")} if res is not None else None]
    a = dict(tau=np.full((NCHAINS, NDIM), -7.0), tau_mean=np.full((NCHAINS, NDIM), -7.0), rhat=np.full((NCHAINS, NDIM), -7.0),
             window=np.full((NCHAINS, NDIM), -7, np.int64), window_mean=np.full((NCHAINS, NDIM), -7, np.int64),
             nexcluded=np.full((NCHAINS, NDIM), -7, np.int32))
    ptr = {np.dtype(np.int64): _lib._lp, np.dtype(np.int32): _lib._ip, np.dtype(np.float64): _lib._dp}
    dout = _lib.GfDiagOut(**{name: a[name].ctypes.data_as(ptr[a[name].dtype]) for name, _ in _lib.GfDiagOut._fields_ if name in a})
    rc = L.gf_sampler_diagnostics(h, C.byref(_lib.GfDiagSpec(5.0, -1)), C.byref(dout))
    out["gf_sampler_diagnostics"] = [rc, {k: digest(v) for k, v in a.items()} if rc == _lib.GF_OK else None]
    r = _NoSummary(s, [Measurement(bestfit_fr=(0.30, 0.36, 0.34)), Measurement(bestfit_fr=(1 / 3,) * 3, smearing=0.05)], seed=7, on_nonunitary="-inf")
    rc, res = rc_of(lambda: Reweighted._run_summary(r))
    out["gf_sampler_reweight"] = [rc, {k: digest(v) for k, v in res.items()} if res is not None else None]
    d_rows = m.alloc(NCHAINS * 2 * 5 * 8 * (3 + NDIM))
    out["gf_sampler_reweight_rows_device"] = [L.gf_sampler_reweight_rows_device(h, C.byref(r._spec), 5, 1, d_rows.ptr), None]
    d_rows.free()
    rc, res = rc_of(lambda: r.marginals(5, **MARGINAL_KW))
    out["gf_sampler_reweight_marginals"] = [rc, marginal_digest([x for per in res for x in per]) if res is not None else None]
    rc, res = rc_of(lambda: r.intervals(5))
    out["gf_sampler_reweight_intervals"] = [rc, interval_digest(res) if res is not None else None]
    rc, res = rc_of(lambda: r.regions(5, NBINS - 1, [90., 99.]))
    out["gf_sampler_reweight_regions"] = [rc, region_digest([x for per in res for x in per]) if res is not None else None]
    assert ns == s.nstored
    return out


# What commit 7c9bd98 (the parent of the change that moved these entry points into gf_postprocess.hip and onto one chain loop)
# returned for a sampler that has stored nothing: the return code of every entry point, and for regions and marginals the arrays.
def _empty_marginals(w):
    p, n = w * (w - 1) // 2, NCHAINS
    return {"counts1": [[n, w, 4], "0"], "counts2": [[n, p, 3, 3], "0"], "nvalid": [[n], "0"], "mean": [[n, w], "nan"],
            "cov": [[n, w, w], "nan"], "ncol": [[n, w], "0"], "order_ranks": [[n, w, 2], "-1"], "order_stats": [[n, w, 2], "nan"],
            "percentiles": [[n, w, 1], "nan"],
            "r1_thres": [[n, w, 1], "0"], "r1_saturated": [[n, w, 1], "False"], "r1_level_in": [[n, w, 1], "nan"],
            "r1_level_out": [[n, w, 1], "nan"], "r1_mass": [[n, w, 1], "0.0"], "r1_cells": [[n, w, 0], []], "r1_density": [[n, w, 0], []],
            "r2_thres": [[n, p, 1], "0"], "r2_saturated": [[n, p, 1], "False"], "r2_level_in": [[n, p, 1], "nan"],
            "r2_level_out": [[n, p, 1], "nan"], "r2_mass": [[n, p, 1], "0.0"], "r2_cells": [[n, p, 0], []], "r2_density": [[n, p, 0], []]}


_UNTOUCHED_COUNTS = {"counts": [[NCHAINS, NBINS, NBINS, NBINS], "77"]}           # returns before anything is written
EMPTY_CHAIN_7C9BD98 = {
    "gf_sampler_postprocess": [0, _UNTOUCHED_COUNTS],
    "gf_sampler_postprocess_with": [0, _UNTOUCHED_COUNTS],
    "gf_sampler_postprocess_device": [0, None],
    "gf_sampler_postprocess_rows_device": [0, None],
    "gf_sampler_postprocess_rows": [0, None],
    "gf_sampler_regions": [0, {"thres": [[NCHAINS, 2], "0"], "saturated": [[NCHAINS, 2], "False"], "level_in": [[NCHAINS, 2], "nan"],
                               "level_out": [[NCHAINS, 2], "nan"], "mass": [[NCHAINS, 2], "0.0"], "cells": [[NCHAINS, 2], "0"]}],
    "gf_sampler_marginals with_fr=0": [0, _empty_marginals(NDIM)],
    "gf_sampler_marginals with_fr=1": [0, _empty_marginals(3 + NDIM)],
    "gf_sampler_element_marginals": [0, _empty_marginals(12)],          # 9 moduli, logLam, the two mass splittings
}

# What commit 2dc3ca1 (the parent of the change that put these entry points on one row-set layer) returned for the entry points that
# were added after the table above was written, observed the same way.
# All of them refuse an empty chain (1 = GF_ERR_INVALID_ARG) before they write anything.
EMPTY_CHAIN_2DC3CA1 = {
    "gf_sampler_intervals with_fr=0": [1, None],
    "gf_sampler_intervals with_fr=1": [1, None],
    "gf_sampler_element_intervals": [1, None],
    "gf_sampler_spectrum": [1, None],
    "gf_sampler_diagnostics": [1, None],
    "gf_sampler_reweight": [1, None],
    "gf_sampler_reweight_rows_device": [1, None],
    "gf_sampler_reweight_marginals": [1, None],
    "gf_sampler_reweight_intervals": [1, None],
    "gf_sampler_reweight_regions": [1, None],
}


def test_empty_chain(bsm7):
    ps, f = bsm7
    s = mcmc_utils.DeviceEnsembleSampler(NWALKERS, NDIM, f, nchains=NCHAINS, seed=3)
    try:
        assert s.nstored == 0
        got = observe(s, f, ps, None)
        for k, v in got.items():
            print(k, v)
        assert got == EMPTY_CHAIN_7C9BD98
        more = observe_more(s, f, ps)
        for k, v in more.items():
            print(k, v)
        assert more == EMPTY_CHAIN_2DC3CA1
        # with stored=0 after a run the chain is as empty as before it
        p0 = np.stack([uniform_theta(ps, NWALKERS, np.random.default_rng(5 + c), seeds=True) for c in range(NCHAINS)])
        s.run_mcmc(p0, 3, storechain=False)
        assert s.nstored == 0 and observe(s, f, ps, None) == EMPTY_CHAIN_7C9BD98 and observe_more(s, f, ps) == EMPTY_CHAIN_2DC3CA1
    finally:
        s.close()


def test_rejected_models_leave_the_sampler_usable(bsm7, golden):
    ps, f = bsm7
    _, ps6 = notebook_sets(golden)
    sm6 = Model(compile_model(ps6, "SM_GAUSS", bestfit_fr=(1 / 3,) * 3, smearing=0.02))          # 6 columns: not this sampler's
    s = mcmc_utils.DeviceEnsembleSampler(NWALKERS, NDIM, f, nchains=NCHAINS, seed=3)
    try:
        p0 = np.stack([uniform_theta(ps, NWALKERS, np.random.default_rng(5 + c), seeds=True) for c in range(NCHAINS)])
        s.run_mcmc(p0, 4)
        assert s.nstored == 4
        got = observe(s, f, ps, [f.model, f.model, sm6])
        for k, v in got.items():
            print(k, v)
        assert len(got) == 7 and all(v[0] == _lib.GF_ERR_INVALID_ARG for v in got.values()), got
        assert got["gf_sampler_postprocess_with"][1] == {"counts": digest(np.full((NCHAINS, NBINS, NBINS, NBINS), 77, np.uint64))}
        # the stream and the arbitration-grid flag are as they were: a valid call goes through and gives the device route's rows
        host = s.postprocess_rows()
        d_rows = f.model.alloc(host.nbytes)
        s.postprocess_rows_to_device(d_rows.ptr)
        dev = d_rows.download(host.shape)
        d_rows.free()
        assert host.shape == (NCHAINS, 4 * NWALKERS, 3 + NDIM) and np.array_equal(host, dev, equal_nan=True)
        assert np.array_equal(host[:, :, 3:], s.flat_steps())
        # and with the sampler's own models the same entry points succeed
        ok = observe(s, f, ps, [f.model] * NCHAINS)
        assert all(v[0] == _lib.GF_OK for v in ok.values()), ok
    finally:
        s.close()
        sm6.close()
