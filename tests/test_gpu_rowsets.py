"""Every fused "reduction of every set on the device" against the composition it stands for: the source's public rows entry point, then
the stand-alone reducer on those rows, bit for bit (NaN equal to NaN).  One case per filled cell of

                       rows  marginals  intervals  element marg.  element int.  regions
    stored chain         x       x          x            x             x           x
    nested posterior     x       x          x            x             -           x
    reweighted chain     x       x          x            -             -           x

(the spectrum entry points are held to numpy on the rows in test_gpu_spectrum.py).  The rows cell holds what the other cells build on:
the with_fr rows carry the plain rows behind the composition, and every source's device rows entry point gives its host entry point's rows.

Shapes.  Stored chain: 3 chains of the 7-column BSM model of test_gpu_postprocess_edges.py, 4160 rows per chain -- one past the
4096-row leaf of the marginal and weight trees -- as 16 walkers x 260 stored steps (the sampler takes no fewer than 2 x ndim = 14
walkers), once with the sampling models and once with per-chain post-processing models.  4160 is 65 element tiles of 64 rows; the
tile's tail is met by the 65-row sets below.  Nested posterior: 3 tutorial runs, nlive 100, the slowest stopped before its tolerance
so that it has no posterior, 65 rows per run.  Reweighted chain: the same stored chain, 2 targets by measurement and 2 by model, 65
rows per (chain, target)."""
import ctypes as C

import numpy as np
import pytest

from common import BIN_EDGES, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import contour, elements
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import intervals as iv
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import nested
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model
from golemflavor_amd.reweight import Measurement

pytestmark = pytest.mark.gpu

NCHAINS, NWALKERS, NSTEPS, NDIM = 3, 16, 260, 7
N = 65
MKW = dict(bins_1d=16, bins_2d=8, coverage=(68., 90.), percentiles=(5., 50., 95.))
PCT = (68., 90.)
RBINS, RCOV = 12, (68., 90.)
REDUCTIONS = ("rows", "marginals", "intervals", "element_marginals", "element_intervals", "regions")
BSM_KW = dict(texture=Texture.OET, dimension=6, binning=BIN_EDGES, source_ratio=(0., 1., 0.), bestfit_fr=(1 / 3,) * 3, smearing=0.02)
FR_NAMES = ["fr_e", "fr_mu", "fr_tau"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


def same_marginals(got, want, tag):
    """lists of MarginalResult, every array of as_arrays()"""
    assert len(got) == len(want), tag
    for k, (g, w) in enumerate(zip(got, want)):
        a, b = g.as_arrays(), w.as_arrays()
        assert sorted(a) == sorted(b), tag
        for f in a:
            assert same(a[f], b[f]), (tag, k, f)


def same_intervals(got, want, tag):
    for f in iv.FIELDS:
        assert same(got[f], want[f]), (tag, f)


def same_regions(got, want, tag):
    """[set][coverage] RegionResult"""
    assert len(got) == len(want), tag
    for k, (rg, rw) in enumerate(zip(got, want)):
        assert len(rg) == len(rw) == len(RCOV), tag
        for g, w in zip(rg, rw):
            for f in ("thres", "saturated", "level_in", "level_out", "mass", "flat_cells", "density"):
                assert same(getattr(g, f), getattr(w, f)), (tag, k, f)


def ranges_of(desc, ndim, with_fr):
    return ([(0., 1.)] * 3 if with_fr else []) + [(desc.lo[c], desc.hi[c]) for c in range(ndim)]


def names_of(ndim, with_fr):
    return (FR_NAMES if with_fr else []) + ["theta%d" % c for c in range(ndim)]


def regions_of_rows(frows, model):
    """the stand-alone region reducer on the compositions of with_fr rows [set][n][3 + ndim]"""
    return [contour.flavor_region(x[:, :3], RBINS, RCOV, model=model) for x in frows]


def device_rows(model, shape, call):
    """what a device rows entry point, call(device pointer) -> return code, leaves in a buffer of `shape` doubles"""
    model = getattr(model, "model", model)
    d = model.alloc(int(np.prod(shape)) * 8)
    try:
        assert call(d.ptr) == _lib.GF_OK
        return d.download(shape)
    finally:
        d.free()


# ---- stored chain --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """the stored chain, its paramset and model, the per-chain post-processing models, and the reference rows of both model choices"""
    ps = Cf.texture_paramset(6)
    f = llh_utils.LnProb(compile_model(ps, "BSM_GAUSS", **BSM_KW), device=0, on_nonunitary="-inf")
    post = [Model(compile_model(ps, "BSM_GAUSS", **dict(BSM_KW, source_ratio=sr))) for sr in ((1., 2., 0.), (0., 1., 0.), (1., 0., 0.))]
    s = mcmc_utils.DeviceEnsembleSampler(NWALKERS, NDIM, f, nchains=NCHAINS, seed=3)
    p0 = np.stack([uniform_theta(ps, NWALKERS, np.random.default_rng(5 + c), seeds=True) for c in range(NCHAINS)])
    s.run_mcmc(p0, NSTEPS)
    theta = s.flat_steps()
    assert theta.shape == (NCHAINS, 4160, NDIM)
    ref = {"theta": theta, "rows": {"own": s.postprocess_rows(), "post": s.postprocess_rows(models=post)}}
    assert not same(ref["rows"]["own"][0], ref["rows"]["post"][0])                 # the post-processing models do change the rows
    yield s, f, ps, post, ref
    s.close()
    f.close()
    for m in post:
        m.close()


def chain_cell(chain, reduction, which):
    s, f, ps, post, ref = chain
    models = post if which == "post" else None
    theta, frows = ref["theta"], ref["rows"][which]
    desc, tag = f.model.desc, "stored chain, %s models, %s" % (which, reduction)
    if reduction == "rows":
        assert same(frows[:, :, 3:], theta), tag
        handles = (C.c_void_p * NCHAINS)(*[m._h.value if hasattr(m._h, "value") else m._h for m in models]) if models else None
        assert same(device_rows(f, frows.shape, lambda ptr: s._L.gf_sampler_postprocess_rows_device(s._h, handles, ptr)), frows), tag
    elif reduction == "marginals":
        for with_fr, x in ((False, theta), (True, frows)):
            rg, nm = ranges_of(desc, NDIM, with_fr), names_of(NDIM, with_fr)
            got = s.marginals(ranges=rg, with_fr=with_fr, models=models, names=nm, **MKW)
            same_marginals(got, mg.chain_marginals(x, rg, model=f, names=nm, **MKW), tag + " with_fr=%d" % with_fr)
    elif reduction == "intervals":
        for with_fr, x in ((False, theta), (True, frows)):
            got = s.intervals(percentiles=PCT, with_fr=with_fr, models=models)
            same_intervals(got, iv.chain_intervals(x, model=f, percentiles=PCT), tag + " with_fr=%d" % with_fr)
    elif reduction in ("element_marginals", "element_intervals"):
        assert models is None                      # element space propagates nothing: CELLS has no such case
        plan, pnames, pranges = elements.element_plan(ps)
        erows = elements.element_rows(theta, plan, model=f)
        if reduction == "element_marginals":
            got = s.marginals(space="elements", llh_paramset=ps, **MKW)
            same_marginals(got, mg.chain_marginals(erows, pranges, model=f, names=pnames, **MKW), tag)
        else:
            got = s.intervals(percentiles=PCT, space="elements", llh_paramset=ps)
            same_intervals(got, iv.chain_intervals(erows, model=f, percentiles=PCT), tag)
    else:
        same_regions(s.regions(RBINS, RCOV, models=models), regions_of_rows(frows, f), tag)


# ---- nested posterior ----------------------------------------------------------------------------------------------------------
def _tutorial(smearing):
    asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=smearing)
    return llh_utils.tutorial_ln_prob(asimov, ps)


@pytest.fixture(scope="module")
def runs():
    """three tutorial runs of different smearing; the one that needs the most iterations is stopped before it is done (max_iter is
    met at a check, every 4 iterations, by the runs not done): it has no posterior, the other two have theirs"""
    fs = [_tutorial(sm) for sm in (1.0, 0.12, 0.01)]
    kw = dict(nlive=100, batch=12, walks=10, seed=3, run_ids=[5, 6, 7])
    with nested.NestedSampler(fs, [0, 1], np.zeros(2), **kw) as probe:
        niter = sorted(int(x) for x in probe.run()["niter"])
    stop = -(-niter[1] // 4) * 4
    assert niter[1] <= stop < niter[2], niter
    s = nested.NestedSampler(fs, [0, 1], np.zeros(2), **kw)
    with pytest.raises(_lib.GolemHipError) as err:
        s.run(max_iter=stop)
    assert err.value.code == _lib.GF_ERR_UNSUPPORTED
    assert sorted(s.posterior()["npoints"] > 0) == [False, True, True]
    ref = {"theta": s.posterior_rows(N), "rows": s.posterior_rows(N, with_fr=True)}
    yield s, fs, ref
    s.close()
    for f in fs:
        f.close()


def nested_cell(runs, reduction):
    s, fs, ref = runs
    theta, frows = ref["theta"], ref["rows"]
    desc, tag = fs[0].model.desc, "nested posterior, %s" % reduction
    empty = int(np.flatnonzero(s.posterior()["npoints"] == 0)[0])
    if reduction == "rows":
        assert theta.shape == (3, N, 2) and same(frows[:, :, 3:], theta), tag
        assert np.isnan(frows[empty]).all() and np.isfinite(np.delete(theta, empty, axis=0)).all(), tag
        for with_fr, x in ((0, theta), (1, frows)):
            assert same(device_rows(fs[0], x.shape, lambda ptr: s._L.gf_nested_posterior_rows_device(s._h, N, with_fr, ptr)), x), (tag, with_fr)
    elif reduction == "marginals":
        for with_fr, x in ((False, theta), (True, frows)):
            rg, nm = ranges_of(desc, 2, with_fr), names_of(2, with_fr)
            got = s.marginals(N, ranges=rg, with_fr=with_fr, names=nm, **MKW)
            same_marginals(got, mg.chain_marginals(x, rg, model=fs[0], names=nm, **MKW), tag + " with_fr=%d" % with_fr)
    elif reduction == "intervals":
        for with_fr, x in ((False, theta), (True, frows)):
            got = s.intervals(N, percentiles=PCT, with_fr=with_fr)
            same_intervals(got, iv.chain_intervals(x, model=fs[0], percentiles=PCT), tag + " with_fr=%d" % with_fr)
    elif reduction == "element_marginals":
        # the tutorial's paramset names no group: the plan is built by hand, the source composition of the two angles and a copy
        plan = elements.make_plan([(elements.GF_ELEMENT_FR3, [0, 1]), (elements.GF_ELEMENT_COPY, [0])])
        rg, nm = [(0., 1.)] * 4, list(elements.FR_NAMES) + ["measured_angle1"]
        prep = mg.prepare(4, rg, nm, **MKW)

        def call(spec, out):
            return s._L.gf_nested_element_marginals(s._h, N, C.byref(plan), spec, out)
        got = mg.run_marginal_call(call, "gf_nested_element_marginals", s.nruns, prep)
        erows = elements.element_rows(theta, plan, model=fs[0])
        same_marginals(got, mg.chain_marginals(erows, rg, model=fs[0], names=nm, **MKW), tag)
    else:
        same_regions(s.regions(N, RBINS, RCOV), regions_of_rows(frows, fs[0]), tag)


# ---- reweighted chain ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reweighted(chain):
    """the stored chain under 2 measurement targets and under 2 model targets: {kind: (Reweighted, reference rows)}"""
    s, f, ps, post, _ = chain
    desc = f.model.desc
    tm = [Model(compile_model(ps, "BSM_GAUSS", **dict(BSM_KW, bestfit_fr=(0.30, 0.36, 0.34), smearing=0.05))),
          Model(compile_model(ps, "BSM_GAUSS", **dict(BSM_KW, smearing=0.03)))]
    out = {}
    for kind, targets in (("measurement", [Measurement(bestfit_fr=(0.30, 0.36, 0.34), smearing=0.05), Measurement(bestfit_fr=(1 / 3,) * 3, smearing=0.03)]), ("model", tm)):
        r = s.reweight(targets, seed=77, on_nonunitary="-inf")
        flat = lambda x: x.reshape((NCHAINS * 2,) + x.shape[2:])                   # noqa: E731  [chain][target] -> [set]
        out[kind] = (r, {"theta": flat(r.rows(N)), "rows": flat(r.rows(N, with_fr=True))})
    yield out, f, desc
    for m in tm:
        m.close()


def reweight_cell(reweighted, reduction, kind):
    out, f, desc = reweighted
    r, ref = out[kind]
    theta, frows = ref["theta"], ref["rows"]
    tag = "reweighted chain, %s targets, %s" % (kind, reduction)
    unnest = lambda res: [x for per_chain in res for x in per_chain]              # noqa: E731
    if reduction == "rows":
        assert theta.shape == (NCHAINS * 2, N, NDIM) and same(frows[:, :, 3:], theta) and np.isfinite(theta).all(), tag
        for with_fr, x in ((0, theta), (1, frows)):
            got = device_rows(f, x.shape, lambda ptr: r._L.gf_sampler_reweight_rows_device(r.sampler._h, C.byref(r._spec), N, with_fr, ptr))
            assert same(got, x), (tag, with_fr)
    elif reduction == "marginals":
        for with_fr, x in ((False, theta), (True, frows)):
            rg, nm = ranges_of(desc, NDIM, with_fr), names_of(NDIM, with_fr)
            got = unnest(r.marginals(N, ranges=rg, with_fr=with_fr, names=nm, **MKW))
            same_marginals(got, mg.chain_marginals(x, rg, model=f, names=nm, **MKW), tag + " with_fr=%d" % with_fr)
    elif reduction == "intervals":
        for with_fr, x in ((False, theta), (True, frows)):
            got = r.intervals(N, percentiles=PCT, with_fr=with_fr)
            got = {k: v.reshape((NCHAINS * 2,) + v.shape[2:]) for k, v in got.items() if k != "percentiles"}
            same_intervals(got, iv.chain_intervals(x, model=f, percentiles=PCT), tag + " with_fr=%d" % with_fr)
    else:
        same_regions(unnest(r.regions(N, RBINS, RCOV)), regions_of_rows(frows, f), tag)


CELLS = ([("chain", red, which) for which in ("own", "post") for red in REDUCTIONS if which == "own" or not red.startswith("element")] +
         [("nested", red, None) for red in REDUCTIONS if red != "element_intervals"] +
         [("reweight", red, kind) for kind in ("measurement", "model") for red in REDUCTIONS if not red.startswith("element")])


@pytest.mark.parametrize("source,reduction,variant", CELLS, ids=["%s-%s%s" % (s, r, "-" + v if v else "") for s, r, v in CELLS])
def test_fused_entry_point_equals_rows_then_reducer(source, reduction, variant, request):
    if source == "chain":
        chain_cell(request.getfixturevalue("chain"), reduction, variant)
    elif source == "nested":
        nested_cell(request.getfixturevalue("runs"), reduction)
    else:
        reweight_cell(request.getfixturevalue("reweighted"), reduction, variant)


def test_one_chain_is_chain_zero_of_three_without_the_chain_axis(chain):
    """The single-chain rule on the device path.  A sampler of one chain and chain 0 of a sampler of three, on the same random stream
    from the same start, hold the same chain; every reduction of the one-chain sampler is then that of chain 0 bit for bit, NaNs in
    place, and carries no chain axis: a result where the other has a list of results, arrays one dimension short."""
    _, f, ps, post, _ = chain
    p0 = np.stack([uniform_theta(ps, NWALKERS, np.random.default_rng(5 + c), seeds=True) for c in range(NCHAINS)])
    one = mcmc_utils.DeviceEnsembleSampler(NWALKERS, NDIM, f, nchains=1, seed=3, stream_ids=[7])
    three = mcmc_utils.DeviceEnsembleSampler(NWALKERS, NDIM, f, nchains=NCHAINS, seed=3, stream_ids=[7, 8, 9])
    try:
        one.run_mcmc(p0[0], NSTEPS)
        three.run_mcmc(p0, NSTEPS)
        assert one.flat_steps().shape == (4160, NDIM) and same(one.flat_steps(), three.flat_steps()[0])
        assert not same(three.flat_steps()[0], three.flat_steps()[1])
        spectra = 0
        for which, m1, m3 in (("own", None, None), ("post", post[:1], post)):
            a, b = one.marginals(with_fr=True, models=m1, **MKW), three.marginals(with_fr=True, models=m3, **MKW)
            assert isinstance(a, mg.MarginalResult) and isinstance(b, list) and len(b) == NCHAINS
            same_marginals([a], b[:1], "marginals, %s models" % which)
            a, b = one.intervals(percentiles=PCT, with_fr=True, models=m1), three.intervals(percentiles=PCT, with_fr=True, models=m3)
            assert a["low"].shape == (3 + NDIM, 2) and b["low"].shape == (NCHAINS, 3 + NDIM, 2) and same(a["percentiles"], b["percentiles"])
            same_intervals(a, {k: b[k][0] for k in iv.FIELDS}, "intervals, %s models" % which)
            a, b = one.regions(RBINS, RCOV, models=m1), three.regions(RBINS, RCOV, models=m3)
            assert isinstance(a[0], contour.RegionResult) and len(b) == NCHAINS
            same_regions([a], b[:1], "regions, %s models" % which)
            a, b = one.regions(RBINS, 90., models=m1), three.regions(RBINS, 90., models=m3)       # one coverage: no coverage level either
            assert isinstance(a, contour.RegionResult) and isinstance(b[0], contour.RegionResult)
            same_regions([[a] * 2], [[b[0]] * 2], "regions at one coverage, %s models" % which)
            a, b = one.spectrum(percentiles=(16, 50, 84), bins=20, models=m1), three.spectrum(percentiles=(16, 50, 84), bins=20, models=m3)
            assert not isinstance(a, list) and len(b) == NCHAINS
            for k, v in a.as_arrays().items():
                assert same(v, b[0].as_arrays()[k]), ("spectrum", which, k)
                spectra += 1
        assert spectra == 2 * 13
        a, b = one.marginals(space="elements", llh_paramset=ps, **MKW), three.marginals(space="elements", llh_paramset=ps, **MKW)
        assert isinstance(a, mg.MarginalResult) and len(b) == NCHAINS
        same_marginals([a], b[:1], "element marginals")
        a, b = one.intervals(percentiles=PCT, space="elements", llh_paramset=ps), three.intervals(percentiles=PCT, space="elements", llh_paramset=ps)
        assert a["low"].shape == b["low"].shape[1:] and b["low"].shape[0] == NCHAINS
        same_intervals(a, {k: b[k][0] for k in iv.FIELDS}, "element intervals")
    finally:
        one.close()
        three.close()
