"""The Python row-set layer (golemflavor_amd/rowsets.py) and the scan's writers on it, without a device: stand-ins for the models, the
sources and the sampler.  What is pinned here is the bookkeeping a device test meets only by chance -- handles in order, the defaults
spelled once, the element-space refusals, each source's rule for the axes it drops, and the one place (`scan.per_point`) that undoes
the single-chain rule -- at one set and at several."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from golemflavor_amd import configs as Cf
from golemflavor_amd import contour, rowsets, scan
from golemflavor_amd.mcmc import DeviceEnsembleSampler
from golemflavor_amd.nested import NestedSampler
from golemflavor_amd.reweight import Reweighted


def source(cls, **attrs):
    """an instance of a source class without its device object"""
    s = object.__new__(cls)
    s.__dict__.update(attrs)
    return s


# ---- handles, defaults, element space ---------------------------------------------------------------------------------------------
def test_handle_of_a_model_and_of_a_posterior_that_carries_one():
    model = SimpleNamespace(_h=C.c_void_p(0x1000))
    assert rowsets.handle(model) is model._h
    assert rowsets.handle(SimpleNamespace(model=model)) is model._h
    h = rowsets.handle(SimpleNamespace(_h=0x2000))
    assert isinstance(h, C.c_void_p) and h.value == 0x2000


def test_model_handles():
    assert rowsets.model_handles(None, 3) is None
    models = [SimpleNamespace(_h=C.c_void_p(0x10)), SimpleNamespace(model=SimpleNamespace(_h=C.c_void_p(0x20))), SimpleNamespace(_h=0x30)]
    arr = rowsets.model_handles(models, 3)
    assert isinstance(arr, C.c_void_p * 3) and list(arr) == [0x10, 0x20, 0x30]
    for n in (2, 4):                                   # a list too long for the chains, and one too short
        with pytest.raises(ValueError) as err:
            rowsets.model_handles(models, n)
        assert str(err.value) == "3 post-processing models for %d chains" % n


def test_sample_columns():
    desc = SimpleNamespace(lo=[-1., 0., 2., 99.], hi=[1., 0.5, 3., 99.])
    assert rowsets.sample_columns(desc, 3, False) == (["theta0", "theta1", "theta2"], [(-1., 1.), (0., 0.5), (2., 3.)])
    assert rowsets.sample_columns(desc, 3, True) == (["fr_e", "fr_mu", "fr_tau", "theta0", "theta1", "theta2"],
                                                     [(0., 1.)] * 3 + [(-1., 1.), (0., 0.5), (2., 3.)])


def test_element_space_refusals():
    ps = Cf.texture_paramset(6)
    plan, names, ranges = rowsets.element_space(ps, 7, True)
    assert len(names) == len(ranges) == 12 and plan is not None
    for kw in (dict(with_fr=True), dict(models=[object()])):
        with pytest.raises(ValueError):
            rowsets.element_space(ps, 7, True, **kw)
    with pytest.raises(ValueError):
        rowsets.element_space(None, 7, True)
    with pytest.raises(ValueError):
        rowsets.element_space(ps, 6, True)


# ---- each source's rule for the axes it drops ----------------------------------------------------------------------------------------
def sets(n):
    """a per-set list and an array with a leading set axis, set k recognisable"""
    return ["set%d" % k for k in range(n)], np.arange(n * 2 * 3).reshape(n, 2, 3)


def test_the_stored_chain_drops_the_axis_of_a_single_chain():
    lst, arr = sets(1)
    one = source(DeviceEnsembleSampler, nchains=1)
    assert one._shape(lst) == "set0" and np.array_equal(one._shape(arr), arr[0])
    lst, arr = sets(3)
    three = source(DeviceEnsembleSampler, nchains=3)
    assert three._shape(lst) == lst and three._shape(arr) is arr
    assert (one._nsets, three._nsets) == (1, 3)


def test_the_nested_sampler_never_drops_the_run_axis():
    for n in (1, 3):
        lst, arr = sets(n)
        s = source(NestedSampler, nruns=n, bases=np.zeros((n, 4)))
        assert s._shape(lst) == lst and s._shape(arr) is arr
        assert (s._nsets, s._ncols, s.ndim) == (n, 4, 4)


@pytest.mark.parametrize("nchains,ntargets", [(1, 2), (2, 1), (2, 2), (1, 1), (3, 1)])
def test_the_reweighted_chain_nests_chain_then_target(nchains, ntargets):
    r = source(Reweighted, nchains=nchains, ntargets=ntargets, ndim=5)
    lst, arr = sets(nchains * ntargets)
    assert (r._nsets, r._ncols) == (nchains * ntargets, 5)
    nested = [["set%d" % (c * ntargets + t) for t in range(ntargets)] for c in range(nchains)]
    got_l, got_a = r._shape(lst), r._shape(arr)
    if nchains == 1:
        assert got_l == nested[0] and got_a.shape == (ntargets, 2, 3) and np.array_equal(got_a, arr)
    else:
        assert got_l == nested and got_a.shape == (nchains, ntargets, 2, 3)
        assert all(np.array_equal(got_a[c, t], arr[c * ntargets + t]) for c in range(nchains) for t in range(ntargets))


def test_the_shared_bodies_hand_every_source_the_same_calls():
    """`_intervals` on stand-in libraries: the entry point by name, the source's leading arguments in front, its number of sets and
    width, and the result in the source's layout"""
    seen = []

    def entry(name):
        def fn(*args):
            seen.append((name, args[:-2]))
            return 0
        return fn
    lib = SimpleNamespace(**{n: entry(n) for n in ("gf_sampler_intervals", "gf_nested_intervals", "gf_sampler_reweight_intervals")})
    desc = SimpleNamespace(lo=[0.] * 4, hi=[1.] * 4)
    one = source(DeviceEnsembleSampler, nchains=1, dim=4, _L=lib, _h="h", model=SimpleNamespace(desc=desc), models=None)
    one._C = C
    res = one._intervals(one._lead(None), (68., 90.), True)
    assert res["low"].shape == (7, 2) and res["nunique"].shape == (7,) and list(res["percentiles"]) == [68., 90.]
    runs = source(NestedSampler, nruns=1, bases=np.zeros((1, 4)), _L=lib, _h="n", models=[SimpleNamespace(desc=desc)])
    assert runs._intervals(("n", 65), (68.,), False)["low"].shape == (1, 4, 1)
    rw = source(Reweighted, nchains=2, ntargets=3, ndim=4, _L=lib, sampler=one, _spec=C.c_int(0))
    assert rw._intervals(("h", "spec", 65), (68.,), False)["status"].shape == (2, 3, 4, 1)
    assert seen == [("gf_sampler_intervals", ("h", None, 1)), ("gf_nested_intervals", ("n", 65, 0)),
                    ("gf_sampler_reweight_intervals", ("h", "spec", 65, 0))]
    one._h = runs._h = None                            # nothing for close() to destroy


# ---- the scan's writers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [[5], [2, 5, 7]])
def test_per_point(order):
    n = len(order)
    lst = ["r%d" % k for k in range(n)]
    assert scan.per_point(lst[0] if n == 1 else lst, order) == lst
    nested = [["r%d_t%d" % (k, t) for t in range(2)] for k in range(n)]                 # [chain][target]
    assert scan.per_point(nested[0] if n == 1 else nested, order) == nested
    full = dict(low=np.arange(n * 3 * 2.).reshape(n, 3, 2), nunique=np.arange(n * 3).reshape(n, 3), percentiles=np.array([68., 90.]))
    res = {k: (v if k == "percentiles" or n > 1 else v[0]) for k, v in full.items()}   # as `intervals` returns it
    got = scan.per_point(res, order)
    assert len(got) == n
    for k, d in enumerate(got):
        assert sorted(d) == sorted(full) and d["percentiles"] is full["percentiles"]
        assert np.array_equal(d["low"], full["low"][k]) and np.array_equal(d["nunique"], full["nunique"][k])


class _Saved:
    """a result that saves itself, as MarginalResult and SpectrumResult do"""
    nvalid = np.array([30])

    def save(self, path):
        np.savez(path, x=np.zeros(1))

    def as_arrays(self):
        return {"acceptance_fraction": np.array([0.5, 0.])}

    def converged(self, tol):
        return False


class _Sampler:
    """what a writer sees of a `DeviceEnsembleSampler` of `nchains` chains; results take the sampler's own single-chain rule"""
    nstored, k, dim = 4, 8, 2
    model = SimpleNamespace(desc=SimpleNamespace(lo=[0., 0.], hi=[1., 1.]))

    def __init__(self, nchains):
        self.nchains = nchains

    _shape = DeviceEnsembleSampler._shape

    def regions(self, nbins, coverage, **kw):
        row = [contour.RegionResult(4, c, 1 + q, False, 0.5, 0.4, 0.9, np.arange(1 + q), np.ones(1 + q)) for q, c in enumerate(coverage)]
        return self._shape([row] * self.nchains)

    def marginals(self, **kw):
        return self._shape([_Saved() for _ in range(self.nchains)])

    spectrum = diagnostics = marginals

    def intervals(self, percentiles, with_fr, models):
        w = self.dim + 3 * with_fr
        res = dict(low=np.zeros((self.nchains, w, len(percentiles))), status=np.ones((self.nchains, w, len(percentiles)), np.int32))
        return dict({k: self._shape(v) for k, v in res.items()}, percentiles=np.array(percentiles))

    def reweight(self, targets, on_nonunitary):
        nc, T = self.nchains, len(targets)
        rw = source(Reweighted, nchains=nc, ntargets=T, bestfit_fr=np.zeros((nc, T, 3)), smearing=np.zeros((nc, T)), offset=np.zeros((nc, T)),
                    _summary=dict(ess=np.zeros((nc, T)), n=np.full(nc, 32)))
        rw.marginals = lambda N, **kw: rw._shape([_Saved() for _ in range(nc * T)])
        return rw


WRITERS = {
    "regions": (lambda d, name: scan.RegionWriter(d, name, [90., 99.]), ["contour_region_%s.npz"],
                ["coverage", "bins_per_axis", "hist_smooth", "points", "seconds", "thres_min", "thres_max"]),
    "marginals": (lambda d, name: scan.MarginalWriter(d, name, elements=lambda g: SimpleNamespace(ranges=[(0., 1.), (0., float(g % 2))])),
                  ["marginals_%s.npz", "marginals_elements_%s.npz"], ["bins", "points", "seconds"]),
    "diagnostics": (scan.DiagnosticsWriter, ["diagnostics_%s.npz"], ["points", "seconds", "tol", "not_converged"]),
    "intervals": (scan.IntervalWriter, ["intervals_%s.npz"], ["percentiles", "points", "seconds", "status_not_ok"]),
    "spectrum": (scan.SpectrumWriter, ["spectrum_%s.npz"], ["percentiles", "bins", "points", "seconds", "samples_without_composition"]),
    "reweight": (lambda d, name: scan.ReweightWriter(d, name, [((1 / 3,) * 3, 0.05), ((1 / 3,) * 3, 0.02)], nrows=10),
                 ["reweight_%s.npz", "reweight_marginals_%s_t0.npz", "reweight_marginals_%s_t1.npz"],
                 ["targets", "points", "seconds", "rows", "targets_without_posterior"]),
}


@pytest.mark.parametrize("key", list(WRITERS))
@pytest.mark.parametrize("order", [[5], [2, 5, 7]])
def test_every_writer_takes_one_chain_and_several(key, order, tmp_path):
    make, files, stat_keys = WRITERS[key]
    d = tmp_path / "out"
    w = make(str(d), lambda g: "p%d" % g)
    assert w.key == key and w.stats() == {} and w.points == 0
    models = None if key == "reweight" else [object()] * len(order)
    w.take(_Sampler(len(order)), models, order)
    assert sorted(p.name for p in d.iterdir()) == sorted(f % ("p%d" % g) for f in files for g in order)
    assert list(w.stats()) == stat_keys and w.points == len(order)
    w.take(_Sampler(len(order)), models, order)
    st = w.stats()
    assert w.points == st["points"] == 2 * len(order) and st["seconds"] == round(w.seconds, 4)
    n = 2 * len(order)
    own = {"regions": ("thres_max", [1, 2]), "diagnostics": ("not_converged", n), "intervals": ("status_not_ok", n * 5 * 2),
           "spectrum": ("samples_without_composition", n * 2), "reweight": ("targets_without_posterior", n * 2), "marginals": ("bins", [100, 50])}
    assert st[own[key][0]] == own[key][1]
    if key == "intervals":
        with np.load(d / ("intervals_p%d.npz" % order[-1])) as z:
            assert z["low"].shape == (5, 2) and list(z["names"]) == ["fr_e", "fr_mu", "fr_tau", "theta0", "theta1"]


def test_reweight_writer_without_rows_saves_the_summaries_alone(tmp_path):
    for order in ([5], [2, 5, 7]):
        d = tmp_path / ("n%d" % len(order))
        w = scan.ReweightWriter(str(d), str, [((1 / 3,) * 3, None)])
        w.take(_Sampler(len(order)), None, order)
        assert sorted(p.name for p in d.iterdir()) == ["reweight_%d.npz" % g for g in order]
        with np.load(d / ("reweight_%d.npz" % order[0])) as z:
            assert sorted(z.files) == ["ess", "n", "target_bestfit_fr", "target_offset", "target_smearing"] and z["ess"].shape == (1,)
