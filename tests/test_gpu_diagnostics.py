"""GPU: the chain diagnostics (csrc/gf_diag.hip, golemflavor_amd.diagnostics) against the host build of the same arithmetic
(tests/diag/diag_host.cpp, which tests/test_diagnostics_host.py pins to numpy and bounds against np.longdouble): every output bit
for bit, whatever the shape, the stacking of a sampler or the entry point."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import diag_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import diagnostics as dg
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import scan
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

CASES = H.cases() + [((16384, 12, 6), None)]
IDS = ["%dx%dx%d" % s for s, _ in CASES]


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


def as_fields(r):
    return {f: getattr(r, f) for f in H.FIELDS}


@pytest.mark.parametrize("shape,x", CASES, ids=IDS)
def test_device_equals_the_host_build_bit_for_bit(model, shape, x):
    if x is None:
        x = H.ar1_chain(shape, 7, phis=(0.9,))
    got = dg.chain_diagnostics(x, model=model, want_rho=True)
    assert got.nsteps == shape[0] and got.nwalkers == shape[1]
    H.assert_same_bits(as_fields(got), H.host_diag(x), str(shape))
    if shape[0] > 70:
        for maxlag in (1, 64):
            H.assert_same_bits(as_fields(dg.chain_diagnostics(x, model=model, maxlag=maxlag, want_rho=True)), H.host_diag(x, maxlag=maxlag),
                               "%s maxlag %d" % (shape, maxlag))


def test_excluded_series_on_the_device(model):
    x = CASES[3][1].copy()
    x[:, 5, 2] = 0.25
    x[17, 3, 0] = np.nan
    x[:, :, 1] = np.arange(14)[None, :]
    got = dg.chain_diagnostics(x, model=model, want_rho=True)
    assert list(got.nexcluded) == [1, 14, 1, 0] and np.isnan(got.tau[1])
    H.assert_same_bits(as_fields(got), H.host_diag(x), "excluded")


def test_series_limit_and_argument_errors(model):
    x = np.zeros((16385, 2, 1))
    spec, out = _lib.GfDiagSpec(5.0, -1), _lib.GfDiagOut()
    call = lambda n, nw, nd, sp: model._L.gf_chain_diagnostics(model._h, x.ctypes.data_as(_lib._dp), n, nw, nd, C.byref(sp), C.byref(out))  # noqa: E731
    assert call(16385, 2, 1, spec) == _lib.GF_ERR_UNSUPPORTED
    assert call(1, 2, 1, spec) == _lib.GF_ERR_INVALID_ARG and call(8, 0, 1, spec) == _lib.GF_ERR_INVALID_ARG
    assert call(8, 2, 17, spec) == _lib.GF_ERR_INVALID_ARG and call(8, 2, 0, spec) == _lib.GF_ERR_INVALID_ARG
    assert call(8, 2, 1, _lib.GfDiagSpec(0.0, -1)) == _lib.GF_ERR_INVALID_ARG and call(8, 2, 1, _lib.GfDiagSpec(5.0, 8)) == _lib.GF_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="thin"):
        dg.chain_diagnostics(x, model=model)
    d = model.alloc(8 * 16385 * 2)
    try:
        assert model._L.gf_chain_diagnostics_device(model._h, d.ptr, 0, 1, 16385, 2, 1, C.byref(spec), C.byref(out)) == _lib.GF_ERR_UNSUPPORTED
    finally:
        d.free()


# ---- sampled chains ----------------------------------------------------------------------------------------------------------------
NW, NSTEPS = 100, 600


@pytest.fixture(scope="module")
def notebook():
    """The notebook posterior sampled as one chain and as chain 1 of a three-chain sampler, 300 steps of burn-in then 600 stored."""
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02))
    np.random.seed(4)
    p0 = np.stack([mcmc_utils.flat_seed(ps, NW) for _ in range(3)])
    one = mcmc_utils.DeviceEnsembleSampler(NW, 6, m, seed=8)
    three = mcmc_utils.DeviceEnsembleSampler(NW, 6, m, nchains=3, seed=8, stream_ids=[5, 0, 9])
    for s, p in ((one, p0[1]), (three, p0)):
        s.run_mcmc(p, 300, storechain=False)
        s.run_mcmc(None, NSTEPS)
    yield m, one, three
    one.close()
    three.close()
    m.close()


def fetched(s):
    out = np.empty((s.nchains, s.nstored, s.k, s.dim))
    return s.chain_to_host(out)


def test_stacking_does_not_matter(notebook):
    m, one, three = notebook
    for round_ in range(2):
        a, b = fetched(one), fetched(three)
        assert a.shape == (1, NSTEPS + 100 * round_, NW, 6) and np.array_equal(a[0], b[1]), "the two samplers hold different chains"
        r1, r3 = one.diagnostics(want_rho=True), three.diagnostics(want_rho=True)
        assert len(r3) == 3 and r1.nsteps == a.shape[1]
        H.assert_same_bits(as_fields(r1), as_fields(r3[1]), "stacked, round %d" % round_)
        H.assert_same_bits(as_fields(r1), as_fields(dg.chain_diagnostics(a[0], model=m, want_rho=True)), "fetched, round %d" % round_)
        assert np.array_equal(r1.acceptance_fraction, r3[1].acceptance_fraction) and r1.acceptance_fraction.shape == (NW,)
        assert np.array_equal(r1.acceptance_fraction, one.acceptance_fraction)
        for k in (0, 2):
            assert not np.array_equal(r3[k].tau, r1.tau)
        if round_ == 0:
            # a second run with thin = 3: 100 more stored steps, the chain's capacity is no longer its length
            for s in (one, three):
                s.run_mcmc(None, 300, thin=3)


def test_notebook_chain_has_converged_and_matches_acor():
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02))
    np.random.seed(4)
    s = mcmc_utils.DeviceEnsembleSampler(NW, 6, m, seed=8)
    try:
        with pytest.raises(ValueError, match="no stored samples"):
            s.diagnostics()
        s.run_mcmc(mcmc_utils.flat_seed(ps, NW), 300, storechain=False)
        s.run_mcmc(None, NSTEPS)
        r = s.diagnostics()
        print("notebook chain: tau %s tau_mean %s rhat %s ess %s" % (r.tau, r.tau_mean, r.rhat, r.ess))
        assert r.converged(10) and np.all(r.nexcluded == 0) and r.rho is None
        h = NSTEPS // 2                                          # B >= 0, so rhat^2 >= (h - 1) / h
        assert np.all(np.isfinite(r.rhat)) and np.all(r.rhat >= np.sqrt((h - 1) / h) * (1 - 1e-12))
        acor = s.get_autocorr_time(tol=10)
        assert np.all(np.abs(r.tau_mean - acor) <= H.FFT_TOL), (r.tau_mean, acor)
        assert np.array_equal(np.asarray(r.ess), NW * NSTEPS / r.tau)
    finally:
        s.close()
        m.close()


def test_bsm_sampler_equals_the_host_build():
    ps7 = Cf.texture_paramset(6)
    kw = dict(texture=Texture.OET, dimension=6, binning=Cf.default_bin_edges(), source_ratio=(0., 1., 0.), bestfit_fr=(1 / 3, 1 / 3, 1 / 3),
              smearing=0.02)
    m = Model(compile_model(ps7, "BSM_GAUSS", **kw))
    rng = np.random.default_rng(2)
    box = np.array(ps7.seeds, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(14, 7))
    p0[:, 6] = rng.uniform(-56, -38, 14)
    s = mcmc_utils.DeviceEnsembleSampler(14, 7, m, seed=3)
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(p0, 193)
        r = s.diagnostics(want_rho=True)
        H.assert_same_bits(as_fields(r), H.host_diag(fetched(s)[0]), "BSM sampler")
    finally:
        s.close()
        m.close()


def test_scan_writes_diagnostics_of_every_point(model, tmp_path, capsys):
    d = str(tmp_path / "scan")
    scan.main(["--config", "C4", "--points", "4", "--nwalkers", "128", "--burnin", "10", "--nsteps", "40", "--datadir", d, "--diagnostics"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["diagnostics"]["points"] == 4 and line["diagnostics"]["seconds"] > 0 and 0 <= line["diagnostics"]["not_converged"] <= 4
    chains = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert len(chains) == 4 and sorted(os.listdir(d)) == sorted(chains + ["diagnostics_%s.npz" % f[:-4] for f in chains])
    bad = 0
    for f in chains:
        z = np.load(os.path.join(d, "diagnostics_%s.npz" % f[:-4]))
        rows = np.load(os.path.join(d, f))
        assert rows.shape == (128 * 40, 9)
        want = dg.chain_diagnostics(rows[:, 3:].reshape(40, 128, 6), model=model)
        arrays = want.as_arrays()
        assert set(z.files) == set(arrays) | {"acceptance_fraction", "acceptance_mean", "acceptance_min", "never_moved"}
        for k in arrays:
            assert np.array_equal(z[k], arrays[k], equal_nan=True), (f, k)
        acc = z["acceptance_fraction"]
        assert acc.shape == (128,) and z["acceptance_mean"] == acc.mean() and z["acceptance_min"] == acc.min() and z["never_moved"] == (acc == 0).sum()
        bad += not want.converged(50)
    assert line["diagnostics"]["not_converged"] == bad
