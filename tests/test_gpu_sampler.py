"""GPU: the device-resident stretch-move sampler (gf_sampler_*)."""
import numpy as np
import pytest

from common import BIN_EDGES, bsm_args, notebook_sets, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.enums import Texture
from stretch_ref import reference_stretch as _reference_stretch

pytestmark = pytest.mark.gpu


def test_device_sampler_equals_reference_stretch_move(golden, oracle):
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    om = oracle.make_model(ps, "SM_GAUSS", bestfit_fr=golden["g6_bestfit_fr"], smearing=0.02)
    rng = np.random.default_rng(3)
    nchains, nwalkers, nsteps, seed = 2, 32, 12, 0x1234567890ABCDEF
    p0 = np.stack([uniform_theta(ps, nwalkers, rng, seeds=True) for _ in range(nchains)])
    s = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, f, nchains=nchains, seed=seed)
    s.run_mcmc(p0, nsteps)
    ref_chain, ref_lnp, ref_acc = _reference_stretch(oracle, om, p0, nsteps, seed)
    got = s.chain.transpose(0, 2, 1, 3)                       # -> (chain, step, walker, dim)
    assert got.shape == ref_chain.shape
    assert np.abs(got - ref_chain).max() < 1e-12              # same accept decisions, same proposals
    assert np.array_equal(np.round(s.acceptance_fraction * nsteps).astype(int), ref_acc)
    assert 0.15 < ref_acc.mean() / nsteps < 0.8
    pos, lnp = s.state
    assert np.allclose(lnp, ref_lnp, rtol=1e-12)
    # reproducible: same seed, same chain; another seed, another chain
    s2 = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, f, nchains=nchains, seed=seed)
    s2.run_mcmc(p0, nsteps)
    assert np.array_equal(s2.chain, s.chain)
    s3 = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, f, nchains=nchains, seed=seed + 1)
    s3.run_mcmc(p0, nsteps)
    assert not np.array_equal(s3.chain, s.chain)
    for x in (s, s2, s3):
        x.close()
    f.close()


def test_stacked_grid_sampler_one_posterior_per_chain(golden, oracle):
    """all grid points of a GPU advance in one launch per half-step, each chain with its own
    posterior (here: three best-fit points / smearings of the notebook posterior)."""
    _, ps = notebook_sets(golden)
    from golemflavor_amd.descriptor import compile_model
    from golemflavor_amd.model import Model
    pts = [((1 / 3, 1 / 3, 1 / 3), 0.02), ((0.2, 0.45, 0.35), 0.05), ((0.5, 0.3, 0.2), 0.01)]
    models = [Model(compile_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=sm)) for bf, sm in pts]
    oms = [oracle.make_model(ps, "SM_GAUSS", bestfit_fr=bf, smearing=sm) for bf, sm in pts]
    rng = np.random.default_rng(8)
    nwalkers, nsteps, seed = 32, 10, 77
    p0 = np.stack([uniform_theta(ps, nwalkers, rng, seeds=True) for _ in pts])
    s = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, models, seed=seed)
    assert s.nchains == 3
    s.run_mcmc(p0, nsteps)
    ref_chain, ref_lnp, ref_acc = _reference_stretch(oracle, oms, p0, nsteps, seed)
    assert np.abs(s.chain.transpose(0, 2, 1, 3) - ref_chain).max() < 1e-12
    assert np.array_equal(np.round(s.acceptance_fraction * nsteps).astype(int), ref_acc)
    assert np.allclose(s.state[1], ref_lnp, rtol=1e-12)
    # the stored lnprob of chain ch is model ch's evaluation of the stored positions, bit for bit
    for ch, m in enumerate(models):
        again = m.lnprob(s.chain[ch].reshape(-1, 6), want_status=False).reshape(nwalkers, nsteps)
        assert np.array_equal(again, s.lnprobability[ch])
    # post-processing uses each chain's own model as well
    post = s.postprocess(want_fr=True)
    for ch, om in enumerate(oms):
        ref_fr, _ = oracle.propagate_batch(om, s.chain[ch].reshape(-1, 6))
        assert np.abs(post["fr"][ch].reshape(-1, 3) - ref_fr).max() < 1e-10
    # identical posteriors in every chain: same chain as the nchains form of the sampler
    s1 = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, [models[0]] * 3, seed=seed)
    s2 = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, models[0], nchains=3, seed=seed)
    s1.run_mcmc(p0, 40)
    s2.run_mcmc(p0, 40)                                          # 40 steps: the hipGraph path too
    assert np.array_equal(s1.chain, s2.chain) and np.array_equal(s1.lnprobability, s2.lnprobability)
    for x in (s, s1, s2):
        x.close()
    # mismatched posteriors are refused
    m4 = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=(1, 2, 0)))
    with pytest.raises(AssertionError):
        mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, [models[0], m4])
    mp = Model(compile_model(ps, "PRIOR_ONLY"))
    with pytest.raises(_lib.GolemHipError):
        mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, [models[0], mp])          # same ndim, other mode
    for m in models + [m4, mp]:
        m.close()


def test_stacked_grid_sampler_bsm_grid_points():
    """Chains with different texture / dimension / source / scale seeding in one sampler (the C5 grid)."""
    from golemflavor_amd import scan
    pts = scan.sens_grid(n_scales=2, n_sources=2)                  # 2 dims x 2 textures x 2 sources x 2 scales = 16
    jobs = [scan._SensPoint(p, g, nwalkers=64, device=0, smearing=0.3) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(64, 12, [j.f for j in jobs], seed=5)
    s.on_nonunitary = "-inf"
    p0 = np.stack([j.p0 for j in jobs])
    s.run_mcmc(p0, 40)
    ch, lp = s.chain, s.lnprobability                               # (16, 64, 40, 12), (16, 64, 40)
    assert ch.shape == (16, 64, 40, 12)
    for g, j in enumerate(jobs):
        again = j.f.model.lnprob(ch[g].reshape(-1, 12), want_status=False).reshape(64, 40)
        fin = np.isfinite(lp[g])
        assert fin.mean() > 0.5, (g, fin.mean())
        assert np.array_equal(again[fin], lp[g][fin])
    # the 16 posteriors differ: so do the chains' final lnprob levels
    assert len({float(np.round(np.nanmax(np.where(np.isfinite(x), x, np.nan)), 6)) for x in lp}) > 4
    assert 0.02 < s.acceptance_fraction.mean() < 0.9
    s.close()
    for j in jobs:
        j.f.close()


def test_bsm_sampler_lanes_per_walker_is_bitwise_neutral(monkeypatch):
    """BSM ensembles split a walker's energy bins over 2, 4 or 16 lanes (critical path nbins -> nbins/LPW);
    the in-order weighted sum makes the chain bitwise independent of that choice."""
    asimov, ps = Cf.fr_paramsets(6, (0.4444444444444444, 0.0))
    args = bsm_args(6, Texture.OET, (0., 1., 0.))
    f = llh_utils.bsm_ln_prob(args, asimov, ps, smearing=0.3, on_nonunitary="-inf")
    rng = np.random.default_rng(12)
    p0 = np.stack([uniform_theta(ps, 48, rng, seeds=True) for _ in range(3)])
    p0[:, :, 11] = rng.uniform(-52, -40, (3, 48))
    chains = {}
    monkeypatch.setenv("GF_SAMPLER_CHAIN", "0")                # the per-half-step grid kernels (ensembles this small take k_stretch_chain otherwise)
    for lpw in ("1", "2", "4", "16"):
        monkeypatch.setenv("GF_SAMPLER_LPW", lpw)
        s = mcmc_utils.DeviceEnsembleSampler(48, 12, f, nchains=3, seed=21)
        s.on_nonunitary = "-inf"
        s.run_mcmc(p0, 36)                                      # 32 steps through the graph + 4 eager
        chains[lpw] = (s.chain, s.lnprobability, s.acceptance_fraction)
        s.close()
    monkeypatch.delenv("GF_SAMPLER_LPW")
    monkeypatch.delenv("GF_SAMPLER_CHAIN")
    for lpw in ("2", "4", "16"):
        for x, y in zip(chains["1"], chains[lpw]):
            assert np.array_equal(x, y, equal_nan=True), lpw
    assert np.isfinite(chains["1"][1]).mean() > 0.5 and 0.05 < chains["1"][2].mean() < 0.9
    f.close()


@pytest.mark.parametrize("nwalkers,stacked", [(48, False), (64, True), (300, True), (600, False)])
def test_per_chain_sampler_equals_grid_sampler(monkeypatch, nwalkers, stacked):
    """Round 4: BSM ensembles of up to 1024 walkers run with ONE WORKGROUP PER CHAIN (k_stretch_chain): a block of steps per
    launch, half-steps behind a workgroup barrier, and the proposals whose unitarity the in-kernel tiers cannot settle are
    settled by the chain's own workgroup (28 nine-lane teams) before it goes on -- a chain that parks nothing never waits
    for one that does.  Same Philox counters, same evaluation, same emulated-x87 chain, same accept rule as the per-half-step
    grid kernels + k_stretch_settle (GF_SAMPLER_CHAIN=0): chain, lnprob chain, acceptance counters, the count of
    non-unitary proposals and the final state must be theirs bit for bit -- through texture OEU's failing region (parked
    proposals in most half-steps), with a half-ensemble smaller than, equal to a fraction of, and larger than one workgroup
    (600 walkers: two passes per half-step), one posterior for all chains and one per chain, across runs with thinning."""
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    rng = np.random.default_rng(31)
    box = np.array(ps.seeds, dtype=float)
    nch = 3
    if stacked:
        fs = [llh_utils.bsm_ln_prob(bsm_args(6, tex, src), asimov, ps, smearing=0.3, on_nonunitary="-inf")
              for tex, src in ((Texture.OEU, (1 / 3, 2 / 3, 0.)), (Texture.OET, (0., 1., 0.)), (Texture.OUT, (1., 0., 0.)))]
        post = fs
    else:
        fs = [llh_utils.bsm_ln_prob(bsm_args(6, Texture.OEU, (1 / 3, 2 / 3, 0.)), asimov, ps, smearing=0.3, on_nonunitary="-inf")]
        post = fs[0]
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(nch, nwalkers, 12))
    p0[:, :, 11] = rng.uniform(-40.0, -30.0, (nch, nwalkers))            # across the top of the scale range: the assert fires there
    out = {}
    for mode in ("1", "0"):                                               # one workgroup per chain / per-half-step grid kernels
        monkeypatch.setenv("GF_SAMPLER_CHAIN", mode)
        s = mcmc_utils.DeviceEnsembleSampler(nwalkers, 12, post, nchains=nch, seed=5, stream_ids=[7, 2, 40])
        s.on_nonunitary = "-inf"
        s.run_mcmc(p0, 21, storechain=False)                              # 16 + 5: two launches of the chain kernel
        nb0 = s.nonunitary_proposals
        s.reset()
        s.run_mcmc(None, 35, thin=3)
        s.run_mcmc(None, 18, thin=3)
        out[mode] = (s.chain, s.lnprobability, s.acceptance_fraction, np.array([nb0, s.nonunitary_proposals]), s.state[0], s.state[1])
        s.close()
    monkeypatch.delenv("GF_SAMPLER_CHAIN")
    for x, y in zip(out["1"], out["0"]):
        assert np.array_equal(x, y, equal_nan=True)
    assert out["1"][0].shape == (nch, nwalkers, 12 + 6, 12)
    assert out["1"][3][1] > 20                                            # the chains do live where proposals are parked and rejected
    for f in fs:
        f.close()


def test_launch_shape_is_probed_and_never_changes_the_chain(monkeypatch):
    """A BSM sampler on small ensembles has two launch shapes (one workgroup per chain; per-half-step grid kernels) whose speed
    depends on where the chains live; with no GF_SAMPLER_CHAIN in the environment every run of 128 steps or more times a block of
    each on the sampler's own chains at its start and takes the faster one; shorter runs take the last decision.  Whatever it
    picks, and through the probe itself -- blocks of one shape, then the other, then the rest -- the chain is the forced
    shapes' chain, bit for bit."""
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    f = llh_utils.bsm_ln_prob(bsm_args(6, Texture.OEU, (1 / 3, 2 / 3, 0.)), asimov, ps, smearing=0.3, on_nonunitary="-inf")
    rng = np.random.default_rng(9)
    box = np.array(ps.seeds, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(4, 64, 12))
    p0[:, :, 11] = rng.uniform(-40.0, -30.0, (4, 64))
    out = {}
    for mode in ("auto", "1", "0"):
        if mode == "auto":
            monkeypatch.delenv("GF_SAMPLER_CHAIN", raising=False)
        else:
            monkeypatch.setenv("GF_SAMPLER_CHAIN", mode)
        s = mcmc_utils.DeviceEnsembleSampler(64, 12, f, nchains=4, seed=3)
        s.on_nonunitary = "-inf"
        s.run_mcmc(p0, 30, storechain=False)                              # too short to probe: per chain, undecided
        shape0 = s.launch_shape()
        s.run_mcmc(None, 130, thin=2)                                     # probed here (auto)
        shape1 = s.launch_shape()
        s.run_mcmc(None, 40, thin=2)                                      # too short to probe again: the last decision
        out[mode] = (s.chain, s.lnprobability, s.acceptance_fraction, s.nonunitary_proposals)
        if mode == "auto":
            assert shape0["shape"] == "undecided" and shape1["shape"] in ("per chain", "grid")
            assert min(shape1["probe_us_per_16_steps"].values()) > 0.0
            assert s.launch_shape() == shape1                              # a short run keeps the decision
        s.close()
    monkeypatch.delenv("GF_SAMPLER_CHAIN", raising=False)
    for other in ("1", "0"):
        for x, y in zip(out["auto"][:3], out[other][:3]):
            assert np.array_equal(x, y, equal_nan=True), other
        assert out["auto"][3] == out[other][3]
    f.close()


def test_walker_mean_and_acor_on_device(golden):
    """mcmc.py:45-51 prints sampler.acor: the ensemble-mean series is reduced on the device."""
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    rng = np.random.default_rng(5)
    p0 = np.stack([uniform_theta(ps, 100, rng, seeds=True) for _ in range(2)])
    s = mcmc_utils.DeviceEnsembleSampler(100, 6, f, nchains=2, seed=3)      # 100 walkers: 600 elements per step, 252-thread stride
    s.run_mcmc(p0, 500, storechain=False)
    s.reset()
    s.run_mcmc(None, 3000, thin=1)
    m = s.walker_mean()
    ref = s.chain.mean(axis=1)                                               # (2, 3000, 6)
    assert m.shape == (2, 3000, 6)
    assert np.abs(m - ref).max() < 1e-13
    with pytest.raises(mcmc_utils.AutocorrError):                           # 3000 steps < 50 tau: emcee-2 refuses too
        s.acor
    tau = s.get_autocorr_time(tol=10)
    assert tau.shape == (2, 6) and np.all(np.isfinite(tau)) and np.all(tau > 20) and np.all(tau < 300)   # notebook: 85-125
    assert np.allclose(tau[0], mcmc_utils.integrated_time(ref[0], tol=10), rtol=1e-9)
    s.close()
    # 4-dim, 64 walkers (256 elements per step: full-block stride), single chain
    ps4 = Cf.unitary_paramset()
    from golemflavor_amd.descriptor import compile_model
    from golemflavor_amd.model import Model
    m4 = Model(compile_model(ps4, "PRIOR_ONLY", source_ratio=(1, 2, 0)))
    np.random.seed(2)
    s4 = mcmc_utils.DeviceEnsembleSampler(64, 4, m4, seed=9)
    s4.run_mcmc(mcmc_utils.flat_seed(ps4, 64), 37, thin=2)
    assert np.abs(s4.walker_mean() - s4.chain.mean(axis=0)).max() < 1e-13
    s4.close()
    m4.close()
    f.close()


@pytest.mark.parametrize("nwalkers,thin", [(100, 1), (36, 3), (640, 2)])
def test_persistent_workgroup_sampler_equals_grid_sampler(golden, monkeypatch, nwalkers, thin):
    """Small ensembles run one workgroup per ensemble with the walkers in LDS and the whole run in one launch;
    same random stream and arithmetic as the per-half-step grid kernels -> bitwise the same chain."""
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    rng = np.random.default_rng(nwalkers)
    nchains = 3
    p0 = np.stack([uniform_theta(ps, nwalkers, rng, seeds=True) for _ in range(nchains)])
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GF_SAMPLER_PERSIST", mode)
        s = mcmc_utils.DeviceEnsembleSampler(nwalkers, 6, f, nchains=nchains, seed=1234)
        s.run_mcmc(p0, 21, storechain=False)
        s.reset()
        s.run_mcmc(None, 40, thin=thin)
        s.run_mcmc(None, 2 * thin, thin=thin)                    # a second stored run appends
        out[mode] = (s.chain, s.lnprobability, s.acceptance_fraction, s.state[0], s.state[1])
        assert s.chain.shape == (nchains, nwalkers, (40 + thin - 1) // thin + 2, 6)
        s.close()
    monkeypatch.delenv("GF_SAMPLER_PERSIST")
    for x, y in zip(out["1"], out["0"]):
        assert np.array_equal(x, y)
    assert 0.2 < out["1"][2].mean() < 0.7
    f.close()


def test_persistent_sampler_across_launch_chunks(golden, monkeypatch):
    """A persistent run is cut into launches of <= 65536 steps; the cut must fall on a multiple of `thin`."""
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    rng = np.random.default_rng(0)
    p0 = uniform_theta(ps, 16, rng, seeds=True)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GF_SAMPLER_PERSIST", mode)
        s = mcmc_utils.DeviceEnsembleSampler(16, 6, f, seed=5)
        s.run_mcmc(p0, 66000, thin=7)
        out[mode] = (s.chain, s.lnprobability, s.acceptance_fraction)
        assert s.chain.shape == (16, (66000 + 6) // 7, 6) and s.iterations == 66000
        s.close()
    monkeypatch.delenv("GF_SAMPLER_PERSIST")
    for x, y in zip(out["1"], out["0"]):
        assert np.array_equal(x, y)
    f.close()


def test_graph_replay_equals_eager_launches(monkeypatch):
    """The per-half-step launches are replayed from a hipGraph in blocks of 16 steps; launching them one by one
    (GF_SAMPLER_NO_GRAPH) must give the same chain, also across several runs with and without storing."""
    asimov, ps = Cf.fr_paramsets(3, (0.4444444444444444, 0.0))
    f = llh_utils.bsm_ln_prob(bsm_args(3, Texture.OUT, (1., 0., 0.)), asimov, ps, smearing=0.3, on_nonunitary="-inf")
    rng = np.random.default_rng(4)
    box = np.array(ps.seeds, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(2, 48, 12))
    p0[:, :, 11] = rng.uniform(-30, -24, (2, 48))
    out = {}
    monkeypatch.setenv("GF_SAMPLER_CHAIN", "0")                # the grid kernels are what a graph replays
    for eager in (False, True):
        if eager:
            monkeypatch.setenv("GF_SAMPLER_NO_GRAPH", "1")
        s = mcmc_utils.DeviceEnsembleSampler(48, 12, f, nchains=2, seed=8)
        s.on_nonunitary = "-inf"
        s.run_mcmc(p0, 37, storechain=False)                      # 32 from the graph + 5 eager
        s.reset()
        s.run_mcmc(None, 50, thin=3)                               # graph captured again: the chain pointer changed
        s.run_mcmc(None, 40, thin=3)                               # same graph replayed
        out[eager] = (s.chain, s.lnprobability, s.acceptance_fraction)
        s.close()
    monkeypatch.delenv("GF_SAMPLER_NO_GRAPH")
    monkeypatch.delenv("GF_SAMPLER_CHAIN")
    for x, y in zip(out[False], out[True]):
        assert np.array_equal(x, y, equal_nan=True)
    assert out[False][0].shape == (2, 48, 17 + 14, 12)
    f.close()


def test_device_sampler_bookkeeping_and_reset(golden):
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    np.random.seed(26)
    p0 = mcmc_utils.flat_seed(ps, nwalkers=128)
    s = mcmc_utils.DeviceEnsembleSampler(128, 6, f, seed=7)
    s.run_mcmc(p0, 50)
    assert s.iterations == 50 and s.chain.shape == (128, 50, 6)
    s.reset()
    assert s.iterations == 0 and s.chain.shape == (128, 0, 6)
    s.run_mcmc(None, 300, thin=3)                              # continues from the burnt-in walkers
    ch, lp = s.chain, s.lnprobability
    assert ch.shape == (128, 100, 6) and lp.shape == (128, 100) and s.iterations == 300
    # the stored lnprob is the kernel's own evaluation of the stored position, bit for bit
    again = f.model.lnprob(ch.reshape(-1, 6), want_status=False).reshape(128, 100)
    assert np.array_equal(again, lp)
    # walkers never leave the prior box, -inf is never accepted
    box = np.array(ps.ranges, dtype=float)
    assert np.all(ch >= box[:, 0]) and np.all(ch <= box[:, 1]) and np.all(np.isfinite(lp))
    acc = s.acceptance_fraction
    assert acc.shape == (128,) and 0.3 < acc.mean() < 0.55
    s.close()
    f.close()


def test_device_sampler_recovers_truncated_gaussian_priors():
    """PRIOR_ONLY posterior of the 12-dim paramset = product of (truncated) Gaussians and boxes with
    known moments (scripts/fr.py:30-58)."""
    _, ps = Cf.fr_paramsets(6, (0.4444, 0.0))
    f = llh_utils.prior_ln_prob(ps)
    np.random.seed(1)
    p0 = np.stack([mcmc_utils.flat_seed(ps, 256) for _ in range(4)])
    s = mcmc_utils.DeviceEnsembleSampler(256, 12, f, nchains=4, seed=99)
    s.run_mcmc(p0, 600, storechain=False)
    s.run_mcmc(None, 1500, thin=5)
    flat = s.flatchain.reshape(-1, 12)
    names = list(ps.names)
    for name, mu, sig in (("s_12_2", 0.307, 0.013), ("c_13_4", (1 - 0.02206) ** 2, 0.00147), ("m21_2", 7.40e-23, 2.1e-24),
                          ("m3x_2", 2.494e-21, 3.3e-23), ("convNorm", 1.0, 0.4)):
        x = flat[:, names.index(name)]
        assert x.mean() == pytest.approx(mu, abs=0.08 * sig + 1e-30), name
        assert x.std() == pytest.approx(sig, rel=0.08), name
    # uniform columns fill their box: dcp ~ U(0, 2pi), logLam ~ U(-56, -30)
    d = flat[:, names.index("dcp")]
    assert d.mean() == pytest.approx(np.pi, abs=0.15) and d.std() == pytest.approx(2 * np.pi / np.sqrt(12), rel=0.08)
    ll = flat[:, names.index("logLam")]
    assert ll.min() >= -56 and ll.max() <= -30 and ll.std() == pytest.approx(26 / np.sqrt(12), rel=0.1)
    s.close()
    f.close()


def test_mcmc_driver_device_resident(golden, capsys):
    """mcmc.mcmc() with the reference's signature, device-resident and host-driven, on the notebook posterior.  Both are held
    to the posterior's REFERENCE widths (a long device chain), not to each other: round 2's one-off failure of this test
    (device std 0.062 against host std 0.110 on sin^4 phi_S) was one walker of the host run trapped in the posterior's
    secondary mode at sin^4 phi_S -> 0, a pure nu_tau source -- lnprob -385 against -302, behind a valley of -450 that the
    stretch move crosses only with z ~ 1/2; one walker in a hundred there turns 0.063 into sqrt(0.063^2 + 0.01 * 0.92^2) =
    0.111 (profiles/r03/flaky_sampler_test_explained.txt).  Either sampler does that in ~2 % of runs; so the bulk is compared
    with the reference and the trapped fraction is bounded separately."""
    asimov, ps = notebook_sets(golden)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    # reference widths: 2048 walkers, 1000 burn-in + 3000 steps thinned by 5 (the long-chain numbers of the profile file: rel 3 %)
    rng = np.random.default_rng(5)
    box = np.array(ps.seeds, dtype=float)
    ref_s = mcmc_utils.DeviceEnsembleSampler(2048, 6, f, seed=3)
    ref_s.run_mcmc(rng.uniform(box[:, 0], box[:, 1], size=(2048, 6)), 1000, storechain=False)
    ref_s.reset()
    ref_s.run_mcmc(None, 3000, thin=5)
    ref = ref_s.flatchain
    ref_s.close()
    ref = ref[ref[:, 4] > 0.3]                                     # the bulk (a trapped walker sits at sin^4 phi_S < 0.01)
    ref_mean, ref_std = ref.mean(axis=0), ref.std(axis=0)
    assert np.allclose(ref_std, [0.0122, 0.0015, 0.0469, 1.3258, 0.0627, 0.0522], rtol=0.03)
    assert np.allclose(ref_mean, [0.2998, 0.9564, 0.5816, 3.1432, 0.9223, 0.9362], atol=0.05 * ref_std)

    def check(samples, label):
        trapped = samples[:, 4] < 0.3
        assert trapped.mean() <= 0.02 + 1e-9, (label, trapped.mean())  # at most two walkers of the hundred
        bulk = samples[~trapped]
        for d in range(6):
            assert abs(bulk[:, d].mean() - ref_mean[d]) < 0.1 * ref_std[d], (label, d)
            assert bulk[:, d].std() == pytest.approx(ref_std[d], rel=0.08), (label, d)

    np.random.seed(26)
    p0 = mcmc_utils.flat_seed(ps, nwalkers=100)
    samples = mcmc_utils.mcmc(p0=p0, ln_prob=f, ndim=6, nwalkers=100, burnin=400, nsteps=1500)   # LnProb -> device-resident
    out = capsys.readouterr().out
    assert samples.shape == (100 * 1500, 6)
    acc = float(out.split("sum of acceptance fraction")[1].split()[0]) / 100
    assert 0.36 < acc < 0.50                                   # reference notebook: 0.427
    assert f.ncalls == 0                                       # no host-driven evaluations at all
    check(samples, "device-resident")
    # the host-driven sampler (one launch + PCIe round trip per half-ensemble) on the same posterior
    np.random.seed(26)
    host = mcmc_utils.mcmc(p0=p0, ln_prob=f, ndim=6, nwalkers=100, burnin=400, nsteps=1500, device_resident=False)
    capsys.readouterr()
    assert f.ncalls > 0
    check(host, "host-driven")
    # a trapped walker is recognised as such: put one into the corner mode by hand and the bulk comparison still holds
    p1 = p0.copy()
    p1[0] = [0.35, 0.957, 0.74, 2.76, 0.0006, -0.81]           # a walker of the profile file's census (lnprob -385.6)
    np.random.seed(27)
    dev2 = mcmc_utils.mcmc(p0=p1, ln_prob=f, ndim=6, nwalkers=100, burnin=400, nsteps=1500)
    capsys.readouterr()
    assert (dev2[:, 4] < 0.3).mean() == pytest.approx(0.01, abs=1e-9)   # that walker stays where it is ...
    assert dev2[:, 4].std() > 1.5 * ref_std[4]                 # ... and inflates the naive width as in the recorded failure
    check(dev2, "device-resident, one walker trapped")
    f.close()


def test_device_sampler_bsm_posterior():
    asimov, ps = Cf.fr_paramsets(6, (0.4444444444444444, 0.0))
    args = bsm_args(6, Texture.OET, (0., 1., 0.))
    f = llh_utils.bsm_ln_prob(args, asimov, ps, smearing=0.05, on_nonunitary="-inf")
    rng = np.random.default_rng(2)
    p0 = uniform_theta(ps, 64, rng, seeds=True)
    p0[:, 11] = rng.uniform(-52, -46, 64)
    s = mcmc_utils.DeviceEnsembleSampler(64, 12, f, seed=11)
    s.run_mcmc(p0, 40)
    ch, lp = s.chain, s.lnprobability
    again = f.model.lnprob(ch.reshape(-1, 12), want_status=False).reshape(64, 40)
    fin = np.isfinite(lp)
    assert np.array_equal(again[fin], lp[fin])
    box = np.array(ps.ranges, dtype=float)
    assert np.all(ch >= box[:, 0]) and np.all(ch <= box[:, 1])
    assert 0.02 < s.acceptance_fraction.mean() < 0.9
    s.close()
    f.close()


def test_chain_postprocessing_on_device(golden, oracle):
    """fr of every stored sample + the flavor histogram of plot.flavor_contour, without the chain crossing PCIe."""
    ps = Cf.unitary_paramset()
    src = np.array([1., 2., 0.]) / 3
    from golemflavor_amd.descriptor import compile_model
    from golemflavor_amd.model import Model
    m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=src))
    np.random.seed(3)
    p0 = np.stack([mcmc_utils.flat_seed(ps, 64) for _ in range(2)])
    s = mcmc_utils.DeviceEnsembleSampler(64, 4, m, nchains=2, seed=4)
    s.run_mcmc(p0, 200, thin=2)
    nb = 26
    post = s.postprocess(want_fr=True, want_status=True, nbins=nb)
    ch = s.chain                                                  # (2, 64, 100, 4)
    assert post["fr"].shape == (2, 64, 100, 3) and post["hist"].shape == (2, nb, nb, nb)
    om = oracle.make_model(ps, "PRIOR_ONLY", source_ratio=src)
    ref_fr, _ = oracle.propagate_batch(om, ch.reshape(-1, 4))
    assert np.abs(post["fr"].reshape(-1, 3) - ref_fr).max() < 1e-10      # mc_unitary.py:189-193
    assert np.all(post["status"] == 0)
    for c in range(2):
        want, _ = np.histogramdd(post["fr"][c].reshape(-1, 3), bins=(nb, nb, nb), range=((0, 1),) * 3)
        assert np.array_equal(post["hist"][c], want.astype(np.uint64))     # plot.py:365-370
        assert post["hist"][c].sum() == 64 * 100
    # propagate each chain with ANOTHER model than it was sampled with (mc_texture.py:216-221): per-chain source
    srcs = [np.array([1., 0., 0.]), np.array([0., 1., 0.])]
    pms = [Model(compile_model(ps, "PRIOR_ONLY", source_ratio=x)) for x in srcs]
    post2 = s.postprocess(want_fr=True, models=pms, step_major=True)
    flat = s.flat_steps()                                         # (2, 100*64, 4), same order as post2
    assert post2["fr"].shape == (2, 100, 64, 3) and flat.shape == (2, 6400, 4)
    assert np.array_equal(np.sort(flat[0], axis=0), np.sort(s.flatchain[0], axis=0))
    for c, x in enumerate(srcs):
        ref2, _ = oracle.propagate_batch(oracle.make_model(ps, "PRIOR_ONLY", source_ratio=x), flat[c])
        assert np.abs(post2["fr"][c].reshape(-1, 3) - ref2).max() < 1e-10
    assert np.abs(post2["fr"][0] - post2["fr"][1]).max() > 0.05
    with pytest.raises(ValueError):
        s.postprocess(models=pms[:1])
    for x in pms:
        x.close()
    # stand-alone histogram entry point, edge cases: 1.0 lands in the last bin, outside / NaN dropped
    pts = np.array([[0., 0., 1.], [1., 0., 0.], [0.5, 0.5, 0.], [1.0000001, 0., 0.], [-1e-9, .5, .5], [np.nan, .1, .9],
                    [1 / 3, 1 / 3, 1 / 3]])
    want, _ = np.histogramdd(pts[[0, 1, 2, 6]], bins=(5, 5, 5), range=((0, 1),) * 3)
    assert np.array_equal(m.flavor_histogram(pts, 5), want.astype(np.uint64))
    s.close()
    m.close()


def test_multinest_style_cube_adapter(golden, oracle):
    """mn.py:26-45: unit cube -> scanned params, other columns fixed, batched.  Pinned on the oracle: theta is mapped
    on the host exactly as mn.py:33-39 writes it and handed to the oracle's llh.ln_prob."""
    asimov, ps = Cf.fr_paramsets(6, (0.4444444444444444, 0.0))
    args = bsm_args(6, Texture.OET, (0., 1., 0.))
    f = llh_utils.bsm_ln_prob(args, asimov, ps, smearing=0.05, on_nonunitary="-inf")
    ps["logLam"].value = -50.0                                     # sens.py fixes the scale per evaluation
    from golemflavor_amd.param import ParamSet
    mn_ps = ParamSet([p for p in ps if p.name != "logLam"])
    g = llh_utils.CubeLnProb(f, mn_ps, ps)
    rng = np.random.default_rng(8)
    cube = rng.uniform(0.3, 0.7, size=(50, 11))
    out = g(cube)
    lo = np.array(mn_ps.ranges)[:, 0]; hi = np.array(mn_ps.ranges)[:, 1]
    theta = np.column_stack([(hi - lo) * cube + lo, np.full(50, -50.0)])
    assert g.on_device                                             # the map ran in gf_lnprob_cube_batch ...
    assert np.array_equal(out, f(theta))                           # ... and is bitwise mn.py:36's expression
    # ... and the values are the reference's: the oracle on the host-mapped theta (mn.py:33-39 -> llh.ln_prob)
    pr = mn_ps.ranges
    theta_ref = np.array([[(pr[i][1] - pr[i][0]) * c[i] + pr[i][0] for i in range(11)] + [-50.0] for c in cube])
    from golemflavor_amd import fr as fr_host
    om = oracle.make_model(ps, "BSM_GAUSS", texture="OET", dimension=6, binning=args.binning, source_ratio=(0., 1., 0.),
                           bestfit_fr=fr_host.angles_to_fr((0.4444444444444444, 0.0)), smearing=0.05)
    ref, ref_st = oracle.lnprob_batch(om, theta_ref, want_status=True)
    assert np.all(ref_st == 0) and np.isfinite(ref).all()
    assert np.abs(out - ref).max() <= 1e-10 * np.abs(ref).max()
    assert g(list(cube[3]), 11, 11) == out[3]
    with pytest.raises(AssertionError):
        g(cube[0], 10, 10)
    # a scanned subset in another column order, and a wider scan box than the model's (host map then)
    sub = ParamSet([ps["astroNorm"], ps["s_23_2"], ps["dcp"]])
    g2 = llh_utils.CubeLnProb(f, sub, ps)
    assert g2.on_device
    c2 = rng.uniform(0.2, 0.8, size=(300, 3))
    th2 = np.tile(np.array(ps.values, dtype=float), (300, 1))
    for k, name in enumerate(["astroNorm", "s_23_2", "dcp"]):
        r = ps[name].ranges
        th2[:, list(ps.names).index(name)] = (r[1] - r[0]) * c2[:, k] + r[0]
    assert np.array_equal(g2(c2), f(th2), equal_nan=True)
    from golemflavor_amd.param import Param
    wide = ParamSet([Param(name="dcp", value=1.0, ranges=[0., 3.0], tag=ps["dcp"].tag)])
    g3 = llh_utils.CubeLnProb(f, wide, ps)
    assert not g3.on_device
    th3 = np.tile(np.array(ps.values, dtype=float), (20, 1))
    th3[:, 3] = 3.0 * c2[:20, 0]
    assert np.array_equal(g3(c2[:20, :1]), f(th3), equal_nan=True)
    # argument checks of the C entry point
    L = _lib.lib()
    import ctypes as C
    cols = (C.c_int32 * 2)(3, 3)
    base = np.array(ps.values, dtype=float)
    outb = np.empty(4)
    assert L.gf_lnprob_cube_batch(f.model._h, c2.ctypes.data_as(_lib._dp), 4, 2, cols, base.ctypes.data_as(_lib._dp),
                                  outb.ctypes.data_as(_lib._dp), None, None) == _lib.GF_ERR_INVALID_ARG   # duplicate column
    f.close()




def test_bsm_sampler_unitarity_through_the_failing_region(oracle):
    """A 12-column chain of texture OEU seeded across the top of its scale range, where the reference's unitarity assert
    fires (fr.py:461-499).  Every proposal's verdict is settled ON THE DEVICE before its accept step: most by the half-step
    kernel itself (SM-weight bound, fp64 estimate), the undecided ones by k_stretch_settle, which replays the reference's
    arithmetic in emulated x87.  So with on_nonunitary='-inf' the chain is the chain of a host-driven run in which those
    proposals score -inf.  Checked against the numpy stretch move on the same Philox stream, evaluated by the ORACLE with the
    oracle's verdicts, proposal by proposal (the proposals bit-identical to the device's: its fused multiply-add is restated
    exactly): every accept decision agrees.  Where the oracle's residual lies within half a decade of 1e-7 the reference's own
    verdict is a property of its libm's last bits; there the proposal's verdict is the host build of the
    device's chain (tests/x87_harness.py: x87t_walker_residuals on the model's own tables), independent of the device, and the
    device must take the same decision.  The number of non-unitary proposals agrees with the oracle's up to the band.  `raise`
    (the reference's behaviour): the run dies."""
    import x87_harness as H
    from stretch_ref import Arbiter, accept_lhs, propose
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    src = (1 / 3, 2 / 3, 0.)
    args = bsm_args(6, Texture.OEU, src)
    rng = np.random.default_rng(4)
    box = np.array(ps.seeds, dtype=float)
    nw, nsteps, seed, a, ndim = 64, 40, 11, 2.0, 12
    nhalf = nw // 2
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(nw, ndim))
    p0[:, 11] = rng.uniform(-40.0, -30.0, nw)
    f = llh_utils.bsm_ln_prob(args, asimov, ps, smearing=0.3, on_nonunitary="-inf")
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, f, seed=seed)
    smp.run_mcmc(p0, nsteps)
    got = smp.chain.transpose(1, 0, 2)                                   # (step, walker, dim)
    got_lnp = smp.lnprobability.T
    nbad_dev = smp.nonunitary_proposals
    om = oracle.make_model(ps, "BSM_GAUSS", texture="OEU", dimension=6, binning=BIN_EDGES, source_ratio=src,
                           bestfit_fr=fr_utils.angles_to_fr(inj), smearing=0.3)
    pos = p0.copy()
    lp, st = oracle.lnprob_batch(om, pos, want_status=True)
    lnp = np.where(st == oracle.NON_UNITARY, -np.inf, lp)                # a start the reference would have died on
    nbad, nband, nforced, naccept = int(np.sum(st == oracle.NON_UNITARY)), 0, 0, 0
    hx = H.build()
    arb = Arbiter(oracle, om, f.model, harness=hx)                       # band proposals: the harness decides (arb.nflip: overrules)
    key = (seed & 0xffffffff, seed >> 32)
    for it in range(nsteps):
        for half in (0, 1):
            t = 2 * it + half
            q, zz, u3 = propose(oracle, key, pos, half, t, a=a)                # q = fma(-z, c_j - s_k, c_j), as the kernel forms it
            lq, sq = oracle.lnprob_batch(om, q, want_status=True)
            bad, band, acquit = arb.verdict(q, sq)
            if acquit.size:                                              # the oracle did not finish these: the model's value
                lq[acquit] = f.model.lnprob(q[acquit])[0]
            lq = np.where(bad, -np.inf, lq)
            nbad += int(np.sum(sq == oracle.NON_UNITARY))
            nband += int(band.sum())
            idx = np.arange(half * nhalf, (half + 1) * nhalf)
            acc = accept_lhs(zz, u3, ndim) > lnp[idx] - lq
            want = np.where(acc[:, None], q, pos[idx])
            dev = got[it][idx]
            differ = np.abs(dev - want).max(axis=1) > 1e-12
            assert not np.any(differ), "step %d half %d: decisions differ (residuals %s, band %s)" % (it, half, res[differ], band[differ])
            nforced += int(differ.sum())
            pos[idx] = dev                                                # (= want wherever they agree)
            lnp[idx] = np.where(differ, got_lnp[it][idx], np.where(acc, lq, lnp[idx]))
            naccept += int(acc.sum())
    assert nbad > 500 and naccept > 200                                  # the chain does live in the failing region, and moves
    nflip = arb.nflip
    print("band proposals %d, harness verdict differs from the oracle's on %d" % (nband, nflip))
    assert nforced == 0 and nflip <= nband and abs(nbad_dev - nbad) <= nband, (nbad_dev, nbad, nband, nforced, nflip)
    assert np.allclose(smp.state[1], lnp, rtol=1e-10)
    # no stored sample is one the reference would have died on, except a start position that never moved (or a band case)
    st = oracle.lnprob_batch(om, got.reshape(-1, ndim), want_status=True)[1].reshape(nsteps, nw)
    moved = np.any(got != p0[None], axis=2)
    assert np.sum((st == oracle.NON_UNITARY) & moved) <= nflip * nsteps
    smp.close()
    g = llh_utils.bsm_ln_prob(args, asimov, ps, smearing=0.3)              # on_nonunitary="raise", the reference's behaviour
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, g, seed=seed)
    with pytest.raises(AssertionError, match="not unitary"):
        smp.run_mcmc(p0, nsteps)
    smp.close()
    f.close()
    g.close()
