"""GPU: the ensemble sampler under the energy-resolved Gaussian likelihood (gf_sampler_create_binned, the MODE_BSM_BINNED instance of
k_stretch / k_stretch_multi in csrc/gf_sampler.hip).  Every comparison is bit for bit: the yardstick is the bulk
kernel -- `Model.lnprob` of the same binned model, held to the reference-generated golden by tests/test_gpu_binned.py -- driven through
the numpy stretch move of tests/stretch_ref.py on the sampler's Philox stream."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from common import BIN_EDGES, bsm_args, uniform_theta
from golemflavor_amd import _lib, llh, scan
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import Param, ParamSet
from golemflavor_amd.reweight import Measurement, lnw_host
from stretch_ref import accept_lhs, propose, reference_stretch

pytestmark = pytest.mark.gpu

SRC = (1., 2., 0.)


# ---- restated from tests/test_gpu_binned.py ----------------------------------------------------------------------------------------
def paramset_of(width, dim):
    """7: the texture posterior; 12: the bulk benchmark's posterior; 11: the NP mixing angles sampled (the generic row width)"""
    if width == 7:
        return Cf.texture_paramset(dim), None
    if width == 12:
        return Cf.fr_paramsets(dim, (0.4444, 0.0))[1], None
    t = list(Cf.texture_paramset(dim))
    mm = [Param(name="np_%s" % k, value=0.5, ranges=r, tag=ParamTag.MMANGLES)
          for k, r in (("s12", [0., 1.]), ("c13", [0., 1.]), ("s23", [0., 1.]), ("dcp", [0., 2 * np.pi]))]
    return ParamSet(t[:6] + mm + t[6:]), Texture.NONE


def bsm_model(width, dim, tex, binning=BIN_EDGES, source=SRC):
    ps, forced = paramset_of(width, dim)
    kw = dict(texture=forced or tex, dimension=dim, binning=np.asarray(binning, dtype=float), source_ratio=source, bestfit_fr=(1 / 3,) * 3,
              smearing=0.02)
    return Model(compile_model(ps, "BSM_GAUSS", **kw)), ps


def a_measurement(K, binning, seed=3, smearing=0.02):
    """Dirichlet compositions well away from what the textures give, widths by the equal-information rule"""
    rng = np.random.default_rng(seed)
    return llh.BinnedMeasurement(rng.dirichlet((6, 5, 4), size=K), smearing, binning=binning)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def scale_rows(ps, n, rng, dim):
    """rows over the seeds' box with the scale in the lower 60 % of its range, below where the reference starts raising"""
    th = uniform_theta(ps, n, rng, seeds=True)
    b = Cf.SCALE_BOUNDARIES[dim]
    th[:, -1] = rng.uniform(b[0], b[0] + 0.6 * (b[1] - b[0]), n)
    return th


def binned_model(width, dim, tex, binning=BIN_EDGES, seed=3, smearing=0.02):
    m, ps = bsm_model(width, dim, tex, binning=binning)
    m.set_binned_measurement(a_measurement(len(binning) - 1, binning, seed=seed, smearing=smearing))
    return m, ps


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def bulk(model, q):
    """the bulk lnprob of the chain's binned model under the on_nonunitary="-inf" rule (a reference_stretch `lnprob`)"""
    lp, st = model.lnprob(np.ascontiguousarray(q), want_status=True)
    return np.where(st == _lib.GF_ST_NON_UNITARY, -np.inf, lp)


def device_run(smp):
    """what a run left: stored chain and lnprob in the device's order, final state, acceptance counts"""
    c, lp, nacc = smp._fetch(chain=True, lnprob=True, naccepted=True)
    pos, lnp = smp.state
    return {"chain": c, "lnp_chain": lp, "pos": pos.reshape(c.shape[0], c.shape[2], c.shape[3]), "lnp": lnp.reshape(c.shape[0], -1), "nacc": nacc}


def assert_same_run(got, ref, what):
    assert got["chain"].shape == ref["chain"].shape, (what, got["chain"].shape, ref["chain"].shape)
    differ = int(np.sum(got["chain"] != ref["chain"]))
    print("%s: %d stored values, %d differ; %d moves" % (what, ref["chain"].size, differ, int(ref["nacc"].sum())))
    assert same_bits(got["chain"], ref["chain"]), (what, differ)
    assert same_bits(got["lnp_chain"], ref["lnp_chain"]), what
    assert same_bits(got["pos"], ref["pos"]) and same_bits(got["lnp"], ref["lnp"]), what
    assert np.array_equal(got["nacc"], ref["nacc"]), what
    assert ref["nacc"].sum() > 0.1 * ref["nacc"].size, "the chain hardly moves: nothing was compared"


def run_against_reference(oracle, models, multi, p0, nsteps, seed, stream_ids=None, what=""):
    """models: one binned Model (multi False: every chain samples it) or one per chain; p0 (nchains, nwalkers, ndim)"""
    nch, nw, nd = p0.shape
    smp = mcmc_utils.DeviceEnsembleSampler(nw, nd, list(models) if multi else models[0], nchains=nch, seed=seed, stream_ids=stream_ids,
                                           energy_resolved=True)
    smp.on_nonunitary = "-inf"
    try:
        assert smp.launch_shape()["shape"] == "grid"
        smp.run_mcmc(p0 if nch > 1 else p0[0], nsteps)
        ref = reference_stretch(oracle, list(models) if multi else models[0], p0, nsteps, seed, lnprob=bulk, full=True, stream_ids=stream_ids)
        assert_same_run(device_run(smp), ref, what)
        return smp, ref
    except BaseException:
        smp.close()
        raise


# ---- 1. one posterior, k_stretch ------------------------------------------------------------------------------------------------------
def test_one_posterior_graph_replays_eager_steps_and_thinning(oracle):
    """7 columns, 32 walkers, 40 steps -- two graph replays of 16 steps and eight eager ones -- from where nothing is non-unitary; then
    reset() and 8 more at thin = 3: the iteration counter goes on, the store index starts again."""
    rng = np.random.default_rng(21)
    m, ps = binned_model(7, 6, Texture.OET)
    with m:
        p0 = scale_rows(ps, 32, rng, 6)[None]
        smp, ref = run_against_reference(oracle, [m], False, p0, 40, seed=9, what="7 columns, 40 steps")
        try:
            assert smp.nonunitary_proposals == 0 and smp.iterations == 40
            smp.reset()
            smp.run_mcmc(None, 8, thin=3)
            again = reference_stretch(oracle, m, ref["pos"], 8, 9, lnprob=bulk, full=True, iteration0=40, thin=3, lnp0=ref["lnp"])
            assert again["chain"].shape[1] == 3
            assert_same_run(device_run(smp), again, "after reset(), 8 steps at thin 3")
        finally:
            smp.close()


# ---- 2. one posterior per chain, k_stretch_multi ------------------------------------------------------------------------------------------
def test_one_posterior_per_chain_with_different_tables(oracle):
    """Three stacked 12-column posteriors on streams (5, 0, 9): different textures, different measurements and 20, 7 and 1 energy bins,
    so that nbins_max and the length of the staged table differ from chain to chain.  64 walkers, 34 steps."""
    rng = np.random.default_rng(22)
    lo, hi = Cf.DEFAULT_BINNING[0], Cf.DEFAULT_BINNING[1]
    spec = [(6, Texture.OET, 20, 4), (3, Texture.OUT, 7, 5), (6, Texture.OEU, 1, 6)]
    made = [binned_model(12, dim, tex, binning=Cf.default_bin_edges((lo, hi, K)), seed=sd) for dim, tex, K, sd in spec]
    models = [m for m, _ in made]
    try:
        assert [m.nbins for m in models] == [20, 7, 1]
        p0 = np.stack([scale_rows(ps, 64, rng, dim) for (_, ps), (dim, _, _, _) in zip(made, spec)])
        smp, _ = run_against_reference(oracle, models, True, p0, 34, seed=13, stream_ids=(5, 0, 9), what="three posteriors, 34 steps")
        smp.close()
    finally:
        for m in models:
            m.close()


# ---- 3. generic row width and ragged launches ----------------------------------------------------------------------------------------------
def test_generic_row_width_one_partial_block(oracle):
    """The 11-column Texture.NONE paramset (the NDIM = 0 instance), 300 walkers: nhalf = 150 is one partial block; 20 steps are eager."""
    rng = np.random.default_rng(23)
    m, ps = binned_model(11, 6, Texture.NONE)
    with m:
        p0 = scale_rows(ps, 300, rng, 6)[None]
        smp, _ = run_against_reference(oracle, [m], False, p0, 20, seed=17, what="11 columns, 300 walkers")
        smp.close()


def test_two_blocks_per_chain_the_last_partial(oracle):
    """12 columns, two chains of 600 walkers on one posterior: 600 proposals per half-step in three blocks, the last one partial and
    the middle one shared by the two chains; 18 steps."""
    rng = np.random.default_rng(24)
    m, ps = binned_model(12, 6, Texture.OET)
    with m:
        p0 = scale_rows(ps, 1200, rng, 6).reshape(2, 600, 12)
        smp, _ = run_against_reference(oracle, [m], False, p0, 18, seed=19, what="12 columns, 2 x 600 walkers")
        smp.close()


def test_two_blocks_per_chain_one_posterior_per_chain(oracle):
    """The same shape through k_stretch_multi: two posteriors of 600 walkers, two blocks per chain, the last one partial."""
    rng = np.random.default_rng(25)
    made = [binned_model(12, 6, tex, seed=sd) for tex, sd in ((Texture.OET, 7), (Texture.OUT, 8))]
    models = [m for m, _ in made]
    try:
        p0 = np.stack([scale_rows(ps, 600, rng, 6) for _, ps in made])
        smp, _ = run_against_reference(oracle, models, True, p0, 18, seed=19, what="12 columns, 2 posteriors x 600 walkers")
        smp.close()
    finally:
        for m in models:
            m.close()


# ---- 4. through the failing region -----------------------------------------------------------------------------------------------------
FAILING_SEED = 11


def failing_region_setup(on_nonunitary):
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    args = bsm_args(6, Texture.OEU, (1 / 3, 2 / 3, 0.))
    rng = np.random.default_rng(4)
    box = np.array(ps.seeds, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(64, 12))
    p0[:, 11] = rng.uniform(-40.0, -30.0, 64)
    f = llh.bsm_ln_prob(args, asimov, ps, smearing=0.3, on_nonunitary=on_nonunitary, binned=a_measurement(20, BIN_EDGES, seed=3, smearing=0.3))
    return f, p0


def test_through_the_failing_region_decision_by_decision(oracle):
    """The 12-column OEU chain of test_bsm_sampler_unitarity_through_the_failing_region (64 walkers, 40 steps, scale seeded over
    [-40, -30], smearing 0.3) under a binned measurement, on_nonunitary="-inf", walked proposal by proposal on the device's own
    positions: every accept decision and every stored lnprob is the one taken from the bulk kernel's value and status of the same
    proposal, and `nonunitary_proposals` is the number of proposals (and start positions) the bulk status calls non-unitary.  The
    status of a binned model is that of the model without the measurement, which tests/test_gpu_sampler.py holds to the reference.
    Conditions on the inputs, not tolerances: more than 200 moves, more than 500 non-unitary proposals, at least one proposal
    completed by k_stretch_settle (the sampler's own census, `parked_proposals`).  `raise`: the run dies."""
    nw, nsteps, seed, ndim = 64, 40, FAILING_SEED, 12
    nhalf = nw // 2
    f, p0 = failing_region_setup("-inf")
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, f, seed=seed, energy_resolved=True)
    try:
        assert smp.on_nonunitary == "-inf"
        smp.run_mcmc(p0, nsteps)
        run = device_run(smp)
        got, got_lnp = run["chain"][0], run["lnp_chain"][0]                      # (step, walker, dim), (step, walker)
        nbad_dev, parked = smp.nonunitary_proposals, smp.parked_proposals
        pos = p0.copy()
        lp, st = f.model.lnprob(pos, want_status=True)
        lnp = np.where(st == _lib.GF_ST_NON_UNITARY, -np.inf, lp)                 # a start the reference would have died on
        nbad, naccept = int(np.sum(st == _lib.GF_ST_NON_UNITARY)), 0
        key = (seed & 0xffffffff, seed >> 32)
        for it in range(nsteps):
            for half in (0, 1):
                q, zz, u3 = propose(oracle, key, pos, half, 2 * it + half)
                lq, sq = f.model.lnprob(q, want_status=True)
                bad = sq == _lib.GF_ST_NON_UNITARY
                lq = np.where(bad, -np.inf, lq)
                nbad += int(bad.sum())
                idx = np.arange(half * nhalf, (half + 1) * nhalf)
                with np.errstate(invalid="ignore"):
                    acc = accept_lhs(zz, u3, ndim) > lnp[idx] - lq
                want = np.where(acc[:, None], q, pos[idx])
                dev = got[it][idx]
                differ = np.any(dev != want, axis=1)
                assert not np.any(differ), "step %d half %d: decisions differ for slots %s (bulk status %s)" % (it, half, np.flatnonzero(differ), sq[differ])
                lnp[idx] = np.where(acc, lq, lnp[idx])
                pos[idx] = dev
                naccept += int(acc.sum())
            assert same_bits(got_lnp[it], lnp), "step %d: stored lnprob" % it       # both halves are final
        print("moves %d, non-unitary proposals %d (device %d), completed by k_stretch_settle %s" % (naccept, nbad, nbad_dev, parked))
        assert naccept > 200 and nbad > 500 and parked is not None and parked >= 1, (naccept, nbad, parked)
        assert nbad_dev == nbad
        assert same_bits(run["lnp"][0], lnp) and same_bits(run["pos"][0], pos)
        assert int(run["nacc"].sum()) == naccept
    finally:
        smp.close()
        f.close()
    g, p0 = failing_region_setup("raise")                                           # the reference's behaviour
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, g, seed=seed, energy_resolved=True)
    try:
        with pytest.raises(AssertionError, match="not unitary"):
            smp.run_mcmc(p0, nsteps)
    finally:
        smp.close()
        g.close()


# ---- 5. stored lnprob is the bulk lnprob of the stored theta ----------------------------------------------------------------------------
def test_stored_lnprob_is_the_bulk_lnprob_of_the_stored_theta():
    """8 stacked C5 points (two dimensions, two textures, the lowest and the highest scale of the grid), each with its own
    measurement; 64 walkers, 48 steps after a burn-in of 16: every stored (row, lnprob) pair is models[c].lnprob(row) bit for bit
    wherever the bulk status is OK."""
    pts = scan.sens_grid()
    picks = []
    source = sorted({p[2] for p in pts})[3]
    for dim in (3, 6):
        for tex in (Texture.OET, Texture.OUT):
            mine = [g for g, p in enumerate(pts) if p[0] == dim and p[1] is tex and p[2] == source]
            picks += [min(mine, key=lambda g: pts[g][3]), max(mine, key=lambda g: pts[g][3])]
    assert len(set(picks)) == 8
    jobs = [scan._SensPoint(pts[g], g, nwalkers=64, device=0, binned=a_measurement(20, BIN_EDGES, seed=100 + g)) for g in picks]
    smp = mcmc_utils.DeviceEnsembleSampler(64, 12, [j.f for j in jobs], seed=25, stream_ids=picks, energy_resolved=True)
    try:
        assert smp.on_nonunitary == "-inf"
        smp.run_mcmc(np.stack([j.p0 for j in jobs]), 16, storechain=False)
        smp.reset()
        smp.run_mcmc(None, 48)
        run = device_run(smp)
        assert run["chain"].shape == (8, 48, 64, 12)
        for c, j in enumerate(jobs):
            rows, stored = run["chain"][c].reshape(-1, 12), run["lnp_chain"][c].reshape(-1)
            lp, st = j.f.model.lnprob(rows, want_status=True)
            ok = st == _lib.GF_ST_OK
            print("point %d (%s): %d of %d rows OK, %d distinct" % (picks[c], pts[picks[c]], ok.sum(), len(ok), len(np.unique(stored))))
            assert ok.sum() >= 0.5 * len(ok) and len(np.unique(stored)) > 64        # (conditions on the inputs: the chain has values, and moves)
            assert same_bits(stored[ok], lp[ok]), (c, int(np.sum(stored[ok] != lp[ok])))
            assert np.all(stored[~ok] == -np.inf)                                 # a start the reference would have died on, never left
    finally:
        smp.close()
        for j in jobs:
            j.close()


# ---- 6. refusals and neighbours -----------------------------------------------------------------------------------------------------------
def flux_sampler(model):
    s = mcmc_utils.DeviceEnsembleSampler(32, 7, model, seed=31)
    s.on_nonunitary = "-inf"
    return s


def test_refusals_and_neighbours():
    rng = np.random.default_rng(26)
    L = _lib.lib()
    m, ps = binned_model(7, 6, Texture.OET, seed=5, smearing=0.05)
    flux, _ = bsm_model(7, 6, Texture.OET)
    with m, flux:
        p0 = scale_rows(ps, 32, rng, 6)
        p0[:, -1] = rng.uniform(-50.0, -42.0, 32)
        # a flux-averaged sampler alone, and one created now and run after everything below
        alone = flux_sampler(flux)
        alone.run_mcmc(p0, 24)
        chain_alone, lnp_alone = alone.chain, alone.lnprobability
        alone.close()
        before = flux_sampler(flux)
        # the keyword without a measurement; a mixture through the C entry point; the old entry point on the binned model
        with pytest.raises(ValueError, match="carries no binned measurement"):
            mcmc_utils.DeviceEnsembleSampler(32, 7, flux, seed=1, energy_resolved=True)
        h = C.c_void_p()
        rc = L.gf_sampler_create_binned((C.c_void_p * 2)(m._h, flux._h), 2, 2, 32, 5, 2.0, C.byref(h))
        assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
        assert b"model 1 carries no binned measurement" in L.gf_last_hip_error()
        rc = L.gf_sampler_create_binned((C.c_void_p * 2)(m._h, m._h), 2, 3, 32, 5, 2.0, C.byref(h))     # nmodels is 1 or nchains
        assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
        rc = L.gf_sampler_create(m._h, 1, 32, 5, 2.0, C.byref(h))
        assert rc == _lib.GF_ERR_UNSUPPORTED and not h.value and b"binned" in L.gf_last_hip_error()
        with pytest.raises(_lib.GolemHipError) as e:
            mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=1)
        assert e.value.code == _lib.GF_ERR_UNSUPPORTED

        def binned_run():
            s = mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=5, energy_resolved=True)
            s.on_nonunitary = "-inf"
            s.run_mcmc(p0, 40)
            return s
        s = binned_run()
        try:
            assert s.launch_shape()["shape"] == "grid"
            c, lp0, _ = s._fetch(chain=True, lnprob=True)
            # measurement targets: refused by the library; model targets, the flux-averaged posterior among them: as for any chain
            with pytest.raises(_lib.GolemHipError) as e:
                s.reweight([Measurement(bestfit_fr=(0.3, 0.3, 0.4))], on_nonunitary="-inf")
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED and "energy-resolved" in str(e.value)
            r = s.reweight([flux], on_nonunitary="-inf")
            rows, base = c.reshape(-1, 7), lp0.reshape(-1)
            lt, st = flux.lnprob(rows, want_status=True)
            want, kind = lnw_host(lt, base, st)
            assert np.sum(kind == 0) >= 1000 and same_bits(r.lnw(0)[0], want)
            assert r.summary()["ess"][0] > 1.0
            # the overrides of the flux-averaged sampler's launch shapes are not read: same shape, same bits
            old = {k: os.environ.get(k) for k in ("GF_SAMPLER_CHAIN", "GF_SAMPLER_LPW")}
            os.environ.update(GF_SAMPLER_CHAIN="1", GF_SAMPLER_LPW="16")
            try:
                forced = binned_run()
                try:
                    assert forced.launch_shape()["shape"] == "grid"
                    cf, lf, _ = forced._fetch(chain=True, lnprob=True)
                    assert same_bits(cf, c) and same_bits(lf, lp0)
                finally:
                    forced.close()
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            # a measurement set between two runs is the one the next run samples
            m.set_binned_measurement(a_measurement(20, BIN_EDGES, seed=6, smearing=0.05))
            s.reset()
            s.run_mcmc(None, 12)
            c2, l2, _ = s._fetch(chain=True, lnprob=True)
            lp, st = m.lnprob(c2.reshape(-1, 7), want_status=True)
            moved = np.any(c2[0] != c[0, -1][None], axis=2).reshape(-1) & (st == _lib.GF_ST_OK)
            assert moved.sum() > 20 and same_bits(l2.reshape(-1)[moved], lp[moved])
        finally:
            s.close()
        before.run_mcmc(p0, 24)
        try:
            assert same_bits(before.chain, chain_alone) and same_bits(before.lnprobability, lnp_alone)
        finally:
            before.close()


# ---- 7. the scan, end to end ----------------------------------------------------------------------------------------------------------------
def test_scan_energy_resolved_end_to_end(tmp_path, capsys):
    """scan.main --config C5 --energy-resolved with --marginals and --diagnostics: the files carry `_ebins`, every chain file is the
    chain of an energy-resolved sampler built by hand for that point on stream g, and --no-stack writes the same files."""
    import json
    argv = ["--config", "C5", "--points", "4", "--nwalkers", "32", "--burnin", "8", "--nsteps", "16", "--energy-resolved", "--marginals",
            "--diagnostics"]
    d1, d2 = str(tmp_path / "stacked"), str(tmp_path / "nostack")
    scan.main(argv + ["--datadir", d1])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["likelihood"] == "energy-resolved" and line["stacked"] and line["nonunitary"]["launch_shape"]["shape"] == "grid"
    pts = scan.sens_grid()[:4]
    names = [scan.point_filename("C5", p, argparse.Namespace(energy_resolved=True)) for p in pts]
    want_files = sorted([n + ".npy" for n in names] + ["marginals_%s.npz" % n for n in names] + ["diagnostics_%s.npz" % n for n in names])
    assert all("_ebins" in f for f in want_files) and sorted(os.listdir(d1)) == want_files
    meas = scan.binned_measurements(argparse.Namespace(binned_smearing=None, binned_measurement=None), sorted({p[0] for p in pts}))
    for g, p in enumerate(pts):
        j = scan._SensPoint(p, g, nwalkers=32, device=0, binned=meas[p[0]])
        s = mcmc_utils.DeviceEnsembleSampler(32, 12, j.f, seed=25, stream_ids=[g], energy_resolved=True)
        try:
            s.run_mcmc(j.p0, 8, storechain=False)
            s.reset()
            s.run_mcmc(None, 16)
            saved = np.load(os.path.join(d1, names[g] + ".npy"))
            assert saved.shape == (16 * 32, 12) and same_bits(saved, s.flat_steps())
            lp, st = j.f.model.lnprob(saved, want_status=True)
            ok = st == _lib.GF_ST_OK
            assert ok.sum() > 0.9 * len(ok) and same_bits(s._fetch(lnprob=True)[1].reshape(-1)[ok], lp[ok])
        finally:
            s.close()
            j.close()
    scan.main(argv + ["--datadir", d2, "--no-stack"])
    assert not json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stacked"]
    assert sorted(os.listdir(d2)) == want_files
    for f in want_files:
        if f.endswith(".npy"):
            assert same_bits(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))), f
        else:
            with np.load(os.path.join(d1, f)) as a, np.load(os.path.join(d2, f)) as b:
                assert sorted(a.files) == sorted(b.files)
                for k in a.files:
                    assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (f, k)
