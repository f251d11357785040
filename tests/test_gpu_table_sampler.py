"""GPU: the ensemble sampler under the tabulated flavour-plane likelihood (gf_sampler_create_table, the MODE_BSM_TABLE instances of
k_stretch / k_stretch_multi in csrc/gf_sampler.hip at 1, 2, 4 and 16 lanes per walker).  Every comparison is bit for
bit: the yardstick is the bulk kernel -- `Model.lnprob` of the same table model, held to the host build of csrc/gf_table.hpp by
tests/test_gpu_table.py -- driven through the numpy stretch move of tests/stretch_ref.py on the sampler's Philox stream.  A reference
run is computed once per shape and shared by the lane counts that are held to it."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

from common import BIN_EDGES, bsm_args
from golemflavor_amd import _lib, contour, llh, scan
from golemflavor_amd import configs as Cf
from golemflavor_amd import diagnostics as dg
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.enums import Texture
from golemflavor_amd.reweight import Measurement, lnw_host
from stretch_ref import accept_lhs, propose, reference_stretch
from test_gpu_binned_sampler import a_measurement, assert_same_run, bsm_model, bulk, device_run, same_bits, scale_rows

pytestmark = pytest.mark.gpu

LPWS = (1, 2, 4, 16)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def surface(N, seed, hole=None):
    """A surface that is no Gaussian: two bumps of different width, a slope and node-by-node noise of +-0.5; `hole(fr)` -> the nodes
    at -inf"""
    rng = np.random.default_rng(seed)

    def f(fr):
        d1 = np.sum((fr - np.array([0.30, 0.36, 0.34])) ** 2, axis=1)
        d2 = np.sum((fr - np.array([0.55, 0.20, 0.25])) ** 2, axis=1)
        v = np.logaddexp(-d1 / (2 * 0.15 ** 2), -1.0 - d2 / (2 * 0.3 ** 2)) + 2.0 * fr[:, 1] + rng.uniform(-0.5, 0.5, len(fr))
        return v if hole is None else np.where(hole(fr), -np.inf, v)
    return llh.TabulatedLikelihood.from_function(f, N)


def stripes(fr):
    """a quarter of the triangle, in three stripes across fr_e"""
    return np.floor(fr[:, 0] * 12.0 + 1e-9).astype(int) % 4 == 0


def striped_table(N):
    """one broad bump (the width of the failing-region chain's Gaussian, 0.3) with the stripes at -inf"""
    def f(fr):
        return np.where(stripes(fr), -np.inf, -np.sum((fr - np.array([1 / 3, 1 / 3, 1 / 3])) ** 2, axis=1) / (2 * 0.3 ** 2))
    return llh.TabulatedLikelihood.from_function(f, N)


def table_model(width, dim, tex, N, seed, binning=BIN_EDGES, hole=None):
    m, ps = bsm_model(width, dim, tex, binning=binning)
    m.set_table_likelihood(surface(N, seed, hole))
    assert m.table_nside == N
    return m, ps


class forced_lpw:
    """GF_SAMPLER_LPW for the runs inside (None: unset), read by gf_sampler_run at every run"""

    def __init__(self, lpw):
        self.lpw = lpw

    def __enter__(self):
        self.old = os.environ.pop("GF_SAMPLER_LPW", None)
        if self.lpw is not None:
            os.environ["GF_SAMPLER_LPW"] = str(self.lpw)

    def __exit__(self, *exc):
        os.environ.pop("GF_SAMPLER_LPW", None)
        if self.old is not None:
            os.environ["GF_SAMPLER_LPW"] = self.old


def table_sampler(models, multi, nch, nw, nd, seed, stream_ids=None):
    smp = mcmc_utils.DeviceEnsembleSampler(nw, nd, list(models) if multi else models[0], nchains=nch, seed=seed, stream_ids=stream_ids,
                                           tabulated=True)
    smp.on_nonunitary = "-inf"
    return smp


def check_shape(smp, lpw):
    shape = smp.launch_shape()
    assert shape["shape"] == "grid", shape
    assert shape["lanes_per_walker"] == lpw if lpw is not None else shape["lanes_per_walker"] in LPWS, (shape, lpw)


_REFS = {}


def shared_reference(key, make):
    """the numpy run of a shape, computed by the first lane count that asks for it and read-only from then on"""
    if key not in _REFS:
        ref = make()
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def run_against_reference(oracle, key, models, multi, p0, nsteps, seed, lpw, stream_ids=None):
    nch, nw, nd = p0.shape
    with forced_lpw(lpw):
        smp = table_sampler(models, multi, nch, nw, nd, seed, stream_ids)
        try:
            assert smp.launch_shape()["shape"] == "grid"
            smp.run_mcmc(p0 if nch > 1 else p0[0], nsteps)
            check_shape(smp, lpw)
            ref = shared_reference(key, lambda: reference_stretch(oracle, list(models) if multi else models[0], p0, nsteps, seed, lnprob=bulk,
                                                                  full=True, stream_ids=stream_ids))
            assert_same_run(device_run(smp), ref, "%s, %s lanes per walker" % (key, lpw))
            return smp, ref
        except BaseException:
            smp.close()
            raise


# ---- 1. one posterior, k_stretch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw", LPWS + (None,))
def test_one_posterior_graph_replays_eager_steps_and_thinning(oracle, lpw):
    """7 columns, 32 walkers, side 64, 40 steps -- two graph replays of 16 steps and eight eager ones; then reset() and 8 more at
    thin = 3: the iteration counter goes on, the store index starts again.  Forced to 1, 2, 4 and 16 lanes per walker and left to the
    rule: the same bits, and launch_shape() names the grid shape and the lane count."""
    m, ps = table_model(7, 6, Texture.OET, 64, seed=41)
    with m:
        p0 = scale_rows(ps, 32, np.random.default_rng(21), 6)[None]
        smp, ref = run_against_reference(oracle, "7 columns, 40 steps", [m], False, p0, 40, 9, lpw)
        try:
            assert smp.nonunitary_proposals == 0 and smp.iterations == 40
            with forced_lpw(lpw):
                smp.reset()
                smp.run_mcmc(None, 8, thin=3)
            check_shape(smp, lpw)
            again = shared_reference("7 columns, 8 steps at thin 3",
                                     lambda: reference_stretch(oracle, m, ref["pos"], 8, 9, lnprob=bulk, full=True, iteration0=40, thin=3, lnp0=ref["lnp"]))
            assert again["chain"].shape[1] == 3
            assert_same_run(device_run(smp), again, "after reset(), 8 steps at thin 3, %s lanes" % lpw)
        finally:
            smp.close()


# ---- 2. one posterior per chain, k_stretch_multi -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw", (1, 4))
def test_one_posterior_per_chain_with_different_sides(oracle, lpw):
    """Three stacked 12-column posteriors on streams (5, 0, 9): tables of side 1, 3 and 64 and 20, 7 and 1 energy bins, so that the
    side, the table's address and the bins a lane takes differ from chain to chain.  64 walkers, 34 steps."""
    rng = np.random.default_rng(22)
    lo, hi = Cf.DEFAULT_BINNING[0], Cf.DEFAULT_BINNING[1]
    spec = [(6, Texture.OET, 20, 1, 4), (3, Texture.OUT, 7, 3, 5), (6, Texture.OEU, 1, 64, 6)]
    made = [table_model(12, dim, tex, N, seed=sd, binning=Cf.default_bin_edges((lo, hi, K))) for dim, tex, K, N, sd in spec]
    models = [m for m, _ in made]
    try:
        assert [m.nbins for m in models] == [20, 7, 1] and [m.table_nside for m in models] == [1, 3, 64]
        p0 = np.stack([scale_rows(ps, 64, rng, dim) for (_, ps), (dim, _, _, _, _) in zip(made, spec)])
        smp, _ = run_against_reference(oracle, "three posteriors, 34 steps", models, True, p0, 34, 13, lpw, stream_ids=(5, 0, 9))
        smp.close()
    finally:
        for m in models:
            m.close()


# ---- 3. generic row width ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw", (1, 16))
def test_generic_row_width_one_partial_block(oracle, lpw):
    """The 11-column Texture.NONE paramset (the NDIM = 0 instance), 300 walkers: nhalf = 150 is one partial block at one lane per
    walker and nine blocks and a partial one at 16; 20 steps are eager."""
    m, ps = table_model(11, 6, Texture.NONE, 24, seed=43)
    with m:
        p0 = scale_rows(ps, 300, np.random.default_rng(23), 6)[None]
        smp, _ = run_against_reference(oracle, "11 columns, 300 walkers", [m], False, p0, 20, 17, lpw)
        smp.close()


# ---- 4. ragged launches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw", (1, 2))
def test_two_chains_of_600_walkers_on_one_posterior(oracle, lpw):
    """12 columns, two chains of 600 walkers on one posterior (k_stretch): 600 proposals per half-step.  One lane per walker: three
    blocks, the middle one shared by the two chains, the last partial.  Two lanes: five blocks, the middle one shared, the last
    partial.  18 steps."""
    m, ps = table_model(12, 6, Texture.OET, 33, seed=44)
    with m:
        p0 = scale_rows(ps, 1200, np.random.default_rng(24), 6).reshape(2, 600, 12)
        smp, _ = run_against_reference(oracle, "12 columns, 2 x 600 walkers", [m], False, p0, 18, 19, lpw)
        smp.close()


@pytest.mark.parametrize("lpw", (1, 2))
def test_two_chains_of_600_walkers_one_posterior_per_chain(oracle, lpw):
    """The same shape through k_stretch_multi: two posteriors of 600 walkers with tables of side 33 and 20, two (three) blocks per
    chain, the last one partial."""
    made = [table_model(12, 6, tex, N, seed=sd) for tex, N, sd in ((Texture.OET, 33, 45), (Texture.OUT, 20, 46))]
    models = [m for m, _ in made]
    try:
        rng = np.random.default_rng(25)
        p0 = np.stack([scale_rows(ps, 600, rng, 6) for _, ps in made])
        smp, _ = run_against_reference(oracle, "12 columns, 2 posteriors x 600 walkers", models, True, p0, 18, 19, lpw)
        smp.close()
    finally:
        for m in models:
            m.close()


# ---- 5. through the failing region ---------------------------------------------------------------------------------------------------------
FAILING_SEED = 11


def failing_region_setup(on_nonunitary):
    """tests/test_gpu_binned_sampler.py's failing_region_setup with a table in place of the binned measurement: the 12-column OEU chain,
    64 walkers, scale seeded over [-40, -30]; the table has -inf stripes over a quarter of the triangle"""
    inj = fr_utils.fr_to_angles((1, 1, 1))
    asimov, ps = Cf.fr_paramsets(6, inj)
    args = bsm_args(6, Texture.OEU, (1 / 3, 2 / 3, 0.))
    rng = np.random.default_rng(4)
    box = np.array(ps.seeds, dtype=float)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(64, 12))
    p0[:, 11] = rng.uniform(-40.0, -30.0, 64)
    f = llh.bsm_ln_prob(args, asimov, ps, smearing=0.3, on_nonunitary=on_nonunitary, table=striped_table(48))
    return f, p0


def test_through_the_failing_region_decision_by_decision(oracle):
    """40 steps through the region where the reference raises, on_nonunitary="-inf", walked proposal by proposal on the device's own
    positions: every accept decision and every stored lnprob is the one taken from the bulk kernel's value and exact status of the same
    proposal, and `nonunitary_proposals` is the number of proposals (and start positions) the bulk status calls non-unitary.
    Conditions on the inputs, asserted on the reference walk: at least one move, one non-unitary proposal, one proposal whose table
    value is -inf, and one proposal completed by k_stretch_settle (the sampler's census, gf_internal_sampler_parked)."""
    nw, nsteps, seed, ndim = 64, 40, FAILING_SEED, 12
    nhalf = nw // 2
    f, p0 = failing_region_setup("-inf")
    smp = mcmc_utils.DeviceEnsembleSampler(nw, ndim, f, seed=seed, tabulated=True)
    try:
        assert smp.on_nonunitary == "-inf"
        smp.run_mcmc(p0, nsteps)
        run = device_run(smp)
        got, got_lnp = run["chain"][0], run["lnp_chain"][0]
        nbad_dev, parked = smp.nonunitary_proposals, smp.parked_proposals
        pos = p0.copy()
        lp, st = f.model.lnprob(pos, want_status=True)
        lnp = np.where(st == _lib.GF_ST_NON_UNITARY, -np.inf, lp)
        nbad, naccept, nhole = int(np.sum(st == _lib.GF_ST_NON_UNITARY)), 0, 0
        key = (seed & 0xffffffff, seed >> 32)
        for it in range(nsteps):
            for half in (0, 1):
                q, zz, u3 = propose(oracle, key, pos, half, 2 * it + half)
                lq, sq = f.model.lnprob(q, want_status=True)
                bad = sq == _lib.GF_ST_NON_UNITARY
                nhole += int(np.sum((sq == _lib.GF_ST_OK) & (lq == -np.inf)))       # inside the box and unitary: the -inf is the table's
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
            assert same_bits(got_lnp[it], lnp), "step %d: stored lnprob" % it
        print("moves %d, non-unitary proposals %d (device %d), table at -inf %d, completed by k_stretch_settle %s" % (naccept, nbad, nbad_dev, nhole, parked))
        assert naccept >= 1 and nbad >= 1 and nhole >= 1 and parked is not None and parked >= 1, (naccept, nbad, nhole, parked)
        assert nbad_dev == nbad
        assert same_bits(run["lnp"][0], lnp) and same_bits(run["pos"][0], pos)
        assert int(run["nacc"].sum()) == naccept
    finally:
        smp.close()
        f.close()


# ---- 6. / 7. stored lnprob and holes --------------------------------------------------------------------------------------------------------
def holed_run(oracle):
    """7 columns, 32 walkers, 36 steps under a table whose hole is drawn through the start positions' own compositions: the walkers
    with fr_e above the median start inside it.  Returns what the tests below read."""
    m, ps = bsm_model(7, 6, Texture.OET)
    p0 = scale_rows(ps, 32, np.random.default_rng(27), 6)
    _, fr0, st0 = m.lnprob(p0, want_fr=True, want_status=True)
    assert np.all(st0 == _lib.GF_ST_OK)
    cut = float(np.median(fr0[:, 0]))
    m.set_table_likelihood(surface(64, 48, hole=lambda fr: fr[:, 0] > cut))
    smp = table_sampler([m], False, 1, 32, 7, 23)
    smp.run_mcmc(p0, 36)
    return m, smp, p0, cut


def test_stored_lnprob_is_the_bulk_lnprob_of_the_stored_theta(oracle):
    """Every stored (row, lnprob) pair is Model.lnprob(row) bit for bit, the rows held at -inf inside the table's hole included."""
    m, smp, p0, cut = holed_run(oracle)
    try:
        run = device_run(smp)
        rows, stored = run["chain"][0].reshape(-1, 7), run["lnp_chain"][0].reshape(-1)
        lp, st = m.lnprob(rows, want_status=True)
        print("%d rows, %d at -inf, %d distinct values" % (len(rows), int(np.sum(stored == -np.inf)), len(np.unique(stored))))
        assert np.all(st == _lib.GF_ST_OK) and np.sum(stored == -np.inf) >= 1 and len(np.unique(stored)) > 32
        assert same_bits(stored, lp), int(np.sum(stored != lp))
    finally:
        smp.close()
        m.close()


def test_walkers_started_in_a_hole_leave_it_and_stay_out(oracle):
    """The walkers started inside the hole hold -inf, leave it (a finite proposal always replaces -inf) and never return: no stored
    sample of a walker after its first finite one lies in the hole.  Acceptance counts, chain and lnprob equal the numpy move's."""
    m, smp, p0, cut = holed_run(oracle)
    try:
        run = device_run(smp)
        ref = reference_stretch(oracle, m, p0[None], 36, 23, lnprob=bulk, full=True)
        assert_same_run(run, ref, "holed table")
        started_in = m.lnprob(p0)[0] == -np.inf
        finite = np.isfinite(run["lnp_chain"][0])                                  # (step, walker)
        left = finite[-1] & started_in
        print("%d of 32 walkers started in the hole, %d left it" % (started_in.sum(), left.sum()))
        assert started_in.sum() >= 8 and left.sum() > started_in.sum() // 2
        assert np.all(finite[1:] >= finite[:-1]), "a walker returned to -inf"
        _, fr, _ = m.lnprob(run["chain"][0].reshape(-1, 7), want_fr=True, want_status=True)
        inside = (fr[:, 0] > cut).reshape(finite.shape)
        # (the converse does not hold: a composition just below the edge has a node of its cell inside the hole and is at -inf too)
        assert inside.any() and not np.any(inside & finite)
    finally:
        smp.close()
        m.close()


# ---- 8. a table replaced between two runs ----------------------------------------------------------------------------------------------------
def test_a_table_replaced_between_two_runs_is_the_one_the_next_run_samples(oracle):
    """A run of 36 steps (two graph replays) under a table of side 16; the model's table is replaced by another of side 16 (written in
    place) and 34 more steps run, then by one of side 40 (the table moves) and 34 more, then by one of side 5 (smaller, written in place
    into the buffer of the side-40 table) and 34 more.  Each later run equals the numpy move on the new table from the run before's final
    state, the walkers holding the lnprob the device holds -- the old table's, not recomputed."""
    m, ps = table_model(7, 6, Texture.OET, 16, seed=50)
    with m:
        p0 = scale_rows(ps, 32, np.random.default_rng(28), 6)[None]
        smp, ref = run_against_reference(oracle, "before the replacement", [m], False, p0, 36, 29, None)
        try:
            done = 36
            for N, sd in ((16, 51), (40, 52), (5, 53)):
                m.set_table_likelihood(surface(N, sd))
                assert m.table_nside == N
                smp.reset()
                smp.run_mcmc(None, 34)
                new = reference_stretch(oracle, m, ref["pos"], 34, 29, lnprob=bulk, full=True, iteration0=done, lnp0=ref["lnp"])
                stale = bulk(m, ref["pos"][0]) != ref["lnp"][0]
                assert stale.sum() > 16, "the replacement changes nothing: nothing was compared"
                assert_same_run(device_run(smp), new, "after a replacement by side %d" % N)
                ref, done = new, done + 34
        finally:
            smp.close()


# ---- 9. refusals and neighbours ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_neighbours(oracle):
    rng = np.random.default_rng(26)
    L = _lib.lib()
    m, ps = table_model(7, 6, Texture.OET, 32, seed=53)
    flux, _ = bsm_model(7, 6, Texture.OET)
    binned, _ = bsm_model(7, 6, Texture.OET)
    with m, flux, binned:
        binned.set_binned_measurement(a_measurement(20, BIN_EDGES))
        p0 = scale_rows(ps, 32, rng, 6)
        # the keyword without a table; a mixture and a binned model through the C entry point; the other entry points on the table model
        with pytest.raises(ValueError, match="carries no tabulated likelihood"):
            mcmc_utils.DeviceEnsembleSampler(32, 7, flux, seed=1, tabulated=True)
        h = C.c_void_p()
        rc = L.gf_sampler_create_table((C.c_void_p * 2)(m._h, flux._h), 2, 2, 32, 5, 2.0, C.byref(h))
        assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
        assert b"model 1 carries no tabulated likelihood" in L.gf_last_hip_error()
        rc = L.gf_sampler_create_table((C.c_void_p * 1)(binned._h), 1, 1, 32, 5, 2.0, C.byref(h))
        assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
        assert b"model 0 carries no tabulated likelihood" in L.gf_last_hip_error()
        rc = L.gf_sampler_create_table((C.c_void_p * 2)(m._h, m._h), 2, 3, 32, 5, 2.0, C.byref(h))      # nmodels is 1 or nchains
        assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
        with pytest.raises(_lib.GolemHipError) as e:
            mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=1)
        assert e.value.code == _lib.GF_ERR_UNSUPPORTED

        s = table_sampler([m], False, 1, 32, 7, 5)
        try:
            s.run_mcmc(p0, 40)
            c, lp0, _ = s._fetch(chain=True, lnprob=True)
            # measurement targets: refused by the library, and the sampler goes on; model targets: as for any chain
            with pytest.raises(_lib.GolemHipError) as e:
                s.reweight([Measurement(bestfit_fr=(0.3, 0.3, 0.4))], on_nonunitary="-inf")
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED and "tabulated" in str(e.value)
            r = s.reweight([flux], on_nonunitary="-inf")
            rows, base = c.reshape(-1, 7), lp0.reshape(-1)
            lt, st = flux.lnprob(rows, want_status=True)
            want, kind = lnw_host(lt, base, st)
            assert np.sum(kind == 0) >= 1000 and same_bits(r.lnw(0)[0], want)
            # the reducers read the chain as any sampler's: equal to the stand-alone reducers on the same rows, uploaded from the host
            frows = s.postprocess_rows()[0]
            assert frows.shape == (40 * 32, 10) and np.array_equal(frows[:, 3:], rows)
            got = s.marginals(with_fr=True)
            want = mg.chain_marginals(frows, [tuple(x) for x in got.ranges], model=m, names=got.names)
            a, b = got.as_arrays(), want.as_arrays()
            assert sorted(a) == sorted(b)
            for k in a:
                assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), ("marginals", k)
            rg, rw = s.regions(30, (68., 90.)), contour.flavor_region(frows[:, :3], 30, (68., 90.), model=m)
            assert len(rg) == len(rw) == 2
            for g, w in zip(rg, rw):
                for k in ("thres", "saturated", "level_in", "level_out", "mass", "flat_cells", "density"):
                    x, y = np.asarray(getattr(g, k)), np.asarray(getattr(w, k))
                    assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), ("regions", k)
            dgot, dwant = s.diagnostics(), dg.chain_diagnostics(c[0], model=m)
            b = dwant.as_arrays()
            a = dgot.as_arrays()
            for k in b:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(b[k]).dtype.kind == "f"), ("diagnostics", k)
            # still usable after all of it: eight more steps equal the numpy move's
            before = device_run(s)
            s.reset()
            s.run_mcmc(None, 8)
            more = reference_stretch(oracle, m, before["pos"], 8, 5, lnprob=bulk, full=True, iteration0=40, lnp0=before["lnp"])
            got8 = device_run(s)
            assert same_bits(got8["chain"], more["chain"]) and same_bits(got8["lnp_chain"], more["lnp_chain"])
        finally:
            s.close()


# ---- 10. the scan, end to end ------------------------------------------------------------------------------------------------------------------
def test_scan_likelihood_table_end_to_end(tmp_path, capsys):
    """scan.main --config C5 --likelihood-table F: the files carry `_ltab`, every chain file is the chain of a tabulated sampler built by
    hand for that point on stream g, and --no-stack writes the same bytes."""
    table = surface(40, 54, hole=lambda fr: fr[:, 0] > 0.9)
    path = str(tmp_path / "surface.npy")
    table.save(path)
    argv = ["--config", "C5", "--likelihood-table", path, "--points", "3", "--nwalkers", "64", "--burnin", "4", "--nsteps", "6"]
    d1, d2 = str(tmp_path / "stacked"), str(tmp_path / "nostack")
    scan.main(argv + ["--datadir", d1])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["likelihood"] == "tabulated" and line["stacked"] and line["nonunitary"]["launch_shape"]["shape"] == "grid"
    pts = scan.sens_grid()[:3]
    names = [scan.point_filename("C5", p, argparse.Namespace(likelihood_table=path)) for p in pts]
    want_files = sorted(n + ".npy" for n in names)
    assert all(f.endswith("_ltab.npy") for f in want_files) and sorted(os.listdir(d1)) == want_files
    for g, p in enumerate(pts):
        j = scan._SensPoint(p, g, nwalkers=64, device=0, table=table)
        s = mcmc_utils.DeviceEnsembleSampler(64, 12, j.f, seed=25, stream_ids=[g], tabulated=True)
        try:
            s.run_mcmc(j.p0, 4, storechain=False)
            s.reset()
            s.run_mcmc(None, 6)
            saved = np.load(os.path.join(d1, names[g] + ".npy"))
            assert saved.shape == (6 * 64, 12) and same_bits(saved, s.flat_steps())
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
        with open(os.path.join(d1, f), "rb") as x, open(os.path.join(d2, f), "rb") as y:
            assert x.read() == y.read(), f
