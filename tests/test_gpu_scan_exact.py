"""GPU: the C4 / C5 grid scans (golemflavor_amd/scan.py), grid point by grid point, against references that share nothing
with scan.py.

For every grid point g the reference is restated from the rules of the reference's jobs: the posterior is compiled by the ORACLE
from that point's (dimension, texture, source, scale); p0 is drawn from default_rng(25 + g) over the paramset's seed box (C5: the
logLam column clip(normal(scale, 0.5), lo, hi)); the chain is the numpy stretch move of tests/stretch_ref.py on the sampler's
Philox stream -- stacked scans: seed 25, stream g; --no-stack: seed 25 + g, stream 0 --, a burn-in, reset(), then the stored run.
The proposals the reference would have died on score -inf (C5) and the rows it would have died on are NaN (C4), with the band
around the threshold decided by the host build of the device's x87 chain (stretch_ref.Arbiter).

Row order (scan.py's docstring): row = step * nwalkers + walker on every delivery path."""
import argparse
import os

import numpy as np
import pytest

from common import BIN_EDGES
from golemflavor_amd import configs as Cf
from golemflavor_amd import dist as gdist
from golemflavor_amd import fr as fr_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import ParamSet
from stretch_ref import Arbiter, reference_stretch

pytestmark = pytest.mark.gpu

SEED = 25                      # scan.py's default seed: the stacked sampler's key; seed + g per point otherwise
NW = 32
ABS_FR = 1e-10


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------
def _c4_paramset(dim):
    """scripts/mc_texture.py:28-76 without logLam (fixed per grid point): 4 mixing angles, 2 mass splittings."""
    return ParamSet(list(Cf.texture_paramset(dim))[:6])


def _c4_p0(dim, g, nw=NW):
    box = np.array(_c4_paramset(dim).seeds, dtype=float)
    return np.random.default_rng(SEED + g).uniform(box[:, 0], box[:, 1], size=(nw, 6))


def _replay(oracle, oms, p0, gs, burnin, nsteps, stacked, lnprob=None):
    """Stored chains (npoints, nsteps, nwalkers, ndim) of the points gs: one stacked sampler (seed 25, stream g) or one sampler
    per point (seed 25 + g, stream 0); burn-in, reset(), stored run -- the step counter runs on across the reset."""
    def run(om, p, seed, sids):
        burn = reference_stretch(oracle, om, p, burnin, seed, lnprob=lnprob, stream_ids=sids, full=True)
        return reference_stretch(oracle, om, burn["pos"], nsteps, seed, lnprob=lnprob, stream_ids=sids, iteration0=burnin,
                                 lnp0=burn["lnp"], full=True)["chain"]
    if stacked:
        return run(oms, p0, SEED, list(gs))
    return np.concatenate([run([oms[i]], p0[i:i + 1], SEED + g, [0]) for i, g in enumerate(gs)])


class C4Point:
    """The oracle's post-processing of one C4 point's samples: flux_averaged_BSMu at the point's scale and source
    (mc_texture.py:216-221; the model's scale from scale_fixed), NaN where the reference raises."""

    def __init__(self, oracle, hx, point, samples, dim, tex):
        self.scale, self.source = point
        self.samples, self.dim, self.tex = samples, dim, tex
        ps6 = _c4_paramset(dim)
        kw = dict(dimension=dim, binning=BIN_EDGES, source_ratio=self.source, scale_fixed=self.scale, bestfit_fr=(1 / 3,) * 3,
                  smearing=0.02)
        om = oracle.make_model(ps6, "BSM_GAUSS", texture=tex, **kw)
        with Model(compile_model(ps6, "BSM_GAUSS", texture=Texture[tex], **kw)) as m:
            arb = Arbiter(oracle, om, m, harness=hx)
            self.fr, st = oracle.propagate_batch(om, samples)
            self.bad, self.band, self.acquit = arb.verdict(samples, st)
            self.r80 = arb.residual
        self._exact = {}

    def exact(self, rows):
        from exact_mp import exact_flux_avg
        todo = [i for i in rows if i not in self._exact]
        if todo:
            th = np.column_stack([self.samples[todo], np.full(len(todo), self.scale)])
            for i, v in zip(todo, exact_flux_avg(th, self.tex, self.dim, self.source, BIN_EDGES)):
                self._exact[i] = v
        return np.array([self._exact[i] for i in rows]).reshape(-1, 3)

    def check(self, rows, label):
        """rows: the scan's rows of this point, one per sample of `samples`."""
        samples, fr_ref, bad, r80 = self.samples, self.fr, self.bad, self.r80
        assert rows.shape == (len(samples), 9), (label, rows.shape)
        _check_samples(rows[:, 3:], samples, label)
        nan = np.isnan(rows[:, :3])
        assert np.array_equal(nan.any(axis=1), nan.all(axis=1)), label
        wrong = np.flatnonzero(nan[:, 0] != bad)
        assert wrong.size == 0, "%s: %d rows with the wrong NaN verdict, e.g. row %d (scan NaN %s, reference non-unitary %s, " \
            "residual %.3e)" % (label, wrong.size, wrong[0], nan[wrong[0], 0], bad[wrong[0]], r80[wrong[0]])
        good = ~bad
        with np.errstate(invalid="ignore"):
            err = np.where(good, np.abs(rows[:, :3] - fr_ref).max(axis=1), 0.0)
        over = np.flatnonzero(good & ~(err <= ABS_FR + 10.0 * r80))        # NaN err: the oracle raised where the harness acquits
        if not over.size:
            return
        # over the bar: arbitrate with 60-digit arithmetic, as test_gpu_fuzz.test_random_bsm_configurations does -- the kernel
        # must be the accurate one; rows the harness acquits (the oracle has no value there) are held to the exact value too
        acq = np.isnan(fr_ref[over]).any(axis=1)
        plain = over[~acq]
        assert plain.size <= max(2, 0.02 * good.sum()), (label, plain.size, int(good.sum()))
        worst = plain[np.argsort(err[plain])[::-1][:6]]
        for pick, bar in ((worst, None), (over[acq][:6], ABS_FR + 10.0 * r80)):
            if not pick.size:
                continue
            exact = self.exact(list(pick))
            dev_err = np.abs(rows[pick, :3] - exact).max(axis=1)
            if bar is None:
                assert dev_err.max() <= 1e-11, (label, pick, dev_err)
                assert np.abs(fr_ref[pick] - exact).max() > dev_err.max(), (label, pick)
            else:
                assert np.all(dev_err <= bar[pick]), (label, pick, dev_err)


def _check_samples(got, want, label):
    """The scan's samples are the reference chain's, row = step * nwalkers + walker: same accept decisions, positions within
    1e-12 of each column's magnitude (the mass splittings are ~1e-21)."""
    scale = np.maximum(np.abs(want).max(axis=0), 1e-300)
    ok = np.abs(got - want) <= 1e-12 * scale
    if not ok.all():
        bad = np.flatnonzero(~ok.all(axis=1))
        msg = "%s: %d of %d sample rows differ from the replay, first row %d" % (label, bad.size, len(want), bad[0])
        n = len(want)
        for nw in (NW, 2048):
            if n % nw == 0:
                ns = n // nw
                wm = want.reshape(ns, nw, -1).transpose(1, 0, 2).reshape(n, -1)   # emcee's walker-major flatchain order
                if np.all(np.abs(got - wm) <= 1e-12 * scale):
                    msg += " -- they are the replay's samples in walker-major order (row = walker * nsteps + step)"
        raise AssertionError(msg)


def _c5_model(oracle, point):
    """(oracle model, golemflavor_amd model, seed box, scale range) of a C5 point: scripts/fr.py:62-104's 12-dim paramset and
    llh.bsm_ln_prob's posterior with the Gaussian substitute, best fit angles_to_fr(fr_to_angles(1, 1, 1))."""
    dim, tex, src, scale = point
    asimov, ps = Cf.fr_paramsets(dim, fr_utils.fr_to_angles((1, 1, 1)))
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    kw = dict(bestfit_fr=bf, smearing=0.02, source_ratio=src, dimension=dim, binning=BIN_EDGES)
    om = oracle.make_model(ps, "BSM_GAUSS", texture=tex.name, **kw)
    return om, Model(compile_model(ps, "BSM_GAUSS", texture=tex, **kw)), np.array(ps.seeds, dtype=float), Cf.SCALE_BOUNDARIES[dim]


def _c5_p0(box, lohi, scale, g, nw=NW):
    rng = np.random.default_rng(SEED + g)
    p0 = rng.uniform(box[:, 0], box[:, 1], size=(nw, 12))
    p0[:, 11] = np.clip(rng.normal(scale, 0.5, nw), *lohi)
    return p0


# ----------------------------------------------------------------------------------------------------------------------
# scans
# ----------------------------------------------------------------------------------------------------------------------
def _main_line(capsys):
    import json
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _device_gather():
    from golemflavor_amd import scan
    stage = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=(1, 2, 0)), device=0)
    return stage, scan.DeviceGather(None, 0, 1, stage)


def _as_list(out, n):
    return [out[g] for g in range(n)] if isinstance(out, dict) else list(out)


@pytest.fixture(scope="module")
def harness():
    import x87_harness as H
    return H.build()


C4_POINTS, C4_BURN, C4_STEPS = 61, 5, 10


@pytest.fixture(scope="module")
def c4_reference(oracle, harness):
    """The default C4 grid's first 61 points (texture OEU: the top scales are the failing region), 32 walkers, 5 + 10 steps:
    the stacked scan's chains replayed, and their oracle post-processing."""
    from golemflavor_amd import scan
    pts = scan.texture_grid(6)[:C4_POINTS]
    assert [round(s, 6) for s, _ in pts[::8]] == [round(s, 6) for s in np.linspace(-56, -30, 8)]
    om_prior = oracle.make_model(_c4_paramset(6), "PRIOR_ONLY", flat_llh=1.0)
    gs = list(range(C4_POINTS))
    p0 = np.stack([_c4_p0(6, g) for g in gs])
    chains = _replay(oracle, [om_prior] * len(gs), p0, gs, C4_BURN, C4_STEPS, stacked=True)
    refs = [C4Point(oracle, harness, pts[g], chains[g].reshape(-1, 6), 6, "OEU") for g in gs]
    nan_pts = sum(r.bad.all() for r in refs)
    assert 0 < nan_pts < C4_POINTS and sum((~r.bad).all() for r in refs) > 0
    return pts, refs, om_prior


def test_c4_scan_every_delivery_path_equals_the_replay(c4_reference, oracle, tmp_path, capsys, monkeypatch):
    """C4 (scripts/mc_texture.py) rows of every grid point: columns 3: the flat-likelihood prior chain of stream g, in the
    documented row order; columns :3 the oracle's flux average at the point's scale and source, NaN exactly where the reference
    raises.  61 chains: gf_sampler_postprocess_rows makes 16 groups of 4 with a ragged last one."""
    from golemflavor_amd import scan
    pts, refs, om_prior = c4_reference
    args = ["--config", "C4", "--texture", "OEU", "--points", str(C4_POINTS), "--nwalkers", str(NW), "--burnin", str(C4_BURN),
            "--nsteps", str(C4_STEPS)]
    per = NW * C4_STEPS
    # one-rank DeviceGather: gf_sampler_postprocess_rows
    scan.main(args + ["--outfile", str(tmp_path / "dg")])
    line = _main_line(capsys)
    assert line["gather"] == "device -> host" and line["chains_shape"] == [C4_POINTS, per, 9]
    rows = np.load(str(tmp_path / "dg.npy"))
    for g, ref in enumerate(refs):
        ref.check(rows[g], "postprocess_rows, point %d" % g)
    # --datadir, no --outfile: gather=None, the host's _TexturePoint.assemble; every file read back
    scan.main(args + ["--datadir", str(tmp_path / "files")])
    assert _main_line(capsys)["gather"].startswith("none")
    ns = argparse.Namespace(dimension=6, texture="OEU")
    files = sorted(os.listdir(str(tmp_path / "files")))
    assert len(files) == C4_POINTS
    for g, ref in enumerate(refs):
        arr = np.load(os.path.join(str(tmp_path / "files"), scan.point_filename("C4", pts[g], ns) + ".npy"))
        ref.check(arr, "--datadir file, point %d" % g)
        assert np.array_equal(arr, rows[g], equal_nan=True)
    # GF_SCAN_RCCL=1: gf_sampler_postprocess_rows_device, then DeviceGather._exchange
    monkeypatch.setenv("GF_SCAN_RCCL", "1")
    scan.main(args + ["--outfile", str(tmp_path / "rccl")])
    line = _main_line(capsys)
    monkeypatch.delenv("GF_SCAN_RCCL")
    assert line["gather"] == "rccl device gather to rank 0" and line["rccl_error"] is None
    rr = np.load(str(tmp_path / "rccl.npy"))
    for g, ref in enumerate(refs):
        ref.check(rr[g], "rows_to_device + exchange, point %d" % g)
    # rank 1's shard of a world of 2 (gather=None): `order` and the stream ids are not 0..n-1
    mine = gdist.shard(C4_POINTS, 1, 2)
    assert mine != list(range(len(mine)))
    make = lambda p, g: scan._TexturePoint(p, g, dimension=6, texture=Texture.OEU, nwalkers=NW, device=0)  # noqa: E731
    out = scan.run_points(pts, mine, make, C4_BURN, C4_STEPS, gather=None)
    assert sorted(out) == mine
    for g in mine:
        refs[g].check(out[g], "rank 1 of 2, point %d" % g)


def test_c4_scan_no_stack_equals_its_own_replay(c4_reference, oracle, harness, capsys, tmp_path):
    """--no-stack: one sampler per point, seed 25 + g on stream 0; its rows in the same (step, walker) order as the stacked
    paths'."""
    from golemflavor_amd import scan
    pts, refs, om_prior = c4_reference
    n = C4_POINTS
    gs = list(range(n))
    scan.main(["--config", "C4", "--texture", "OEU", "--points", str(n), "--nwalkers", str(NW), "--burnin", str(C4_BURN),
               "--nsteps", str(C4_STEPS), "--no-stack", "--outfile", str(tmp_path / "ns")])
    line = _main_line(capsys)
    assert line["stacked"] is False
    rows = np.load(str(tmp_path / "ns.npy"))
    p0 = np.stack([_c4_p0(6, g) for g in gs])
    chains = _replay(oracle, [om_prior] * len(gs), p0, gs, C4_BURN, C4_STEPS, stacked=False)
    for i, g in enumerate(gs):
        C4Point(oracle, harness, pts[g], chains[i].reshape(-1, 6), 6, "OEU").check(rows[g], "--no-stack, point %d" % g)


def test_c4_through_the_unitarity_transition(oracle, harness):
    """Texture OEU between logLam -36.2 and -34.1, where a point's rows are part unitary, part not, and many sit in the band
    around the threshold: the NaN pattern row by row through both post-processing paths (the per-chain model switch of
    postprocess(models=...) with the host's assemble, and gf_sampler_postprocess_rows)."""
    from golemflavor_amd import scan
    scales = (-36.17, -35.34, -34.93, -34.52, -34.11)
    sources = ((0.5, 0.5, 0.0), (1.0, 0.0, 0.0), (0.2, 0.8, 0.0))
    pts = [(s, src) for s in scales for src in sources]
    gs = list(range(len(pts)))
    om_prior = oracle.make_model(_c4_paramset(6), "PRIOR_ONLY", flat_llh=1.0)
    burnin, nsteps = 5, 10
    chains = _replay(oracle, [om_prior] * len(gs), np.stack([_c4_p0(6, g) for g in gs]), gs, burnin, nsteps, stacked=True)
    refs = [C4Point(oracle, harness, pts[g], chains[g].reshape(-1, 6), 6, "OEU") for g in gs]
    mixed = sum(0 < r.bad.sum() < len(r.bad) for r in refs)
    nband = sum(int(r.band.sum()) for r in refs)
    print("transition: %d of %d points mixed, %d band rows" % (mixed, len(refs), nband))
    assert mixed >= 5 and nband > 50
    make = lambda p, g: scan._TexturePoint(p, g, dimension=6, texture=Texture.OEU, nwalkers=NW, device=0)  # noqa: E731
    out = scan.run_points(pts, gs, make, burnin, nsteps, gather=None)
    for g in gs:
        refs[g].check(out[g], "host assemble, transition point %d" % g)
    stage, dg = _device_gather()
    rows = scan.run_points(pts, gs, make, burnin, nsteps, gather=dg)
    stage.close()
    for g in gs:
        refs[g].check(rows[g], "postprocess_rows, transition point %d" % g)


def test_c4_scan_at_size_paths_agree_and_match_the_oracle(oracle, harness, tmp_path, capsys, monkeypatch):
    """The full 64-point C4 grid (OEU) at 2048 walkers and 24 stored steps: 226 MB of rows, 16 groups of 4 chains, 14 ring
    chunks of 16 MB.  The DeviceGather, GF_SCAN_RCCL=1 and gather=None paths agree bit for bit, NaNs included, and a subsample
    -- the rows on both sides of every group boundary and every 16 MB boundary, plus random rows -- is the oracle's."""
    from golemflavor_amd import scan
    nw, burnin, nsteps = 2048, 2, 24
    args = ["--config", "C4", "--texture", "OEU", "--nwalkers", str(nw), "--burnin", str(burnin), "--nsteps", str(nsteps)]
    scan.main(args + ["--outfile", str(tmp_path / "dg")])
    assert _main_line(capsys)["chains_shape"] == [64, nw * nsteps, 9]
    a = np.load(str(tmp_path / "dg.npy"))
    monkeypatch.setenv("GF_SCAN_RCCL", "1")
    scan.main(args + ["--outfile", str(tmp_path / "rccl")])
    assert _main_line(capsys)["gather"] == "rccl device gather to rank 0"
    monkeypatch.delenv("GF_SCAN_RCCL")
    assert np.array_equal(a, np.load(str(tmp_path / "rccl.npy")), equal_nan=True)
    os.remove(str(tmp_path / "rccl.npy"))
    scan.main(args + ["--datadir", str(tmp_path / "files")])
    _main_line(capsys)
    pts = scan.texture_grid(6)
    ns = argparse.Namespace(dimension=6, texture="OEU")
    for g in range(64):
        f = os.path.join(str(tmp_path / "files"), scan.point_filename("C4", pts[g], ns) + ".npy")
        assert np.array_equal(a[g], np.load(f), equal_nan=True), g
    assert np.isnan(a[:, :, 0]).any() and np.isfinite(a[:, :, 0]).any()
    # the subsample, as flat row indices of the (64 * per, 9) block
    per = nw * nsteps
    row_bytes, total = 9 * 8, 64 * per
    edges = [c * per for c in range(4, 64, 4)]                                          # group boundaries (4 chains per group)
    edges += [(k << 24) // row_bytes for k in range(1, (total * row_bytes >> 24) + 1)]   # 16 MB chunk boundaries
    flat = set()
    for e in edges:
        flat.update(range(max(0, e - 2), min(total, e + 3)))
    rng = np.random.default_rng(64)
    flat.update(rng.choice(total, 16000, replace=False).tolist())
    flat = np.array(sorted(flat))
    print("subsample: %d rows, %d boundaries" % (flat.size, len(edges)))
    for g in range(64):
        idx = flat[(flat >= g * per) & (flat < (g + 1) * per)] - g * per
        if idx.size:
            ref = C4Point(oracle, harness, pts[g], a[g, idx, 3:], 6, "OEU")
            ref.check(a[g, idx], "at size, point %d" % g)
    # two points' chains replayed in full: each point's rows are its own chain, in the documented order
    om_prior = oracle.make_model(_c4_paramset(6), "PRIOR_ONLY", flat_llh=1.0)
    gs = [5, 58]
    chains = _replay(oracle, [om_prior] * 2, np.stack([_c4_p0(6, g, nw) for g in gs]), gs, burnin, nsteps, stacked=True)
    for i, g in enumerate(gs):
        _check_samples(a[g, :, 3:], chains[i].reshape(-1, 6), "at size, point %d" % g)


C5_BURN, C5_STEPS = 3, 6


@pytest.fixture(scope="module")
def c5_reference(oracle, harness):
    """A reduced sens_grid -- both dimensions, both textures, 2 sources, 3 scales (24 points) -- and two points of texture OUT,
    dimension 6 above it, where the reference's unitarity assert fires on part of the walkers (the grid's own top scale, -36.5,
    is short of it; a long chain drifts there), 32 walkers, 3 + 6 steps, replayed with on_nonunitary='-inf' -- stacked (seed 25,
    stream g) and one sampler per point (seed 25 + g, stream 0)."""
    from golemflavor_amd import scan
    pts = scan.sens_grid(n_scales=3, n_sources=2)
    assert len(pts) == 24 and {(d, t) for d, t, _, _ in pts} == {(3, Texture.OET), (3, Texture.OUT), (6, Texture.OET), (6, Texture.OUT)}
    pts += [(6, Texture.OUT, (0.0, 1.0, 0.0), -31.0), (6, Texture.OUT, (0.5, 0.5, 0.0), -30.5)]
    built = [_c5_model(oracle, p) for p in pts]
    p0 = np.stack([_c5_p0(box, lohi, p[3], g) for g, (p, (_, _, box, lohi)) in enumerate(zip(pts, built))])
    out = {}
    for stacked in (True, False):
        arbs = [Arbiter(oracle, om, m, harness=harness) for om, m, _, _ in built]
        gs = list(range(len(pts)))
        # the burn-in's non-unitary proposals are not counted by the device after reset(): count the stored run's apart
        chains = {}

        def run(idx, seed, sids):
            sub = [arbs[i] for i in idx]
            burn = reference_stretch(oracle, sub, p0[idx], C5_BURN, seed, lnprob=lambda a, th: a.lnprob(None, th),
                                     stream_ids=sids, full=True)
            before = sum(a.nbad for a in sub), sum(a.nband for a in sub)
            res = reference_stretch(oracle, sub, burn["pos"], C5_STEPS, seed, lnprob=lambda a, th: a.lnprob(None, th),
                                    stream_ids=sids, iteration0=C5_BURN, lnp0=burn["lnp"], full=True)
            return res["chain"], sum(a.nbad for a in sub) - before[0], sum(a.nband for a in sub) - before[1]
        if stacked:
            ch, nbad, nband = run(gs, SEED, gs)
            chains = {g: ch[g].reshape(-1, 12) for g in gs}
        else:
            nbad = nband = 0
            for g in gs:
                ch, b, n = run([g], SEED + g, [0])
                chains[g] = ch[0].reshape(-1, 12)
                nbad, nband = nbad + b, nband + n
        out[stacked] = (chains, nbad, nband)
    for _, m, _, _ in built:
        m.close()
    return pts, out


def test_c5_scan_every_delivery_path_equals_the_replay(c5_reference, monkeypatch):
    """C5 (the 12-column posterior of scripts/fr.py / sens.py): every point's chain is the replay of that point's posterior on
    stream g, with the proposals the reference would have died on rejected -- streamed (run_mcmc_to_host), read back after the
    run (GF_SCAN_NO_STREAMED_CHAIN=1: chain_to_device + exchange), gather=None and --no-stack."""
    from golemflavor_amd import scan
    pts, ref = c5_reference
    chains, nbad, nband = ref[True]
    print("C5 replay: %d non-unitary proposals in the stored run, %d in the band" % (nbad, nband))
    assert nbad > 0 and nband > 0                                        # the settle path contributes to the data checked
    n = len(pts)
    make = lambda p, g: scan._SensPoint(p, g, nwalkers=NW, device=0)    # noqa: E731
    for label in ("streamed", "read back after the run", "gather=None"):
        if label == "read back after the run":
            monkeypatch.setenv("GF_SCAN_NO_STREAMED_CHAIN", "1")
        stage, dg = (None, None) if label == "gather=None" else _device_gather()
        out = _as_list(scan.run_points(pts, list(range(n)), make, C5_BURN, C5_STEPS, gather=dg), n)
        monkeypatch.delenv("GF_SCAN_NO_STREAMED_CHAIN", raising=False)
        if stage is not None:
            stage.close()
        dev_bad = scan.LAST_NONUNITARY["nonunitary_proposals_rejected"]
        print("C5 %s: %s" % (label, {k: v for k, v in scan.LAST_NONUNITARY.items() if k != "host_thread_times"}))
        assert dev_bad > 0 and abs(dev_bad - nbad) <= nband, (label, dev_bad, nbad, nband)
        for g in range(n):
            assert out[g].shape == (NW * C5_STEPS, 12)
            _check_samples(out[g], chains[g], "C5 %s, point %d" % (label, g))
    chains, nbad, nband = ref[False]
    out = scan.run_points(pts, list(range(n)), make, C5_BURN, C5_STEPS, stacked=False)
    for g in range(n):
        _check_samples(out[g], chains[g], "C5 --no-stack, point %d" % g)
