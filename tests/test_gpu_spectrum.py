"""GPU: the composition at every energy bin (csrc/gf_spectrum.hip, golemflavor_amd/spectrum.py) -- the kernel against
the reference-generated golden and against two independent device paths, its status rule and launch shapes, and the reductions over
a sampler's chains, a nested run's posterior rows and a scan's grid points against numpy."""
import ctypes as C
import fractions
import json
import math
import os

import numpy as np
import pytest

from common import BIN_EDGES, TEX_BY_VALUE, uniform_theta
from golemflavor_amd import _lib, scan
from golemflavor_amd import configs as Cf
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import spectrum as sp
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import Param, ParamSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS_FR = 1e-10          # test_gpu_parity_r2.py: against the reference where it is itself accurate
EXACT_FR = 1e-11        # ... and against the exact value on every pair
U = 2.0 ** -53
STATUS_SEED = 11


@pytest.fixture(scope="module")
def gs():
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_spectrum.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def texture_model(dim, tex, source=(1., 2., 0.), binning=BIN_EDGES):
    return Model(compile_model(Cf.texture_paramset(dim), "BSM_GAUSS", texture=tex, dimension=dim, binning=np.asarray(binning, dtype=float),
                               source_ratio=source, bestfit_fr=(1 / 3,) * 3, smearing=0.02))


def test_golden_parity_per_row_and_bin(gs):
    worst_ref = worst_exact = 0.0
    nref = 0
    for ci, (dim, texv) in enumerate(gs["configs"]):
        with texture_model(int(dim), TEX_BY_VALUE[int(texv)], source=tuple(gs["source"]), binning=gs["binning"]) as m:
            assert m.nbins == 20
            f = m.propagate_bins(gs["theta"][ci], want_status=False)
        assert f.shape == (12, 20, 3) and np.isfinite(f).all()
        worst_exact = max(worst_exact, np.abs(f - gs["fr_exact"][ci]).max())
        clean = (gs["ok"][ci] == 1) & (np.abs(gs["abs2_diff"][ci]).max(axis=(2, 3)) < 1e-12)
        nref += int(clean.sum())
        worst_ref = max(worst_ref, np.abs(f[clean] - gs["fr_ref"][ci][clean]).max())
    print("per-bin parity: %d clean pairs, worst vs reference %.3e, worst vs exact %.3e" % (nref, worst_ref, worst_exact))
    assert nref >= 400
    assert worst_ref <= ABS_FR
    assert worst_exact <= EXACT_FR


def test_bin_k_equals_a_one_bin_model_at_its_centre():
    """Geometric binning of ratio 4: every centre 2 e0 4^k is exact in fp64, and so are the edges (centre / 2, 2 centre) of the one-bin
    model.  Same per-bin arithmetic; the one-bin flux average adds a multiply by the width, a three-term sum, a reciprocal and a
    product, each an ulp or two on values <= 1."""
    e0 = 65536.0
    edges = e0 * 4.0 ** np.arange(6)
    centres = np.sqrt(edges[:-1] * edges[1:])
    assert np.array_equal(centres, 2 * e0 * 4.0 ** np.arange(5))
    rng = np.random.default_rng(5)
    worst = 0.0
    for dim, tex in ((6, Texture.OET), (3, Texture.OUT)):
        th = uniform_theta(Cf.texture_paramset(dim), 200, rng, seeds=False)
        with texture_model(dim, tex, binning=edges) as m:
            f = m.propagate_bins(th, want_status=False)
        assert f.shape == (200, 5, 3)
        for k, c in enumerate(centres):
            with texture_model(dim, tex, binning=np.array([c / 2, 2 * c])) as m1:
                assert m1.nbins == 1 and np.sqrt(m1.desc.bin_edges[0] * m1.desc.bin_edges[1]) == c
                one = m1.propagate(th, want_status=False)
            worst = max(worst, np.abs(f[:, k, :] - one).max())
    print("bin k against the one-bin model: worst %.3e" % worst)
    assert worst <= 1e-14


def test_bins_recombine_to_the_flux_average():
    rng = np.random.default_rng(7)
    ps = Cf.texture_paramset(6)
    th = uniform_theta(ps, 1000, rng, seeds=False)
    with texture_model(6, Texture.OET) as m:
        f = m.propagate_bins(th, want_status=False)
        avg = m.propagate(th, want_status=False)
    assert np.abs(f.sum(axis=-1) - 1.0).max() <= 1e-13
    w = np.abs(np.diff(BIN_EDGES))
    rec = np.einsum("nkc,k->nc", f, w)
    rec /= rec.sum(axis=1, keepdims=True)
    print("recombination: worst %.3e" % np.abs(rec - avg).max())
    assert np.abs(rec - avg).max() <= 1e-14


def status_rows(lo, hi, n=512):
    rng = np.random.default_rng(STATUS_SEED)
    th = uniform_theta(Cf.texture_paramset(6), n, rng, seeds=True)
    th[:, 6] = rng.uniform(lo, hi, n)
    return th


LOW_EDGES = BIN_EDGES[:12]           # the default binning's first 11 bins, up to 1.00e6 GeV


def check_status_rule(th, binning=BIN_EDGES):
    """NaN in every bin exactly where propagate's status is not GF_ST_OK, finite elsewhere; without the status nothing is NaN and the
    finite rows are the same bits.  Returns the mask of the failing rows."""
    with texture_model(6, Texture.OEU, binning=binning) as m:
        _, st_avg = m.propagate(th)
        f, st = m.propagate_bins(th)
        raw = m.propagate_bins(th, want_status=False)
    assert f.shape == (len(th), len(binning) - 1, 3)
    assert np.array_equal(st, st_avg)
    bad = st != _lib.GF_ST_OK
    assert np.isnan(f[bad]).all() and np.isfinite(f[~bad]).all()
    assert np.isfinite(raw).all()
    assert np.array_equal(raw[~bad], f[~bad])                       # bitwise
    return bad


def test_status_rule_over_the_top_two_decades():
    """dim 6, OEU, source (1, 2, 0), logLam uniform over the top two decades of its range ([-32, -30]), 512 rows, both verdicts at
    least 8 times.  The verdict is the whole walker's, so it is the highest bin's: the new-physics term over the standard one grows
    as Lam E^4, and each default bin (ratio 1.29 in E) moves the scale at which the reference starts raising down by 0.44 decades.
    With all 20 default bins (to 1e7 GeV) that scale is logLam -36 to -35 and every row of [-32, -30] raises (next test); with
    the default bins below 1e6 GeV it lies inside [-32, -30].  The oracle's status (the reference's arithmetic) of this seed's
    rows, OK / NON_UNITARY, with the first k default bins: k <= 7: 512 / 0, 8: 490 / 22, 10: 330 / 182, 11: 226 / 286, 12: 103 / 409,
    14: 2 / 510, k >= 15: 0 / 512.  k = 11 is the most even."""
    hi = Cf.SCALE_BOUNDARIES[6][1]
    assert len(LOW_EDGES) == 12 and 0.99e6 < LOW_EDGES[-1] < 1.01e6
    bad = check_status_rule(status_rows(hi - 2.0, hi), binning=LOW_EDGES)
    print("top two decades, 11 bins below 1e6 GeV: %d failing rows, %d passing" % (bad.sum(), (~bad).sum()))
    assert bad.sum() >= 8 and (~bad).sum() >= 8


def test_status_rule_where_every_row_fails():
    """The same rows with all 20 default bins: the reference raises on every one of them (the oracle's status: 0 / 512), so every
    value is NaN with the status and finite without it."""
    hi = Cf.SCALE_BOUNDARIES[6][1]
    bad = check_status_rule(status_rows(hi - 2.0, hi))
    print("top two decades, default binning: %d failing rows, %d passing" % (bad.sum(), (~bad).sum()))
    assert bad.all()


def test_status_rule_across_the_transition():
    """The same checks with all 20 default bins, where both verdicts occur with them: logLam uniform over [-37, -34] (the oracle's
    status of this seed's rows: both kinds more than 100 times)."""
    bad = check_status_rule(status_rows(-37.0, -34.0))
    print("transition: %d failing rows, %d passing" % (bad.sum(), (~bad).sum()))
    assert bad.sum() >= 8 and (~bad).sum() >= 8


def _bins_device(m, th, nbins, bin_major, layout=_lib.GF_LAYOUT_AOS, status=None, guard=64):
    """propagate_bins_device into a buffer with `guard` sentinel doubles behind the output; returns (out, guard words)"""
    n = th.shape[0]
    total = n * nbins * 3
    host = np.full(total + guard, -7.25)
    d_out = m.alloc(host.nbytes).upload(host)
    src = th if layout == _lib.GF_LAYOUT_AOS else np.ascontiguousarray(th.T)
    d_th = m.alloc(src.nbytes).upload(src)
    d_st = m.alloc(4 * n).upload(status) if status is not None else None
    try:
        m.propagate_bins_device(d_th.ptr, n, d_out.ptr, d_st.ptr if d_st is not None else None, bin_major=bin_major, layout=layout)
        m.sync()
        back = d_out.download((total + guard,))
    finally:
        for b in (d_out, d_th, d_st):
            if b is not None:
                b.free()
    shape = (nbins, n, 3) if bin_major else (n, nbins, 3)
    return back[:total].reshape(shape), back[total:]


@pytest.mark.parametrize("nbins_e", [1, 3, 20, 64])
def test_launch_shapes_layouts_and_guard_words(nbins_e):
    rng = np.random.default_rng(100 + nbins_e)
    edges = np.logspace(np.log10(6e4), np.log10(1e7), nbins_e + 1)
    ps7 = Cf.texture_paramset(6)
    _, ps12 = Cf.fr_paramsets(6, (0.4, 0.0))
    ps_none = ParamSet(list(ps7)[:6] + [Param(name="np_s12_2", value=0.5, ranges=[0., 1.], std=0.2, tag=ParamTag.MMANGLES),
                                        Param(name="np_c13_4", value=0.5, ranges=[0., 1.], std=0.2, tag=ParamTag.MMANGLES),
                                        Param(name="np_s23_2", value=0.5, ranges=[0., 1.], std=0.2, tag=ParamTag.MMANGLES),
                                        Param(name="np_dcp", value=1.0, ranges=[0., 2 * np.pi], std=0.2, tag=ParamTag.MMANGLES),
                                        list(ps7)[6]])
    cases = (("7 columns", ps7, Texture.OET), ("12 columns", ps12, Texture.OUT), ("NONE, sampled NP angles", ps_none, Texture.NONE))
    for what, ps, tex in cases:
        desc = compile_model(ps, "BSM_GAUSS", texture=tex, dimension=6, binning=edges, source_ratio=(1., 2., 0.), bestfit_fr=(1 / 3,) * 3,
                             smearing=0.02)
        with Model(desc) as m:
            assert m.nbins == nbins_e
            for n in (1, 63, 64, 65, 257):
                th = uniform_theta(ps, n, rng, seeds=False)
                want = m.propagate_bins(th, want_status=False)
                assert want.shape == (n, nbins_e, 3) and np.isfinite(want).all(), (what, n)
                for layout in (_lib.GF_LAYOUT_AOS, _lib.GF_LAYOUT_SOA):
                    row, g0 = _bins_device(m, th, nbins_e, False, layout)
                    binm, g1 = _bins_device(m, th, nbins_e, True, layout)
                    assert np.array_equal(row, want), (what, n, layout)
                    assert np.array_equal(binm, np.transpose(row, (1, 0, 2))), (what, n, layout)      # a permutation, bitwise
                    assert np.all(g0 == -7.25) and np.all(g1 == -7.25), (what, n, layout)
                # the rows of a batch do not depend on the batch: row j alone
                j = n // 2
                assert np.array_equal(m.propagate_bins(th[j:j + 1], want_status=False)[0], want[j]), (what, n)


def test_device_status_masks_rows_in_both_layouts():
    th = status_rows(-37.0, -34.0, 130)
    st = np.zeros(130, np.int32)
    st[[0, 64, 129]] = [_lib.GF_ST_NON_UNITARY, _lib.GF_ST_NAN, _lib.GF_ST_OUT_OF_PRIOR]
    with texture_model(6, Texture.OEU) as m:
        raw = m.propagate_bins(th, want_status=False)
        for bin_major in (False, True):
            got, guard = _bins_device(m, th, 20, bin_major, status=st)
            got = np.transpose(got, (1, 0, 2)) if bin_major else got
            assert np.isnan(got[st != 0]).all() and np.array_equal(got[st == 0], raw[st == 0]) and np.all(guard == -7.25)


def numpy_spectrum_matches(r, f, edges, q, bins, what, exact_moments_bins=()):
    """`r` against numpy on host compositions f (n, nbinsE, 3): counts and percentiles exactly, nvalid, and mean / cov under the
    summation-tree bars of test_gpu_marginals.py."""
    good = f[~np.isnan(f).any(axis=(1, 2))]
    nv, nE = len(good), f.shape[1]
    assert np.array_equal(r.energies, np.sqrt(edges[:-1] * edges[1:])) and np.array_equal(r.widths, np.abs(np.diff(edges)))
    assert r.nvalid.tolist() == [nv] * nE, what
    d = mg.moment_tree_depth(nv)
    for k in range(nE):
        for c in range(3):
            x = good[:, k, c]
            assert np.array_equal(r.counts[k, c], np.histogram(x, bins=bins, range=(0., 1.))[0].astype(np.uint64)), (what, k, c)
            assert np.array_equal(r.percentiles[k, c], np.percentile(x, q)), (what, k, c)
            exact = fractions.Fraction(math.fsum(x)) / nv
            bound = (d + 2) * U * math.fsum(np.abs(x)) / nv
            assert abs(fractions.Fraction(float(r.mean[k, c])) - exact) <= bound, (what, k, c)
        assert np.array_equal(r.cov[k], r.cov[k].T), (what, k)
    for k in exact_moments_bins:
        F = [[fractions.Fraction(float(t)) for t in good[:, k, c]] for c in range(3)]
        mu = [sum(col) / nv for col in F]
        B = [(d + 1) * U * float(sum(abs(t) for t in col)) / nv for col in F]
        m = [fractions.Fraction(float(t)) for t in r.mean[k]]
        for i in range(3):
            assert abs(m[i] - mu[i]) <= B[i], (what, k, i)
            for j in range(3):
                exact = sum((a - mu[i]) * (b - mu[j]) for a, b in zip(F[i], F[j])) / (nv - 1)
                sabs = float(sum(abs((a - m[i]) * (b - m[j])) for a, b in zip(F[i], F[j])))
                bound = ((d + 4) * U * sabs + nv * B[i] * B[j]) / (nv - 1)
                assert abs(fractions.Fraction(float(r.cov[k, i, j])) - exact) <= bound, (what, k, i, j)


def same_spectrum(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in sp.SpectrumResult.ARRAYS)


def test_sampler_spectrum_against_numpy_and_alone():
    """Three chains of the 12-column BSM posterior with different dimensions, textures, sources and scales, at the smallest even
    walker count the sampler accepts for 12 columns (2 ndim), 40 stored steps."""
    grid = scan.sens_grid()
    pts = [grid[3], grid[70], grid[-1]]
    nw, q, bins = 24, (5., 16., 50., 84., 95.), 50
    jobs = [scan._SensPoint(p, g, nwalkers=nw, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(nw, 12, [j.f for j in jobs], seed=25, stream_ids=[0, 1, 2])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 40)
        chain = s.flat_steps()
        assert chain.shape == (3, nw * 40, 12)
        got = s.spectrum(percentiles=q, bins=bins)
        assert len(got) == 3
        for ch in range(3):
            f, st = jobs[ch].f.model.propagate_bins(chain[ch])
            assert np.array_equal(np.isnan(f).any(axis=(1, 2)), st != _lib.GF_ST_OK)
            numpy_spectrum_matches(got[ch], f, BIN_EDGES, q, bins, "chain %d" % ch, exact_moments_bins=(0, 19))
            assert np.abs(got[ch].flux_average().sum() - 1) < 1e-15
        # other settings go through
        r = s.spectrum(percentiles=(50.,), bins=7)
        f, _ = jobs[1].f.model.propagate_bins(chain[1])
        numpy_spectrum_matches(r[1], f, BIN_EDGES, (50.,), 7, "chain 1, 7 bins")
    finally:
        s.close()
    # chain 1 alone, same random stream: the same chain and the same bits in every array
    alone = mcmc_utils.DeviceEnsembleSampler(nw, 12, [jobs[1].f], seed=25, stream_ids=[1])
    alone.on_nonunitary = "-inf"
    try:
        alone.run_mcmc(jobs[1].p0[None], 40)
        assert np.array_equal(alone.flat_steps().reshape(-1, 12), chain[1])
        assert same_spectrum(alone.spectrum(percentiles=q, bins=bins), got[1])
    finally:
        alone.close()
        for j in jobs:
            j.close()


def test_sampler_spectrum_with_post_processing_models():
    """mc_texture's path: the chains sample the priors and every sample goes through the grid point's BSM model."""
    grid = scan.texture_grid(6)
    pts = [grid[2], grid[30], grid[61]]
    nw, q = 12, (16., 50., 84.)
    jobs = [scan._TexturePoint(p, g, dimension=6, texture=Texture.OET, nwalkers=nw, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(nw, 6, [j.f for j in jobs], seed=25, stream_ids=[0, 1, 2])
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 40)
        chain = s.flat_steps()
        models = [j.post_model for j in jobs]
        got = s.spectrum(percentiles=q, bins=25, models=models)
        rows = s.postprocess_rows(models=models)
        with pytest.raises(ValueError):
            s.spectrum()                                             # the sampling models are prior-only: no energy bins
        for ch in range(3):
            f, st = models[ch].propagate_bins(chain[ch])
            numpy_spectrum_matches(got[ch], f, BIN_EDGES, q, 25, "texture chain %d" % ch, exact_moments_bins=(19,))
            # the same samples have a composition as in the rows a scan saves
            assert np.array_equal(np.isnan(rows[ch][:, 0]), st != _lib.GF_ST_OK)
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_nested_spectrum_equals_numpy_on_the_posterior_rows():
    import argparse
    from golemflavor_amd import nested
    args = argparse.Namespace(source_ratio=(0., 1., 0.), dimension=6, texture=Texture.OET, binning=BIN_EDGES)
    asimov, ps = Cf.sens_paramsets(6, (1, 1, 1))
    scales = nested.sens_scales(6, 4)[1:3]
    res = nested.evidence_scan(args, asimov, ps, scales, nlive=200, seed=3, on_nonunitary="-inf", return_sampler=True)
    s = res["sampler"]
    try:
        q = (5., 50., 95.)
        got = s.spectrum(256, percentiles=q, bins=20)
        rows = s.posterior_rows(256)
        assert len(got) == s.nruns == 2
        for r in range(s.nruns):
            f, _ = getattr(s.models[r], "model", s.models[r]).propagate_bins(rows[r])
            numpy_spectrum_matches(got[r], f, BIN_EDGES, q, 20, "run %d" % r, exact_moments_bins=(0,))
    finally:
        s.close()
        for m in s.models:
            m.close()


def test_scan_writes_one_spectrum_per_point_equal_to_the_api(tmp_path, capsys):
    d = str(tmp_path / "scan")
    scan.main(["--config", "C4", "--points", "3", "--nwalkers", "32", "--burnin", "10", "--nsteps", "30", "--datadir", d,
               "--spectrum", "16", "50", "84", "--spectrum-bins", "30"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["spectrum"]["points"] == 3 and line["spectrum"]["percentiles"] == [16., 50., 84.] and line["spectrum"]["bins"] == 30
    chains = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert len(chains) == 3 and sorted(os.listdir(d)) == sorted(chains + ["spectrum_%s.npz" % f[:-4] for f in chains])
    pts = scan.texture_grid(6)[:3]
    for g, p in enumerate(pts):
        ns = argparse_namespace(p)
        stem = scan.point_filename("C4", p, ns)
        rows = np.load(os.path.join(d, stem + ".npy"))
        assert rows.shape == (32 * 30, 9)
        z = sp.SpectrumResult.load(os.path.join(d, "spectrum_%s.npz" % stem))
        job = scan._TexturePoint(p, g, dimension=6, texture=Texture.OET, nwalkers=32, device=0)
        try:
            f, st = job.post_model.propagate_bins(rows[:, 3:])
        finally:
            job.close()
        assert np.array_equal(np.isnan(rows[:, 0]), st != _lib.GF_ST_OK)
        numpy_spectrum_matches(z, f, BIN_EDGES, (16., 50., 84.), 30, "point %d" % g)
        # and the flux average of the mean spectrum is the mean of the saved compositions, up to the two orders of summation
        fin = ~np.isnan(rows[:, 0])
        assert np.abs(z.flux_average() - rows[fin, :3].mean(axis=0)).max() < 1e-12


def argparse_namespace(point):
    import argparse
    return argparse.Namespace(dimension=6, texture="OET")


def test_models_without_energy_bins_are_refused():
    ang = (0.5, 0.2)
    asimov, ps = Cf.notebook_paramsets(ang)
    for desc in (compile_model(ps, "SM_GAUSS", bestfit_fr=(1 / 3,) * 3, smearing=0.02), compile_model(Cf.unitary_paramset(), "PRIOR_ONLY")):
        with Model(desc) as m:
            assert m.nbins == 0
            th = np.zeros((4, m.ndim))
            with pytest.raises(ValueError):
                m.propagate_bins(th)
            with pytest.raises(ValueError):
                m.propagate_bins_device(None, 4, None)
            # the C entry points say so themselves, before anything is launched
            out = np.zeros((4, 1, 3))
            rc = m._L.gf_propagate_bins(m._h, th.ctypes.data_as(_lib._dp), 4, out.ctypes.data_as(_lib._dp), None)
            assert rc == _lib.GF_ERR_UNSUPPORTED
            assert m._L.gf_propagate_bins_device(m._h, None, 0, 4, None, 0, None) == _lib.GF_ERR_UNSUPPORTED
            s = mcmc_utils.DeviceEnsembleSampler(2 * m.ndim, m.ndim, m, seed=1)
            try:
                s.run_mcmc(mcmc_utils.flat_seed(ps if m.ndim == len(ps) else Cf.unitary_paramset(), 2 * m.ndim), 4)
                with pytest.raises(ValueError):
                    s.spectrum()
                spec = _lib.GfSpectrumSpec(10, 0, None)
                o = _lib.GfSpectrumOut()
                assert m._L.gf_sampler_spectrum(s._h, None, C.byref(spec), C.byref(o)) == _lib.GF_ERR_UNSUPPORTED
            finally:
                s.close()
