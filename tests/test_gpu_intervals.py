"""The shortest interval around the mode on the device (csrc/gf_interval.hip): the segmented radix sort against np.sort, the
intervals against the reference's goldens (tests/golden/golden_interval.npz; here they are data: the reference is not imported) and
against the numpy restatement `intervals.interval_host`, exactly as numbers throughout; the batching; the sampler entry points.

Tile of the sort: 4096 keys (256 threads x 16)."""
import json
import os

import numpy as np
import pytest

import interval_harness as H
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import intervals as iv
from golemflavor_amd import llh as llh_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import nested, scan
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


# ---- the sort ----------------------------------------------------------------------------------------------------------------------
def sort_rows(nchains, n, width, seed):
    """rows with negatives, +/-0, denormals and duplicates in every column; column 0: its values share the upper six key bytes"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nchains, n, width)) * 10. ** rng.integers(-3, 4, (1, 1, width))
    pick = rng.random(x.shape)
    x[pick < 0.05] = 0.0
    x[(pick >= 0.05) & (pick < 0.10)] = -0.0
    x[(pick >= 0.10) & (pick < 0.15)] = 5e-324 * rng.integers(1, 1000, x.shape)[(pick >= 0.10) & (pick < 0.15)]
    x[(pick >= 0.15) & (pick < 0.18)] *= -1e-310 / np.maximum(np.abs(x[(pick >= 0.15) & (pick < 0.18)]), 1e-300)
    dup = (pick >= 0.18) & (pick < 0.40)
    x[dup] = np.round(x[dup], 1)
    x[:, :, 0] = 1.0 + rng.integers(0, 65536, (nchains, n)) * 2. ** -52
    return x


def check_sorted(got, x, skip=()):
    nchains, n, width = x.shape
    assert got.shape == (nchains, width, n)
    for ch in range(nchains):
        for c in range(width):
            if (ch, c) in skip:
                continue
            want = np.sort(x[ch, :, c])
            assert np.array_equal(got[ch, c], want), (ch, c)
            # +/-0.0 are one number to np.sort: every one is there, and the negative ones come first
            z = got[ch, c][got[ch, c] == 0]
            assert np.signbit(z).sum() == np.signbit(x[ch, :, c][x[ch, :, c] == 0]).sum() and np.all(np.diff(np.signbit(z).astype(int)) <= 0), (ch, c)


@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("width", [1, 4, 12, 15])
def test_sort_equals_np_sort(model, nchains, width):
    for k, n in enumerate((1, 2, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)):
        x = sort_rows(nchains, n, width, 100 * width + 10 * nchains + k)
        check_sorted(iv.sort_columns(x, model=model), x)


def test_non_finite_values_flag_their_column_only(model):
    n, width = 4097, 5
    x = sort_rows(2, n, width, 7)
    clean = iv.sort_columns(x, model=model)
    base = iv.chain_intervals(x, model=model, percentiles=(68., 90.))
    y = x.copy()
    y[0, 17, 1] = np.inf
    y[0, 4096, 2] = -np.inf
    y[1, 300, 3] = np.nan
    y[1, 301, 3] = -np.nan
    got = iv.sort_columns(y, model=model)
    bad = {(0, 1), (0, 2), (1, 3)}
    check_sorted(got, y, skip=bad)
    for ch in range(2):
        for c in range(width):
            if (ch, c) not in bad:
                assert np.array_equal(got[ch, c], clean[ch, c])
    assert got[0, 1, -1] == np.inf and np.array_equal(got[0, 1, :-1], np.sort(y[0, :, 1])[:-1])
    assert got[0, 2, 0] == -np.inf and np.array_equal(got[0, 2, 1:], np.sort(y[0, :, 2])[1:])
    assert np.all(np.isnan(got[1, 3, -2:])) and np.array_equal(got[1, 3, :-2], np.sort(y[1, :, 3])[:-2])      # every NaN last
    r = iv.chain_intervals(y, model=model, percentiles=(68., 90.))
    for ch in range(2):
        for c in range(width):
            if (ch, c) in bad:
                assert list(r["status"][ch, c]) == [1, 1] and r["nunique"][ch, c] == -1 and r["nbins"][ch, c] == -1
                assert np.all(np.isnan(r["low"][ch, c])) and np.all(np.isnan(r["up"][ch, c])) and np.isnan(r["center"][ch, c])
            else:
                for f in iv.FIELDS:
                    assert H.same_numbers(r[f][ch, c], base[f][ch, c]), (f, ch, c)


# ---- the intervals -----------------------------------------------------------------------------------------------------------------
def test_goldens_on_the_device(model):
    """every golden: the columns of equal length packed into one chain, the others one chain each"""
    by_len = {}
    for g in H.goldens():
        by_len.setdefault(len(g[1]), []).append(g)
    assert sorted(len(v) for v in by_len.values())[-1] >= 6          # the 4096-value cases share a chain
    seen = 0
    for n, gs in by_len.items():
        rows = np.stack([g[1] for g in gs], axis=1)
        pct = gs[0][2]
        got = iv.chain_intervals(rows, model=model, percentiles=pct)
        for c, (name, x, _, low, center, up, status, nbins) in enumerate(gs):
            assert np.array_equal(got["status"][c], status), (name, got["status"][c], status)
            assert H.same_numbers(got["low"][c], low) and H.same_numbers(got["up"][c], up), (name, got["low"][c], low, got["up"][c], up)
            if np.any(status == 0):
                assert got["center"][c] == center[status == 0][0], name
            assert got["nbins"][c] == (-1 if np.isnan(nbins) else int(nbins)), name
            assert got["nunique"][c] == len(np.unique(x)), name
            seen += 1
    assert seen == 12


AR1 = [((300, 4), 11), ((4097, 7), 12), ((20000, 12), 13)]
PCT = (68., 90., 100.)


@pytest.fixture(scope="module")
def ar1():
    """the rows (three stacked chains each) and the restatement's results, computed once"""
    out = {}
    for (n, w), seed in AR1:
        x = H.ar1_rows(n, w, 3, seed)
        out[(n, w)] = (x, [iv.rows_intervals_host(x[ch], PCT) for ch in range(3)])
    return out


@pytest.mark.parametrize("shape", [s for s, _ in AR1], ids=["%dx%d" % s for s, _ in AR1])
def test_device_equals_the_restatement(model, ar1, shape):
    x, want = ar1[shape]
    got = iv.chain_intervals(x, model=model, percentiles=PCT)
    for ch in range(3):
        H.assert_same_result({f: got[f][ch] for f in iv.FIELDS}, want[ch], "%s chain %d" % (shape, ch))
    assert np.all(got["status"][:, :, :2] == 0) and np.all(got["status"][:, :, 2] == 3)
    # one chain alone, from host rows: the same numbers
    one = iv.chain_intervals(x[1], model=model, percentiles=PCT)
    H.assert_same_result(one, {f: got[f][1] for f in iv.FIELDS}, "%s chain 1 alone" % (shape,))
    # the order of the percentiles changes nothing
    rev = iv.chain_intervals(x[2], model=model, percentiles=PCT[::-1])
    assert H.same_numbers(rev["low"][:, ::-1], got["low"][2]) and H.same_numbers(rev["up"][:, ::-1], got["up"][2])


def test_batching_changes_no_bit(model, ar1, monkeypatch):
    x, _ = ar1[(4097, 7)]
    whole = iv.chain_intervals(x, model=model, percentiles=PCT)
    sorted_whole = iv.sort_columns(x, model=model)
    monkeypatch.setenv("GF_INTERVAL_SCRATCH_BYTES", "1")             # below one chain's buffers: one chain per batch
    split = iv.chain_intervals(x, model=model, percentiles=PCT)
    sorted_split = iv.sort_columns(x, model=model)
    for f in iv.FIELDS:
        a, b = np.ascontiguousarray(whole[f]), np.ascontiguousarray(split[f])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert sorted_whole.tobytes() == sorted_split.tobytes()
    monkeypatch.setenv("GF_INTERVAL_SCRATCH_BYTES", str(2 * 2 * 8 * 7 * 4097))      # two chains, then one
    two = iv.chain_intervals(x, model=model, percentiles=PCT)
    for f in iv.FIELDS:
        assert np.ascontiguousarray(whole[f]).tobytes() == np.ascontiguousarray(two[f]).tobytes(), f


def test_arguments(model):
    x = np.zeros((4, 2))
    for bad in ((), (0.,), (100.5,), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            iv.chain_intervals(x, model=model, percentiles=bad)
    with pytest.raises(ValueError):
        iv.chain_intervals(np.zeros((0, 2)), model=model)
    with pytest.raises(Exception, match="invalid argument"):
        iv.chain_intervals(np.zeros((4, 20)), model=model)
    r = iv.chain_intervals(x, model=model)                            # constant columns: status 2, one distinct value
    assert np.all(r["status"] == 2) and list(r["nunique"]) == [1, 1] and list(r["percentiles"]) == [68., 90.]


# ---- the other entry points ------------------------------------------------------------------------------------------------------------
def same_as_rows(got, rows, model, pct):
    want = iv.chain_intervals(rows, model=model, percentiles=pct)
    for f in iv.FIELDS:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), f
    return want


def test_sampler_theta_and_elements(model):
    pts = scan.sens_grid()[:2]
    jobs = [scan._SensPoint(p, g, nwalkers=128, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(128, 12, [j.f for j in jobs], seed=25, stream_ids=[0, 1])
    s.on_nonunitary = "-inf"
    try:
        with pytest.raises(ValueError, match="no stored samples"):
            s.intervals()
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 40)
        x = s.flat_steps()
        assert x.shape == (2, 128 * 40, 12)
        got = s.intervals(percentiles=PCT)
        want = same_as_rows(got, x, model, PCT)
        # against the restatement too, and the stretch move repeats rows: fewer distinct values than rows
        for ch in range(2):
            H.assert_same_result({f: got[f][ch] for f in iv.FIELDS}, iv.rows_intervals_host(x[ch], PCT), "chain %d" % ch)
        assert np.all(want["nunique"] < 128 * 40) and np.all(want["nunique"] > 128)
        from golemflavor_amd import elements as el
        ps = scan._SensPoint.descriptor(pts[0])[0]
        plan, names, _ = el.element_plan(ps)
        erows = np.stack([el.element_rows(x[ch], plan, model=model) for ch in range(2)])
        assert erows.shape[2] == len(names)
        same_as_rows(s.intervals(percentiles=PCT, space="elements", llh_paramset=ps), erows, model, PCT)
        with pytest.raises(ValueError):
            s.intervals(space="elements")
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_sampler_with_fr(model):
    pts = scan.texture_grid(6)[:2]
    jobs = [scan._TexturePoint(p, g, dimension=6, texture=scan.Texture.OET, nwalkers=128, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(128, 6, [j.f for j in jobs], seed=25, stream_ids=[0, 1])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 40)
        models = [j.post_model for j in jobs]
        rows = s.postprocess_rows(models=models)
        same_as_rows(s.intervals(percentiles=(68., 90.), with_fr=True, models=models), rows, model, (68., 90.))
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_nested_runs(model):
    fs = []
    for sm in (0.05, 0.08):
        asimov, ps = Cf.tutorial_paramsets(fr_utils.fr_to_angles((1., 2., 0.)), smearing=sm)
        fs.append(llh_utils.tutorial_ln_prob(asimov, ps))
    try:
        with nested.NestedSampler(fs, [0, 1], np.zeros(2), run_ids=[5, 6], nlive=100, batch=12, walks=10, seed=3) as s:
            s.run()
            for with_fr in (False, True):
                rows = s.posterior_rows(1000, with_fr=with_fr)
                same_as_rows(s.intervals(1000, percentiles=(68., 90.), with_fr=with_fr), rows, model, (68., 90.))
    finally:
        for f in fs:
            f.close()


def test_scan_writes_intervals_for_a_c5_shaped_run(model, tmp_path, capsys):
    d = str(tmp_path / "c5")
    scan.main(["--config", "C5", "--points", "3", "--nwalkers", "64", "--burnin", "5", "--nsteps", "30", "--datadir", d, "--intervals", "68", "90", "99"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["intervals"]["points"] == 3 and line["intervals"]["percentiles"] == [68., 90., 99.]
    chains = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert len(chains) == 3 and sorted(os.listdir(d)) == sorted(chains + ["intervals_%s.npz" % f[:-4] for f in chains])
    for f in chains:
        rows = np.load(os.path.join(d, f))
        z = np.load(os.path.join(d, "intervals_%s.npz" % f[:-4]))
        assert rows.shape == (64 * 30, 12) and z["low"].shape == (12, 3) and len(z["names"]) == 12
        want = iv.chain_intervals(rows, model=model, percentiles=(68., 90., 99.))
        for k in iv.FIELDS:
            assert H.same_numbers(z[k], want[k]), (f, k)
