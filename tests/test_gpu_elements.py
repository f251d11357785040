"""The element-space transform on the device (csrc/gf_elements.hip) and the marginals of a chain in element space.

The device build of the moduli is held to the assertions of tests/test_elements_host.py: same tolerance, same cap, same input.
`sampler.marginals(space="elements")` is held to the two-step path (get the chain, `element_rows`, `chain_marginals`), which it
must equal in every array."""
import numpy as np
import pytest

import elements_harness as H
from golemflavor_amd import configs as Cf
from golemflavor_amd import elements as el
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import marginals as mg
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import scan
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

U9 = [(el.GF_ELEMENT_U9, [0, 1, 2, 3])]


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


@pytest.fixture(scope="module")
def mixing():
    """the CPU test's input (the edge rows alone would exceed the cap on entries near a float32 boundary), with the oracle's moduli"""
    x = H.mixing_input()
    return x, H.oracle_absu(x)


def device_rows(model, rows, plan):
    """gf_element_rows_device on uploaded rows"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    w = el.plan_width(plan, rows.shape[1])
    d_in, d_out = model.alloc(max(rows.nbytes, 8)), model.alloc(max(8 * rows.shape[0] * w, 8))
    try:
        d_in.upload(rows)
        el.element_rows_device(d_in, rows.shape[0], rows.shape[1], plan, d_out, model=model)
        return d_out.download((rows.shape[0], w))
    finally:
        d_in.free()
        d_out.free()


def test_device_moduli_against_the_oracle(model, mixing):
    x, ref = mixing
    got = device_rows(model, x, el.make_plan(U9, round32=False))
    H.check_moduli(got, ref, "device")
    P = got.reshape(-1, 3, 3) ** 2
    assert np.abs(P.sum(axis=2) - 1).max() <= H.TOL and np.abs(P.sum(axis=1) - 1).max() <= H.TOL


def test_device_float32_column_exact_away_from_boundaries(model, mixing):
    x, ref = mixing
    near, steps = H.float32_steps(device_rows(model, x, el.make_plan(U9, round32=True)), ref, "device")
    assert near.mean() <= H.F32_EXCLUDED_CAP
    assert not steps[~near].any()


def test_device_float32_column_within_one_step_near_boundaries(model, mixing):
    """on the entries the first assertion leaves out: one float32 step at most (k_element_rows_exact's rows among them)"""
    x, ref = mixing
    near, steps = H.float32_steps(device_rows(model, x, el.make_plan(U9, round32=True)), ref, "device")
    assert steps[near].max(initial=0) <= 1


def test_device_source_composition_against_the_oracle(model):
    x = H.source_input()
    got = device_rows(model, x, el.make_plan([(el.GF_ELEMENT_FR3, [0, 1])]))
    err = np.abs(got - H.oracle_fr(x))
    print("device fractions: max abs err %.3e" % err.max())
    assert err.max() <= H.TOL
    assert got.min() >= 0 and np.abs(got.sum(axis=1) - 1).max() <= H.TOL


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 256 * 8 * 256 * 2 + 77])
def test_row_counts_either_side_of_every_tile_boundary(model, n):
    """1, 63 / 64 / 65 (a wave's tile), 1000 (no multiple of a block's 256 rows), more than one pass of the largest grid
    (8 blocks of 256 rows on each of at most 256 compute units): the device rows equal the host build's in the copied columns
    bit for bit and within the oracle's tolerance elsewhere, and gf_element_rows (host rows) equals the device entry bit for bit."""
    L = H.build()
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 1, size=(n, 7))
    x[:, 4] *= 2 * np.pi
    plan = el.make_plan([(el.GF_ELEMENT_COPY, [0]), (el.GF_ELEMENT_U9, [1, 3, 5, 4]), (el.GF_ELEMENT_FR3, [6, 2]), (el.GF_ELEMENT_COPY, [6])],
                        round32=False)
    got, want = device_rows(model, x, plan), H.host_rows(L, plan, x)
    assert got.shape == (n, 14)
    assert np.array_equal(got[:, [0, 13]], x[:, [0, 6]])
    assert np.abs(got - want).max() <= H.TOL
    assert np.array_equal(el.element_rows(x, plan, model=model), got)


@pytest.mark.parametrize("width", list(range(2, 17)))
def test_input_widths_with_groups_at_odd_positions(model, width):
    L = H.build()
    rng = np.random.default_rng(width)
    n = 4099
    x = rng.uniform(0, 1, size=(n, width))
    x[::97, rng.integers(width)] = np.nan
    cols = list(rng.permutation(width))
    groups = []
    if width >= 6:
        groups.append((el.GF_ELEMENT_U9, cols[:4]))
        x[:, cols[3]] *= 2 * np.pi
        cols = cols[4:]
    groups.append((el.GF_ELEMENT_FR3, cols[:2]))
    groups += [(el.GF_ELEMENT_COPY, [c]) for c in cols[2:]][:el.GF_ELEMENT_MAX_WIDTH - (12 if width >= 6 else 3)]
    for r32 in (False, True):
        plan = el.make_plan(groups[::-1] if width % 2 else groups, round32=r32)
        got, want = device_rows(model, x, plan), H.host_rows(L, plan, x)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= (2.0 ** -24 if r32 else H.TOL)      # one float32 step at most where rounded
        assert np.array_equal(el.element_rows(x, plan, model=model), got, equal_nan=True)


def test_invalid_plans_are_refused_by_the_entry_points(model):
    """GF_ERR_INVALID_ARG from the C entry points themselves (the Python wrappers check the plan before they call)"""
    import ctypes as C
    from golemflavor_amd import _lib
    L = _lib.lib()
    x = np.zeros((4, 5))
    out = np.zeros((4, 32))
    d_in, d_out = model.alloc(x.nbytes), model.alloc(out.nbytes)
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=(1., 0., 0.), flat_llh=1.0))
    s = mcmc_utils.DeviceEnsembleSampler(8, 4, m, seed=1)
    try:
        s.run_mcmc(np.random.default_rng(0).uniform(0.2, 0.8, size=(8, 4)), 4)
        prep = mg.prepare(9, [(0., 1.)] * 9)
        for bad, win in ((el.make_plan([(el.GF_ELEMENT_COPY, [5])]), 5),                     # column out of range
                         (el.make_plan([(el.GF_ELEMENT_U9, [0, 1, 2, 3])] * 3), 5),          # 27 output columns
                         (el.make_plan(U9), 17), (_lib.GfElementPlan(), 5)):                 # too many input columns; no group
            assert L.gf_element_rows(model._h, x.ctypes.data_as(_lib._dp), 4, win, C.byref(bad), out.ctypes.data_as(_lib._dp)) \
                == _lib.GF_ERR_INVALID_ARG
            assert L.gf_element_rows_device(model._h, d_in.ptr, 4, win, C.byref(bad), d_out.ptr) == _lib.GF_ERR_INVALID_ARG
            if win == 5:                                                                     # the sampler's rows have 4 columns: invalid there too
                with pytest.raises(_lib.GolemHipError) as err:
                    mg.run_marginal_call(lambda spec, o: L.gf_sampler_element_marginals(s._h, C.byref(bad), spec, o), "bad plan", 1, prep)
                assert err.value.code == _lib.GF_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            el.element_rows(x, el.make_plan([(el.GF_ELEMENT_COPY, [5])]), model=model)
    finally:
        s.close()
        m.close()
        d_in.free()
        d_out.free()


# ---- sampled chains ----------------------------------------------------------------------------------------------------------------
def same_marginals(a, b):
    x, y = a.as_arrays(), b.as_arrays()
    assert set(x) == set(y)
    for k in x:
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"), k
    return True


def check_sampler(s, ps, model, nchains):
    """space="elements" against get the chain -> element_rows -> chain_marginals; the default result before and after"""
    before = s.marginals()
    x = s.flat_steps().reshape(nchains, -1, len(ps))
    got = s.marginals(space="elements", llh_paramset=ps)
    got = [got] if nchains == 1 else got
    plan, names, ranges = el.element_plan(ps)
    rows = el.element_rows(x, plan, model=model)
    assert rows.shape == x.shape[:2] + (len(names),)
    want = mg.chain_marginals(rows, ranges, model=model, names=names)
    for ch in range(nchains):
        assert list(got[ch].names) == list(names) and same_marginals(got[ch], want[ch])
        for c in range(len(names)):
            assert np.array_equal(got[ch].counts1[c], np.histogram(rows[ch][:, c], bins=100, range=ranges[c])[0]), (ch, c)
    after = s.marginals()
    for a, b in zip([before] if nchains == 1 else before, [after] if nchains == 1 else after):
        assert same_marginals(a, b)                                                   # the stored chain was only read
    assert np.array_equal(s.flat_steps().reshape(x.shape), x)
    off = s.marginals(space="elements", llh_paramset=ps, round32=False)
    off = [off] if nchains == 1 else off
    want64 = mg.chain_marginals(el.element_rows(x, el.element_plan(ps, round32=False)[0], model=model), ranges, model=model, names=names)
    assert all(same_marginals(a, b) for a, b in zip(off, want64))
    with pytest.raises(ValueError):
        s.marginals(space="elements", llh_paramset=ps, with_fr=True)
    with pytest.raises(ValueError):
        s.marginals(space="elements")
    return got


def test_notebook_chain_in_element_space(model):
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    m = Model(compile_model(ps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02))
    np.random.seed(4)
    s = mcmc_utils.DeviceEnsembleSampler(512, 6, m, seed=8)
    try:
        s.run_mcmc(mcmc_utils.flat_seed(ps, 512), 200)
        got = check_sampler(s, ps, model, 1)[0]
        assert list(got.names) == list(el.U_NAMES + el.FR_NAMES) and got.nvalid == 512 * 200
    finally:
        s.close()
        m.close()


def test_c4_shaped_chains_in_element_space(model):
    pts = scan.texture_grid(6)[:2]
    jobs = [scan._TexturePoint(p, g, dimension=6, texture=scan.Texture.OET, nwalkers=256, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(256, 6, [j.f for j in jobs], seed=25, stream_ids=[0, 1])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 100)
        got = check_sampler(s, jobs[0].ps6, model, 2)
        assert list(got[0].names) == list(el.U_NAMES) + ["m21_2", "m3x_2"]
    finally:
        s.close()
        for j in jobs:
            j.close()


def test_c5_shaped_chains_in_element_space(model):
    pts = scan.sens_grid()[:3]
    jobs = [scan._SensPoint(p, g, nwalkers=512, device=0) for g, p in enumerate(pts)]
    s = mcmc_utils.DeviceEnsembleSampler(512, 12, [j.f for j in jobs], seed=25, stream_ids=[0, 1, 2])
    s.on_nonunitary = "-inf"
    try:
        s.run_mcmc(np.stack([j.p0 for j in jobs]), 200)
        ps = scan._SensPoint.descriptor(pts[0])[0]
        got = check_sampler(s, ps, model, 3)
        assert len(got[0].names) == 17 and len(got[0].pairs) == 136
    finally:
        s.close()
        for j in jobs:
            j.close()


# ---- the command lines' files --------------------------------------------------------------------------------------------------------
def check_scan_files(model, tmp_path, config, npoints, chain_cols, paramset_of):
    """`scan --marginals --elements`: marginals_elements_<point>.npz beside marginals_<point>.npz and the chain file, in
    as_arrays()' layout, equal to the two-step path on the saved chain (element_rows of the sample columns, chain_marginals)"""
    import os
    d = str(tmp_path / config)
    scan.main(["--config", config, "--points", str(npoints), "--nwalkers", "128", "--burnin", "10", "--nsteps", "40", "--datadir", d,
               "--marginals", "--elements"])
    chains = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert len(chains) == npoints
    assert sorted(os.listdir(d)) == sorted(chains + ["marginals_%s.npz" % f[:-4] for f in chains] + ["marginals_elements_%s.npz" % f[:-4] for f in chains])
    for g, f in enumerate(chains):
        z = np.load(os.path.join(d, "marginals_elements_%s.npz" % f[:-4]))
        rows = np.load(os.path.join(d, f))[:, chain_cols]
        ps = paramset_of(f)
        plan, names, ranges = el.element_plan(ps)
        assert list(z["names"]) == list(names) and [tuple(r) for r in z["ranges"]] == [tuple(r) for r in ranges]
        want = mg.chain_marginals(el.element_rows(rows, plan, model=model), ranges, model=model, names=names).as_arrays()
        assert set(want) == set(z.files)
        for k in want:
            assert np.array_equal(want[k], z[k], equal_nan=want[k].dtype.kind == "f"), (f, k)
    return chains


def test_scan_c4_writes_element_marginals(model, tmp_path, capsys):
    ps6 = Cf.ParamSet(list(Cf.texture_paramset(6))[:6])
    check_scan_files(model, tmp_path, "C4", 3, slice(3, 9), lambda f: ps6)


def test_scan_c5_writes_element_marginals_over_each_points_own_ranges(model, tmp_path, capsys):
    """the first points of the C5 grid are dimension 3; with 130 points the dimension-6 ones follow (a stacked sampler holds both):
    every file's logLam range is its own dimension's"""
    def ps_of(f):
        return Cf.fr_paramsets(int(f.split("_DIM")[1][0]), (0.5, 0.0))[1]
    chains = check_scan_files(model, tmp_path, "C5", 130, slice(0, 12), ps_of)
    assert {f.split("_DIM")[1][0] for f in chains} == {"3", "6"}


def test_mcmc_plot_elements_saves_the_element_marginals(model, tmp_path, capsys):
    """mcmc.mcmc(..., plot_elements=True): <outfile>_elements.npz equals the two-step path on the samples it returns"""
    from golemflavor_amd import llh as llh_utils
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, ps = Cf.notebook_paramsets(ang)
    f = llh_utils.notebook_ln_prob(asimov, ps)
    outfile = str(tmp_path / "out" / "chain_DIM6")
    np.random.seed(26)
    p0 = mcmc_utils.flat_seed(ps, nwalkers=64)
    try:
        samples = mcmc_utils.mcmc(p0=p0, ln_prob=f, ndim=6, nwalkers=64, burnin=50, nsteps=120, seed=9, plot_elements=True, llh_paramset=ps,
                                  outfile=outfile)
    finally:
        f.close()
    z = np.load(mcmc_utils.element_marginals_file(outfile))
    plan, names, ranges = el.element_plan(ps)
    steps = samples.reshape(64, 120, 6).transpose(1, 0, 2).reshape(-1, 6)             # emcee's walker-major -> the device's order
    want = mg.chain_marginals(el.element_rows(steps, plan, model=model), ranges, model=model, names=names).as_arrays()
    assert set(want) == set(z.files) and list(z["names"]) == list(el.U_NAMES + el.FR_NAMES)
    for k in want:
        assert np.array_equal(want[k], z[k], equal_nan=want[k].dtype.kind == "f"), k
