"""CPU: the energy-resolved composition without a device -- the golden of tests/golden/make_golden_spectrum.py against
the oracle per bin and against the reference's own flux average, the Python side of `golemflavor_amd.spectrum`, and the declarations
of the new C entry points."""
import os
import re

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import spectrum as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = 1e-9
TEX_ANGLES = {1: (0.5, 1.0, Z, Z), 2: (Z, 0.25, Z, Z), 3: (Z, 1.0, 0.5, Z)}
NEW_SYMBOLS = ("gf_model_nbins", "gf_propagate_bins_device", "gf_propagate_bins", "gf_sampler_spectrum", "gf_nested_spectrum")


@pytest.fixture(scope="module")
def gs():
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_spectrum.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_what_the_generator_promises(gs):
    assert gs["configs"].tolist() == [[3, 2], [6, 1], [6, 3], [4, 2]]
    assert gs["theta"].shape == (4, 12, 7) and gs["fr_ref"].shape == (4, 12, 20, 3) and gs["abs2_ref"].shape == (4, 12, 20, 3, 3)
    assert (gs["ok"] == 0).sum() >= 20 and (gs["ok"] == 1).sum() >= 400
    assert np.allclose(gs["binning"], np.logspace(np.log10(6e4), np.log10(1e7), 21), rtol=0, atol=0)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_spectrum.npz")) < 200 * 1024
    # every composition sums to one, the reference's and the exact one
    assert np.abs(gs["fr_ref"].sum(axis=-1) - 1)[gs["ok"] == 1].max() < 1e-7 and np.abs(gs["fr_exact"].sum(axis=-1) - 1).max() < 1e-15


def test_oracle_per_bin_agrees_with_the_golden_on_passing_pairs(gs, oracle):
    """oracle.params_to_BSMu + oracle.u_to_fr at every bin centre, under G7's bar (test_oracle_golden.py): both are 80-bit
    evaluations of an ill-conditioned closed form and agree with each other to the noise the reference itself shows against the
    exact value.  G7 also asks for the same verdict; its rows use the NuFIT matrix both sides hold as a constant.  Here the mixing
    angles are a row's own, the oracle's angles_to_u and numpy's differ in the last bits of the 80-bit matrix, and at the very top of
    a scale range (logLam = -30 for dimension 6, rows on which the reference raises in other bins anyway) the residual is rounding
    noise of order 1e-7 that those bits move: two of the 960 pairs pass in the reference and fail in the oracle.  Such pairs may
    only occur in rows whose flux average raised, and at most 1 % of the pairs; they have no oracle value to compare."""
    centres = np.sqrt(gs["binning"][:-1] * gs["binning"][1:])
    npairs, worst_fr, other_verdict = 0, 0.0, 0
    for ci, (dim, texv) in enumerate(gs["configs"]):
        for ri, th in enumerate(gs["theta"][ci]):
            for k, e in enumerate(centres):
                if not gs["ok"][ci, ri, k]:
                    continue
                u, uok = oracle.params_to_BSMu(TEX_ANGLES[int(texv)], th[6], int(dim), e, mass_eigenvalues=th[4:6], sm_angles=th[:4])
                if not uok:
                    assert gs["flux_status"][ci, ri] == 2, (ci, ri, k)
                    other_verdict += 1
                    continue
                exact = gs["abs2_ref"][ci, ri, k] - gs["abs2_diff"][ci, ri, k].astype(np.float64)
                ref_noise = np.abs(gs["abs2_diff"][ci, ri, k]).max()
                assert np.abs(np.abs(u) ** 2 - exact).max() <= max(1e-12, 10 * ref_noise), (ci, ri, k)
                f = oracle.u_to_fr(gs["source"], u)
                # f = P P^T s is a contraction of |U|^2 with weights that sum to one, twice: at most twice its error
                assert np.abs(f - gs["fr_exact"][ci, ri, k]).max() <= 2 * max(1e-12, 10 * ref_noise), (ci, ri, k)
                worst_fr = max(worst_fr, np.abs(f - gs["fr_ref"][ci, ri, k]).max())
                npairs += 1
    assert npairs + other_verdict == int((gs["ok"] == 1).sum()) and npairs >= 400 and other_verdict <= 9
    print("oracle vs reference per bin: %d pairs, worst composition difference %.3e" % (npairs, worst_fr))


def test_recombined_golden_bins_equal_the_references_flux_average(gs):
    """fr.py:454-457 on the stored per-bin values equals the reference's own flux_averaged_BSMu to 1e-15 relative: both are
    long-double sums of the same 20 terms (the stored terms are rounded to fp64, 1.1e-16 each)."""
    widths = np.abs(np.diff(gs["binning"])).astype(np.longdouble)
    span = np.longdouble(gs["binning"][-1]) - np.longdouble(gs["binning"][0])
    nrows = 0
    for ci in range(4):
        for ri in range(12):
            if gs["flux_status"][ci, ri] != 0:
                assert np.isnan(gs["flux_avg"][ci, ri]).all() and (gs["ok"][ci, ri] == 0).any()
                continue
            assert (gs["ok"][ci, ri] == 1).all()
            integrated = np.sum(gs["fr_ref"][ci, ri].astype(np.longdouble).T * widths, axis=1)
            averaged = (np.longdouble(1) / span) * integrated
            f = np.asarray(averaged / np.sum(averaged), dtype=np.float64)
            ref = gs["flux_avg"][ci, ri]
            assert np.abs(f - ref).max() <= 1e-15 * np.abs(ref).max(), (ci, ri)
            nrows += 1
    assert nrows >= 40


def test_prepare_validates_its_arguments():
    edges = np.logspace(4, 7, 21)
    p = sp.prepare(edges)
    assert p["bins"] == 50 and p["q"].tolist() == [5., 16., 50., 84., 95.] and len(p["energies"]) == 20
    assert np.array_equal(p["energies"], np.sqrt(edges[:-1] * edges[1:])) and np.array_equal(p["widths"], np.abs(np.diff(edges)))
    assert np.array_equal(p["hist_edges"], np.linspace(0., 1., 51))
    for bad in (dict(edges=[1.]), dict(edges=np.ones((2, 2))), dict(edges=[1., 1.]), dict(edges=[1., 3., 2.]), dict(edges=[-1., 2.]),
                dict(edges=[1., np.nan]), dict(edges=np.arange(1., 67.)), dict(edges=edges, bins=0), dict(edges=edges, bins=1025),
                dict(edges=edges, percentiles=(-1.,)), dict(edges=edges, percentiles=(101.,)), dict(edges=edges, percentiles=[[5.]]),
                dict(edges=edges, percentiles=tuple(range(9)))):
        with pytest.raises(ValueError):
            sp.prepare(**bad)
    assert len(sp.prepare(np.arange(1., 66.))["energies"]) == 64                 # GF_MAX_BINS
    assert len(sp.prepare(edges, percentiles=())["q"]) == 0


def _synthetic_result(seed=3):
    rng = np.random.default_rng(seed)
    edges = np.logspace(np.log10(6e4), np.log10(1e7), 6)
    f = rng.dirichlet([2., 3., 4.], size=(500, 5))
    f[::50] = np.nan
    return sp.rows_spectrum_host(f, edges, percentiles=(16., 50., 84.), bins=20), f, edges


def test_result_round_trips_and_flux_average_follows_the_reference(tmp_path):
    r, f, edges = _synthetic_result()
    assert r.nvalid.tolist() == [490] * 5 and r.counts.sum(axis=-1).tolist() == [[490] * 3] * 5
    good = f[~np.isnan(f).any(axis=(1, 2))]
    assert np.array_equal(r.percentiles[2, 1], np.percentile(good[:, 2, 1], (16., 50., 84.)))
    path = str(tmp_path / "spectrum.npz")
    r.save(path)
    back = sp.SpectrumResult.load(path)
    for k in sp.SpectrumResult.ARRAYS:
        assert np.array_equal(getattr(r, k), getattr(back, k), equal_nan=True), k
    with np.load(path) as z:
        assert set(z.files) == set(sp.SpectrumResult.ARRAYS) | {"names"} and z["names"].tolist() == list(sp.FLAVOURS)
    # fr.py:454-457, written out
    measured_flux = r.mean.T
    integrated = np.sum(measured_flux * np.abs(np.diff(edges)), axis=1)
    averaged = (1. / (edges[-1] - edges[0])) * integrated
    assert np.array_equal(r.flux_average(), averaged / np.sum(averaged))
    assert np.array_equal(back.flux_average(), r.flux_average()) and abs(r.flux_average().sum() - 1) < 1e-15


def test_header_declares_the_entry_points_and_the_binding_has_them():
    with open(os.path.join(ROOT, "include", "golemflavor_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", header) and _lib.GF_ABI_VERSION == 5
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct gf_spectrum_spec" in header and "typedef struct gf_spectrum_out" in header
    assert [n for n, _ in _lib.GfSpectrumSpec._fields_] == ["nbins1", "nq", "q"]
    assert [n for n, _ in _lib.GfSpectrumOut._fields_] == ["nvalid", "mean", "cov", "ostat", "orank", "counts"]
