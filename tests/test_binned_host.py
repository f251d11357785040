"""Host: the energy-resolved Gaussian likelihood's pieces that need no GPU -- the ABI stays put, the new prototypes
are declared on both sides, `BinnedMeasurement` validates, the equal-information rule holds, sens names its files, and the tests'
numpy restatement is the reference's multi_gaussian bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from binned_ref import binned_lnl_host, binned_terms_host, multi_gaussian_host
from golemflavor_amd import _lib, llh, sens
from golemflavor_amd import configs as Cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "golemflavor_hip.h")
NEW = ("gf_model_set_binned_measurement", "gf_model_is_binned")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_abi_version_and_descriptor_size_are_unchanged():
    assert re.search(r"^#define\s+GF_ABI_VERSION\s+5\s*$", header_text(), re.M)
    assert _lib.GF_ABI_VERSION == 5
    # gf_model_desc as it was before the binned measurement: 14 + 2 + 16 int32, then 5 x 16 + 4 + 2 + 3 + 1 + 4 + 1 + 3 + 3 + 65 doubles
    assert C.sizeof(_lib.GfModelDesc) == 4 * (6 + 4 + 2 + 2 + 1 + 4 + 1 + 2 + 16) + 8 * (5 * 16 + 4 + 2 + 3 + 1 + 4 + 1 + 3 + 1 + 1 + 1 + 65)
    assert C.sizeof(_lib.GfModelDesc) == 1480
    assert _lib.lib().gf_sizeof_model_desc() == 1480                 # the library agrees (no GPU needed to load it)


def test_new_prototypes_in_header_and_binding():
    h = header_text()
    assert re.search(r"int\s+gf_model_set_binned_measurement\(gf_model\*\s*m,\s*int\s+nbins,\s*const\s+double\*\s*fr_bins,\s*const\s+double\*\s*sigma\);", h)
    assert re.search(r"int\s+gf_model_is_binned\(const\s+gf_model\*\s*m\);", h)
    for name in NEW:
        assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["gf_model_set_binned_measurement"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, _lib._dp, _lib._dp]
    assert _lib.SIGNATURES["gf_model_is_binned"] == (C.c_int, [C.c_void_p])


def test_binned_measurement_validation():
    edges = Cf.default_bin_edges()
    K = len(edges) - 1
    f = np.full((K, 3), 1 / 3)
    m = llh.BinnedMeasurement(f, 0.02, binning=edges)
    assert m.nbins == K and m.sigma.shape == (K,) and np.array_equal(m.sigma, llh.equal_information_smearing(0.02, edges))
    explicit = llh.BinnedMeasurement(f, np.linspace(0.01, 0.2, K))
    assert np.array_equal(explicit.sigma, np.linspace(0.01, 0.2, K))
    assert np.array_equal(llh.BinnedMeasurement(f, np.linspace(0.01, 0.2, K), binning=edges).sigma, explicit.sigma)   # explicit widths win
    c = llh.BinnedMeasurement.constant((0.2, 0.3, 0.5), 0.02, edges)
    assert c.fr_bins.shape == (K, 3) and np.array_equal(c.fr_bins[7], [0.2, 0.3, 0.5])
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f[:-1], 0.02, binning=edges)                       # wrong K for the binning
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f.reshape(-1), 0.02, binning=edges)                # not (K, 3)
    bad = f.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(bad, 0.02, binning=edges)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(bad, 0.02, binning=edges)
    for s in (0.0, -0.02, np.nan):
        with pytest.raises(ValueError):
            llh.BinnedMeasurement(f, s, binning=edges)
    sg = np.full(K, 0.02)
    sg[5] = 0.0
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f, sg)
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f, np.full(K - 1, 0.02), binning=edges)            # wrong number of smearings
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f, [0.02, 0.03], binning=edges)
    with pytest.raises(ValueError):
        llh.BinnedMeasurement(f, 0.02)                                           # one smearing for K bins needs the binning


@pytest.mark.parametrize("edges", [Cf.default_bin_edges(), np.array([1e4, 3e4, 2e5, 1e7])], ids=["default", "three"])
def test_equal_information_rule(edges):
    w = np.abs(np.diff(edges)) / (edges[-1] - edges[0])
    for sm in (0.02, 0.011, 0.3):
        s = llh.equal_information_smearing(sm, edges)
        assert s.shape == w.shape and np.all(s >= sm)
        tot = float(np.sum(w * w * s * s))
        assert abs(tot - sm * sm) <= 8 * np.spacing(sm * sm), (tot, sm * sm)
    with pytest.raises(ValueError):
        llh.equal_information_smearing(0.0, edges)
    with pytest.raises(ValueError):
        llh.equal_information_smearing(0.02, edges[:1])


def test_sens_arguments_and_file_names(tmp_path):
    plain = sens.parse_args(["--datadir", "/d"])
    assert not plain.energy_resolved and plain.binned_measurement is None and plain.binned_smearing is None
    stat0, llh0 = sens.output_paths(plain)
    a = sens.parse_args(["--datadir", "/d", "--energy-resolved"])
    assert a.energy_resolved
    stat, mx = sens.output_paths(a)
    assert stat == stat0 + "_ebins" and mx == llh0 + "_ebins"
    assert sens.posterior_path(a, -30.0) == sens.posterior_path(plain, -30.0).replace("_scale_", "_ebins_scale_")
    assert sens.spectrum_path(a, -30.0) == sens.spectrum_path(plain, -30.0).replace("_scale_", "_ebins_scale_")
    seg = sens.parse_args(["--datadir", "/d", "--energy-resolved", "--eval-segment", "2", "--segments", "5"])
    assert "_ebins_scale_" in sens.output_paths(seg)[0]
    # the measurement --energy-resolved builds: the injected composition in every bin, widths by the equal-information rule
    asimov, _ = Cf.sens_paramsets(a.dimension, a.injected_ratio, data=a.data)
    m = sens.binned_measurement(a, asimov)
    assert m.nbins == 20 and np.allclose(m.fr_bins, 1 / 3, atol=1e-15)
    assert np.array_equal(m.sigma, llh.equal_information_smearing(0.02, a.binning))
    assert sens.binned_measurement(plain, asimov) is None
    one = sens.parse_args(["--datadir", "/d", "--energy-resolved", "--binned-smearing", "0.05"])
    assert np.array_equal(sens.binned_measurement(one, asimov).sigma, llh.equal_information_smearing(0.05, one.binning))
    widths = [str(0.01 * (k + 1)) for k in range(20)]
    ex = sens.parse_args(["--datadir", "/d", "--energy-resolved", "--binned-smearing"] + widths)
    assert np.array_equal(sens.binned_measurement(ex, asimov).sigma, np.array([float(x) for x in widths]))
    f = tmp_path / "meas.npy"
    arr = np.random.default_rng(1).dirichlet((2, 2, 2), size=20)
    np.save(f, arr)
    fm = sens.parse_args(["--datadir", "/d", "--binned-measurement", str(f)])
    assert fm.energy_resolved and sens.output_paths(fm)[0].endswith("_ebins")
    assert np.array_equal(sens.binned_measurement(fm, asimov).fr_bins, arr)
    for bad in (["--binned-smearing", "0.02"], ["--energy-resolved", "--binned-smearing", "0.02", "0.03"],
                ["--energy-resolved", "--binned-smearing", "-1"]):
        with pytest.raises(SystemExit):
            sens.parse_args(["--datadir", "/d"] + bad)


def test_host_restatement_is_the_oracles_multi_gaussian(oracle):
    rng = np.random.default_rng(23)
    K = 20
    edges = Cf.default_bin_edges()
    meas = llh.BinnedMeasurement(rng.dirichlet((3, 3, 3), size=K), 0.02, binning=edges)
    fr = rng.dirichlet((1, 1, 1), size=(40, K))
    terms = binned_terms_host(fr, meas)
    for i in range(fr.shape[0]):
        for k in range(K):
            ref = oracle.multi_gaussian(fr[i, k], meas.fr_bins[k], meas.sigma[k], 0.0)
            assert terms[i, k] == ref or (np.isnan(terms[i, k]) and np.isnan(ref)), (i, k, terms[i, k], ref)
    # across the underflow wall: widths small enough for the subnormal band and for -inf
    band = inf = 0
    for sg in np.linspace(0.012, 0.03, 37):
        for i in range(40):
            got = multi_gaussian_host(fr[i, 0], (0.9, 0.05, 0.05), sg)
            ref = oracle.multi_gaussian(fr[i, 0], (0.9, 0.05, 0.05), sg, 0.0)
            assert got == ref, (sg, i, got, ref)
            band += int(np.isfinite(ref) and ref < -708.4)
            inf += int(ref == -np.inf)
    assert band >= 3 and inf >= 3, (band, inf)
    # the sum: ascending k from 0.0, then the offset
    lnl, t = binned_lnl_host(fr[:5], meas, return_terms=True)
    for i in range(5):
        acc = 0.0
        for k in range(K):
            acc = acc + float(t[i, k])
        assert lnl[i] == acc + (-320.0)
