"""Host side of the ensemble sampler under a tabulated flavour-plane likelihood ("Ensemble sampler"): scan.py's option and
file names, the header's declaration against the binding, and `DeviceEnsembleSampler(tabulated=True)`'s refusals.  No GPU."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from golemflavor_amd import _lib, scan
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.enums import Texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def table_file(tmp_path):
    """a loadable table of side 2"""
    path = str(tmp_path / "table.npy")
    np.save(path, np.linspace(-3.0, 0.0, 6))
    return path


@pytest.mark.parametrize("extra, says", [
    (["--config", "C4"], "--config C5"),
    (["--config", "C5", "--energy-resolved"], "does not combine with --energy-resolved"),
    (["--config", "C5", "--binned-measurement", "nowhere.npy"], "does not combine with --energy-resolved"),
    (["--config", "C5", "--energy-resolved", "--binned-smearing", "0.02"], "does not combine with --energy-resolved"),
    (["--config", "C5", "--datadir", "d", "--reweight-injected", "1", "1", "1"], "--reweight-injected does not combine with --likelihood-table"),
])
def test_scan_argument_errors(extra, says, table_file, capsys):
    with pytest.raises(SystemExit) as e:
        scan.main(extra + ["--likelihood-table", table_file])
    assert e.value.code == 2
    assert says in capsys.readouterr().err


def test_scan_refuses_a_file_that_does_not_load(tmp_path, capsys):
    five = str(tmp_path / "five.npy")
    np.save(five, np.zeros(5))                                    # five values are the nodes of no lattice
    nan = str(tmp_path / "nan.npy")
    np.save(nan, np.array([0.0, np.nan, 0.0]))
    for path, says in ((str(tmp_path / "nowhere.npy"), "nowhere.npy"), (five, "5 values"), (nan, "NaN")):
        with pytest.raises(SystemExit) as e:
            scan.main(["--config", "C5", "--likelihood-table", path])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--likelihood-table" in err and says in err, err


def test_ltab_file_names():
    """`_ltab` behind the point's stem, where `_ebins` goes: the chain file and, through `name_of`, every writer's file; without the
    option the names are what they were."""
    pt = (6, Texture.OUT, (0.0, 1.0, 0.0), -47.0)
    plain = scan.point_filename("C5", pt, argparse.Namespace())
    off = scan.point_filename("C5", pt, argparse.Namespace(likelihood_table=None, energy_resolved=False))
    on = scan.point_filename("C5", pt, argparse.Namespace(likelihood_table="some.npy", energy_resolved=False))
    assert plain == off == "fr_DIM6_sfr_0_1_0_OUT_logLam-47.000"
    assert on == plain + "_ltab"
    assert scan.point_filename("C5", pt, argparse.Namespace(energy_resolved=True)) == plain + "_ebins"
    w = scan.MarginalWriter("dd", lambda g: on)
    assert w.file("marginals", 0) == os.path.join("dd", "marginals_%s_ltab.npz" % plain)
    # every writer names its files through PointWriter.file and the scan's name_of
    for cls in (scan.RegionWriter, scan.SpectrumWriter, scan.DiagnosticsWriter, scan.IntervalWriter, scan.BinnedReweightWriter):
        assert cls.file is scan.PointWriter.file
        assert scan.PointWriter("dd", lambda g: on).file(cls.key, 0) == os.path.join("dd", "%s_%s_ltab.npz" % (cls.key, plain))
    # C4 has no such names: its option is an argument error
    c4 = scan.point_filename("C4", (-47.0, (0.0, 1.0, 0.0)), argparse.Namespace(dimension=6, texture="OET", likelihood_table="some.npy"))
    assert "_ltab" not in c4


def test_header_declares_what_the_binding_binds():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    m = re.search(r"^int\s+gf_sampler_create_table\s*\(([^)]*)\)\s*;", hdr, re.M)
    assert m, "gf_sampler_create_table is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["gf_model* const* models", "int nmodels", "int nchains", "int nwalkers", "uint64_t seed", "double a", "gf_sampler** out"]
    by_type = {"gf_model* const*": C.POINTER(C.c_void_p), "int": C.c_int, "uint64_t": C.c_uint64, "double": C.c_double,
               "gf_sampler**": C.POINTER(C.c_void_p)}
    want = [by_type[p.rsplit(" ", 1)[0]] for p in params]
    res, args = _lib.SIGNATURES["gf_sampler_create_table"]
    assert res is C.c_int and args == want
    fn = _lib.lib().gf_sampler_create_table                       # exported, and bound with these types
    assert fn.restype is C.c_int and list(fn.argtypes) == want
    assert "out of scope" not in hdr[hdr.index("GF_TABLE_MAX_NSIDE") - 3000:hdr.index("GF_TABLE_MAX_NSIDE")]


class _StubModel:
    """what DeviceEnsembleSampler looks at before it touches the library"""
    _h = object()

    def __init__(self, ndim, table_nside=0, binned=None):
        self.ndim, self.table_nside = ndim, table_nside
        if binned is not None:
            self.binned = binned


def test_tabulated_needs_a_table_on_every_posterior(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="posterior 0 carries no tabulated likelihood"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, _StubModel(7), tabulated=True)
    with pytest.raises(ValueError, match="posterior 1 carries no tabulated likelihood"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, [_StubModel(7, table_nside=64), _StubModel(7)], tabulated=True)
    with pytest.raises(ValueError, match="carries no tabulated likelihood"):
        mcmc_utils.mcmc(None, _StubModel(7), 7, 32, 1, 1, device_resident=True, seed=1, tabulated=True)
    with pytest.raises(ValueError, match="tabulated=True and energy_resolved=True"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, _StubModel(7, table_nside=64, binned=object()), tabulated=True, energy_resolved=True)
    # with a table everywhere the next thing it does is ask for the library
    with pytest.raises(AssertionError, match="the library was called"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, _StubModel(7, table_nside=64), tabulated=True)
