"""Host side of the energy-resolved ensemble sampler ("Ensemble sampler"): scan.py's flags and file names, the header's
declaration against the binding, and `DeviceEnsembleSampler(energy_resolved=True)`'s refusal of a posterior without a measurement.
No GPU."""
import argparse
import ctypes as C
import os
import re

import pytest

from golemflavor_amd import _lib, scan
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.enums import Texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv, says", [
    (["--config", "C4", "--energy-resolved"], "--config C5"),
    (["--config", "C4", "--binned-measurement", "nowhere.npy"], "--config C5"),
    (["--config", "C5", "--energy-resolved", "--datadir", "d", "--reweight-injected", "1", "1", "1"], "--reweight-injected does not combine"),
    (["--config", "C5", "--energy-resolved", "--binned-smearing", "0.02", "0.03", "0.04"], "one per energy bin (20)"),
    (["--config", "C5", "--energy-resolved", "--binned-smearing", "-0.02"], "one positive value"),
    (["--config", "C5", "--binned-smearing", "0.02"], "needs --energy-resolved"),
])
def test_scan_argument_errors(argv, says, capsys):
    with pytest.raises(SystemExit) as e:
        scan.main(argv)
    assert e.value.code == 2
    assert says in capsys.readouterr().err


def test_ebins_file_names():
    """`_ebins` behind the point's stem: the chain file and, through `name_of`, every writer's file; without the flag the names are
    what they were."""
    pt = (6, Texture.OUT, (0.0, 1.0, 0.0), -47.0)
    plain = scan.point_filename("C5", pt, argparse.Namespace())
    off = scan.point_filename("C5", pt, argparse.Namespace(energy_resolved=False))
    on = scan.point_filename("C5", pt, argparse.Namespace(energy_resolved=True))
    assert plain == off == "fr_DIM6_sfr_0_1_0_OUT_logLam-47.000"
    assert on == plain + "_ebins"
    w = scan.MarginalWriter("dd", lambda g: on)
    assert w.file("marginals", 0) == os.path.join("dd", "marginals_%s_ebins.npz" % plain)
    assert scan.DiagnosticsWriter("dd", lambda g: on).file("diagnostics", 0).endswith("_ebins.npz")
    # C4 has no such names: its flag is an argument error
    c4 = scan.point_filename("C4", (-47.0, (0.0, 1.0, 0.0)), argparse.Namespace(dimension=6, texture="OET", energy_resolved=True))
    assert "_ebins" not in c4


def test_header_declares_what_the_binding_binds():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    m = re.search(r"^int\s+gf_sampler_create_binned\s*\(([^)]*)\)\s*;", hdr, re.M)
    assert m, "gf_sampler_create_binned is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["gf_model* const* models", "int nmodels", "int nchains", "int nwalkers", "uint64_t seed", "double a", "gf_sampler** out"]
    by_type = {"gf_model* const*": C.POINTER(C.c_void_p), "int": C.c_int, "uint64_t": C.c_uint64, "double": C.c_double,
               "gf_sampler**": C.POINTER(C.c_void_p)}
    want = [by_type[p.rsplit(" ", 1)[0]] for p in params]
    res, args = _lib.SIGNATURES["gf_sampler_create_binned"]
    assert res is C.c_int and args == want
    fn = _lib.lib().gf_sampler_create_binned                      # exported, and bound with these types
    assert fn.restype is C.c_int and list(fn.argtypes) == want


class _StubModel:
    """what DeviceEnsembleSampler looks at before it touches the library"""
    _h = object()

    def __init__(self, ndim, binned=None):
        self.ndim = ndim
        if binned is not None:
            self.binned = binned


def test_energy_resolved_needs_a_measurement_on_every_posterior(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="posterior 0 carries no binned measurement"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, _StubModel(7), energy_resolved=True)
    with pytest.raises(ValueError, match="posterior 1 carries no binned measurement"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, [_StubModel(7, binned=object()), _StubModel(7)], energy_resolved=True)
    with pytest.raises(ValueError, match="carries no binned measurement"):
        mcmc_utils.mcmc(None, _StubModel(7), 7, 32, 1, 1, device_resident=True, seed=1, energy_resolved=True)
    # with a measurement everywhere the next thing it does is ask for the library
    with pytest.raises(AssertionError, match="the library was called"):
        mcmc_utils.DeviceEnsembleSampler(32, 7, _StubModel(7, binned=object()), energy_resolved=True)
