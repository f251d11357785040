"""Host side of the tempered sampler of the energy-resolved and the tabulated likelihood: the two entry points in the
header, the binding and the library's exports, their null-handle refusals, the one keyword conflict of
`tempering.evidence_scan_tempered`, and the command line, which stays as it was.  No GPU."""
import ctypes as C
import os
import re

import pytest

from golemflavor_amd import _lib, tempering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("gf_sampler_create_tempered_binned", "gf_sampler_create_tempered_table")
PARAMS = ["gf_model* const* models", "int nmodels", "int ngroups", "int ntemps", "const double* betas", "int nwalkers", "uint64_t seed",
          "double a", "int swap_every", "gf_sampler** out"]


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "golemflavor_hip.h")).read()
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    L = _lib.lib()
    assert L.gf_abi_version() == 5

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, hdr, re.M)
        assert m, "%s is not declared" % name
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    assert params("gf_sampler_create_tempered") == PARAMS
    for name in NEW_SYMBOLS:
        assert params(name) == PARAMS, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert res is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == args
        assert args == _lib.SIGNATURES["gf_sampler_create_tempered"][1] and len(args) == len(PARAMS)
    # additive: the descriptor is the one ABI 5 has had
    assert L.gf_sizeof_model_desc() == C.sizeof(_lib.GfModelDesc) == 1480


def test_entry_points_refuse_null_handles():
    L = _lib.lib()
    betas = (C.c_double * 2)(1.0, 0.0)
    for name in NEW_SYMBOLS:
        fn = getattr(L, name)
        out = C.c_void_p(1)
        assert fn(None, 1, 1, 2, betas, 24, 0, 2.0, 0, C.byref(out)) == _lib.GF_ERR_INVALID_ARG
        handles = (C.c_void_p * 1)(None)
        assert fn(handles, 1, 1, 2, None, 24, 0, 2.0, 0, C.byref(out)) == _lib.GF_ERR_INVALID_ARG
        assert fn(handles, 1, 1, 2, betas, 24, 0, 2.0, 0, None) == _lib.GF_ERR_INVALID_ARG
        # a null model behind a good ladder: refused, and the handle handed back is null
        assert fn(handles, 1, 1, 2, betas, 24, 0, 2.0, 0, C.byref(out)) == _lib.GF_ERR_INVALID_ARG and not out.value


def test_evidence_scan_takes_one_likelihood():
    """both keywords: refused before anything is built -- there is no parameter set, no argument and no device behind this call"""
    with pytest.raises(ValueError, match="two likelihoods"):
        tempering.evidence_scan_tempered(None, None, None, [0.0], binned=object(), table=object())


@pytest.mark.parametrize("extra", [["--energy-resolved"], ["--likelihood-table", "t.npy"], ["--binned-measurement", "m.npy"]])
def test_the_command_line_still_refuses_the_two_likelihoods(extra, capsys):
    """the library and `evidence_scan_tempered` take the two likelihoods, sens.py's parser keeps its refusal"""
    from golemflavor_amd import sens
    with pytest.raises(SystemExit) as e:
        sens.parse_args(["--evidence-method", "stepping-stone"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "flux-averaged likelihood only" in err and "--energy-resolved or --likelihood-table" in err
