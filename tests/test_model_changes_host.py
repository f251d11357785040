"""Host side of "models that change under a live handle" (tests/test_gpu_model_changes.py is the GPU side): the internal
count of likelihoods set on a model is exported and bound, stays out of the public header, and the ABI version does not move.  No GPU."""
import os
import re

from golemflavor_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "golemflavor_amd", "csrc")


def read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def test_the_count_is_internal_and_bound():
    hdr = read(ROOT, "include", "golemflavor_hip.h")
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", hdr) and _lib.GF_ABI_VERSION == 5
    assert "gf_model_likelihood_sets" not in hdr and "gf_model_likelihood_sets" not in _lib.SIGNATURES
    assert re.search(r"^uint64_t\s+gf_model_likelihood_sets\(const\s+gf_model\*\s*m\);", read(CSRC, "gf_internal.h"), re.M)
    assert hasattr(_lib.lib(), "gf_model_likelihood_sets")               # exported
    assert _lib.likelihood_sets(None) == 0                               # ... and bound: a NULL model has none

