"""The element-space transform (csrc/gf_elements.hpp) built for the host and held to the CPU oracle, `elements.element_plan` on the
package's paramsets, the header / binding of the new entry points and the command lines' handling of the new flags.  No device.

The input (tests/elements_harness.py) is seeded: edge rows -- each of s12^2, c13^4, s23^2 at 0, 1, 2^-k and 1 - 2^-k, k = 1 .. 52,
delta at the multiples of pi/2 and random, the other columns random, at their own corners, and all at an edge at once -- then 2^22
rows uniform over the box.  TOL = 4 x the maximum absolute error measured over it (2.22e-15 at (1 - 2^-34, 1 - 2^-31, 1 - 2^-18, 0),
entry U_mu2; 3.9e-16 over the uniform rows): the 80-bit asin / cos route of the reference is the ill-conditioned side there
(cos(asin(s)) as s -> 1), not the square roots of this package.

The float32 column: an absolute tolerance of 8.9e-15 is below a float32 step only down to ~7.5e-8 (= TOL 2^23), and where an entry
vanishes the reference returns its own rounding noise (cos(pi/2 in 80 bits) = 2.7e-20), not 0.  Rows with a modulus below 2^-20
therefore go through the reference's route in emulated 80-bit arithmetic (csrc/gf_elements_exact.hpp).  Measured on the host
build: 15 442 of 37 855 080 entries are near a float32 rounding boundary (4.1e-4, under the cap), none of the others differs, 57 of
the near ones differ, all by one step."""
import argparse
import os
import re

import numpy as np
import pytest

import elements_harness as H
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import elements as el
from golemflavor_amd.enums import ParamTag
from golemflavor_amd.param import Param, ParamSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U9 = [(el.GF_ELEMENT_U9, [0, 1, 2, 3])]


@pytest.fixture(scope="module")
def host():
    return H.build()


@pytest.fixture(scope="module")
def mixing(host):
    x = H.mixing_input()
    assert len(x) >= 4 << 20
    return x, H.oracle_absu(x), H.host_rows(host, el.make_plan(U9, round32=False), x), H.host_rows(host, el.make_plan(U9, round32=True), x)


# ---- 1. the host build against the oracle ------------------------------------------------------------------------------------------
def test_moduli_against_the_oracle(mixing):
    from oracle import oracle as O
    x, ref, got, _ = mixing
    worst, row = H.check_moduli(got, ref, "host")
    # the tolerance is four times a measurement: the constant must be this input's measurement and inside the conditioning bound
    assert H.TOL == 4 * H.MEASURED_MAX and H.MEASURED_MAX <= 1e-14 and H.MEASURED_MAX / 2 <= worst <= H.MEASURED_MAX
    print("worst row", [v.hex() for v in x[row]])
    for i in (0, row, len(x) - 1):                            # the long-double moduli are those of the complex oracle.angles_to_u
        assert np.abs(np.abs(O.angles_to_u(x[i])).ravel() - ref[i].astype(np.float64)).max() <= 2.0 ** -52


def test_source_composition_against_the_oracle(host):
    x = H.source_input()
    assert len(x) >= 4 << 20
    got = H.host_rows(host, el.make_plan([(el.GF_ELEMENT_FR3, [0, 1])]), x)
    err = np.abs(got - H.oracle_fr(x))
    print("host fractions: max abs err %.3e at row %d" % (err.max(), int(np.argmax(err.max(axis=1)))))
    assert err.max() <= H.TOL
    assert got.min() >= 0.0 and np.abs(got.sum(axis=1) - 1).max() <= H.TOL


# ---- 2. the float32 column -----------------------------------------------------------------------------------------------------------
def test_float32_column_exact_away_from_boundaries(mixing):
    x, ref, _, got32 = mixing
    near, steps = H.float32_steps(got32, ref, "host")
    assert near.mean() <= H.F32_EXCLUDED_CAP
    assert not steps[~near].any()
    big = ref >= H.TOL * 2.0 ** 23                            # float32's step there is at least TOL
    assert steps[big].max() <= 1


def test_float32_column_within_one_step_near_boundaries(mixing):
    """on the entries the first assertion leaves out: one float32 step at most"""
    x, ref, _, got32 = mixing
    near, steps = H.float32_steps(got32, ref, "host")
    assert steps[near].max(initial=0) <= 1


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------
def test_rows_and_columns_of_the_squared_moduli_sum_to_one(mixing):
    P = mixing[2].reshape(-1, 3, 3) ** 2
    assert np.abs(P.sum(axis=2) - 1).max() <= H.TOL and np.abs(P.sum(axis=1) - 1).max() <= H.TOL


def test_nan_and_out_of_domain_stay_in_their_group(host):
    plan = el.make_plan([(el.GF_ELEMENT_COPY, [6]), (el.GF_ELEMENT_U9, [0, 1, 2, 3]), (el.GF_ELEMENT_FR3, [4, 5])])
    base = np.array([0.3, 0.9, 0.5, 1.0, 0.4, 0.2, 7.0])
    cols = {"u": slice(1, 10), "fr": slice(10, 13)}
    for c in range(7):
        for bad in (np.nan,) + ((-0.25, 1.5) if c < 3 else ()) + ((1e7,) if c == 3 else ()):
            x = base.copy()
            x[c] = bad
            out = H.host_rows(host, plan, x[None])[0]
            nan = np.isnan(out)
            want = np.zeros(13, bool)
            want[0] = c == 6 and np.isnan(bad)
            want[cols["u"]] = c < 4
            want[cols["fr"]] = c in (4, 5)
            assert np.array_equal(nan, want), (c, bad, out)
    assert not np.isnan(H.host_rows(host, plan, base[None])).any()


# ---- 4. element_plan ---------------------------------------------------------------------------------------------------------------
def plan_groups(plan):
    n = {el.GF_ELEMENT_COPY: 1, el.GF_ELEMENT_U9: 4, el.GF_ELEMENT_FR3: 2}
    return [(plan.group[g].kind, list(plan.group[g].col[:n[plan.group[g].kind]])) for g in range(plan.ngroups)]


UNIT9, UNIT3 = [(0., 1.)] * 9, [(0., 1.)] * 3
NUIS = ["convNorm", "promptNorm", "muonNorm", "astroNorm", "astroDeltaGamma"]
NUIS_RANGES = [(0.1, 10.), (0., 20.), (0., 10.), (0., 20.), (-5., 5.)]
MASS_RANGES = [(6.80E-23, 8.02E-23), (2.399E-21, 2.593E-21)]


@pytest.mark.parametrize("make", [lambda: Cf.fr_paramsets(6, (0.5, 0.0))[1], lambda: Cf.sens_paramsets(3, (1, 1, 1))[1]])
def test_plan_of_the_twelve_column_sets(make):
    ps = make()
    dim = 6 if ps["logLam"].ranges[0] == -56 else 3
    plan, names, ranges = el.element_plan(ps)
    assert plan_groups(plan) == ([(el.GF_ELEMENT_COPY, [c]) for c in range(6, 11)] + [(el.GF_ELEMENT_U9, [0, 1, 2, 3]), (el.GF_ELEMENT_COPY, [11]),
                                 (el.GF_ELEMENT_COPY, [4]), (el.GF_ELEMENT_COPY, [5])])
    assert names == NUIS + list(el.U_NAMES) + ["logLam", "m21_2", "m3x_2"]
    assert ranges == NUIS_RANGES + UNIT9 + [tuple(float(v) for v in Cf.SCALE_BOUNDARIES[dim])] + MASS_RANGES
    assert plan.round32 == 1 and el.element_plan(ps, round32=False)[0].round32 == 0 and len(names) == 17


def test_plan_of_the_texture_set():
    plan, names, ranges = el.element_plan(Cf.texture_paramset(6))
    assert plan_groups(plan) == [(el.GF_ELEMENT_U9, [0, 1, 2, 3]), (el.GF_ELEMENT_COPY, [6]), (el.GF_ELEMENT_COPY, [4]), (el.GF_ELEMENT_COPY, [5])]
    assert names == list(el.U_NAMES) + ["logLam", "m21_2", "m3x_2"] and ranges == UNIT9 + [(-56., -30.)] + MASS_RANGES


def test_plan_of_the_notebook_set():
    plan, names, ranges = el.element_plan(Cf.notebook_paramsets((0.5, 0.0))[1])
    assert plan_groups(plan) == [(el.GF_ELEMENT_U9, [0, 1, 2, 3]), (el.GF_ELEMENT_FR3, [4, 5])]
    assert names == ["U_e1", "U_e2", "U_e3", "U_mu1", "U_mu2", "U_mu3", "U_tau1", "U_tau2", "U_tau3", "phi_e", "phi_mu", "phi_tau"]
    assert ranges == UNIT9 + UNIT3


def test_plan_of_the_texture_none_set_takes_the_mmangles():
    tag = ParamTag.MMANGLES
    mm = [Param(name='np_s_12_2', value=0.5, ranges=[0., 1.], std=0.2, tag=tag), Param(name='np_c_13_4', value=0.5, ranges=[0., 1.], std=0.2, tag=tag),
          Param(name='np_s_23_2', value=0.5, ranges=[0., 1.], std=0.2, tag=tag), Param(name='np_dcp', value=1.0, ranges=[0., 2 * np.pi], std=0.2, tag=tag)]
    base = list(Cf.texture_paramset(6))
    plan, names, ranges = el.element_plan(ParamSet(base[:-1] + mm + base[-1:]))               # G13's eleven columns
    assert plan_groups(plan) == [(el.GF_ELEMENT_U9, [6, 7, 8, 9]), (el.GF_ELEMENT_COPY, [10])] + [(el.GF_ELEMENT_COPY, [c]) for c in range(6)]
    assert names == list(el.U_NAMES) + ["logLam", "s_12_2", "c_13_4", "s_23_2", "dcp", "m21_2", "m3x_2"]
    assert ranges == UNIT9 + [(-56., -30.)] + [(0., 1.)] * 3 + [(0., 2 * np.pi)] + MASS_RANGES


def test_sets_without_a_group_raise():
    with pytest.raises(ValueError):
        el.element_plan(Cf.mcx_paramset()[4:])                 # one source column, no mixing group
    with pytest.raises(ValueError):
        el.element_plan(Cf.tutorial_paramsets((0.5, 0.0))[1])
    assert el.element_groups(Cf.mcx_paramset()) == ((0, 1, 2, 3), None)


def test_host_build_follows_the_plan(host):
    ps = Cf.fr_paramsets(6, (0.5, 0.0))[1]
    plan, names, _ = el.element_plan(ps, round32=False)
    rng = np.random.default_rng(3)
    box = np.array(ps.ranges, dtype=float)
    x = rng.uniform(box[:, 0], box[:, 1], size=(1000, 12))
    out = H.host_rows(host, plan, x)
    assert np.array_equal(out[:, :5], x[:, 6:11]) and np.array_equal(out[:, 14], x[:, 11]) and np.array_equal(out[:, 15:], x[:, 4:6])
    assert np.abs(out[:, 5:14] - H.oracle_absu(x[:, :4]).astype(np.float64)).max() <= H.TOL


# ---- 5. header and ABI -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_matches():
    with open(os.path.join(ROOT, "include", "golemflavor_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define GF_ABI_VERSION 5\b", hdr) and _lib.GF_ABI_VERSION == 5
    for name in ("gf_element_plan_width", "gf_element_rows_device", "gf_element_rows", "gf_sampler_element_marginals"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == m.group(1).count(",") + 1, name
        assert hasattr(_lib.lib(), name)
    import ctypes as C
    assert C.sizeof(_lib.GfElementGroup) == 20 and C.sizeof(_lib.GfElementPlan) == 8 + 20 * (_lib.GF_MAX_DIM + 3)
    assert "#define GF_ELEMENT_MAX_WIDTH (GF_MAX_DIM + 3)" in hdr


def test_plan_validation_of_the_library_and_the_host_build_agree(host):
    import ctypes as C
    cases = [(el.make_plan(U9), 4, 9), (el.make_plan(U9), 3, -1), (el.make_plan([(el.GF_ELEMENT_COPY, [16])]), 16, -1),
             (el.make_plan([(el.GF_ELEMENT_COPY, [0])]), 17, -1), (el.make_plan(U9 * 2 + [(el.GF_ELEMENT_COPY, [0])]), 4, 19),
             (el.make_plan(U9 * 2 + [(el.GF_ELEMENT_FR3, [0, 1])]), 4, -1), (el.make_plan([(el.GF_ELEMENT_COPY, [-1])]), 4, -1)]
    for plan, win, want in cases:
        assert host.elh_plan_width(C.byref(plan), win) == want
        assert _lib.lib().gf_element_plan_width(C.byref(plan), win) == want
    empty = _lib.GfElementPlan()
    assert _lib.lib().gf_element_plan_width(C.byref(empty), 4) == -1
    with pytest.raises(ValueError):
        el.make_plan([(el.GF_ELEMENT_U9, [0, 1])])


# ---- 6. command lines ----------------------------------------------------------------------------------------------------------------
def test_scan_elements_needs_marginals(capsys):
    from golemflavor_amd import scan
    with pytest.raises(SystemExit):
        scan.main(["--config", "C4", "--points", "1", "--elements", "--datadir", "x"])
    assert "--elements needs --marginals" in capsys.readouterr().err
    ns = argparse.Namespace(config="C5", dimension=6, texture="OET")
    ps = scan._point_paramset(ns, scan.sens_grid()[:1])(0)
    assert len(ps) == 12 and el.element_plan(ps)[1][5:14] == list(el.U_NAMES)
    ns.config = "C4"
    assert el.element_plan(scan._point_paramset(ns, scan.texture_grid(6)[:1])(0))[1] == list(el.U_NAMES) + ["m21_2", "m3x_2"]
    w = scan.MarginalWriter("d", str)
    assert w.elements is None


def test_mcmc_plot_elements_arguments():
    from golemflavor_amd import mcmc
    a = mcmc.mcmc_argparse(argparse.ArgumentParser()).parse_args(["--plot-elements", "True"])
    assert a.plot_elements is True
    assert mcmc.element_marginals_file("out/chain_DIM6.npy") == "out/chain_DIM6_elements.npz"
    assert mcmc.element_marginals_file("out/chain_DIM6") == "out/chain_DIM6_elements.npz"
    with pytest.raises(ValueError):
        mcmc.mcmc(None, None, 6, 8, 1, 1, plot_elements=True)
    assert "only" not in mcmc.mcmc_argparse.__doc__ and "elements.npz" in mcmc.mcmc_argparse.__doc__
