"""Host: the tabulated flavour-plane likelihood's pieces that need no GPU -- the header csrc/gf_table.hpp in its host
build (tests/table/table_host.cpp) against exact rationals and on crafted compositions, the -inf rule, `TabulatedLikelihood.lnl` against
the host build bit for bit, the Python plumbing, the ABI and the parser's refusals.

The bound on the interpolation, with Ta, Tb, Tc the three node values: 16 * 2**-53 * (|Ta| + |Tb| + |Tc|) -- six operations, each with
one rounding of an intermediate that is at most twice that sum."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import table_harness as TH
from golemflavor_amd import _lib, llh, sens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "golemflavor_hip.h")
SIDES = (1, 2, 3, 64, 2048)
U = 2.0 ** -53


def random_table(N, seed, lo=-50.0, hi=5.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, llh.TabulatedLikelihood.node_count(N))


def compositions(N, seed, n=400):
    """random compositions of the triangle, and points tied to the lattice of side N: nodes, edge midpoints, cell diagonals"""
    rng = np.random.default_rng(seed)
    fr = [rng.dirichlet((1, 1, 1), size=n)]
    i = rng.integers(0, N + 1, n)
    j = (rng.random(n) * (N + 1 - i)).astype(np.int64)
    node = np.stack([i / N, j / N, (N - i - j) / N], axis=1)
    fr.append(node)
    fr.append(node + np.array([0.5 / N, 0.0, -0.5 / N]))
    fr.append(node + np.array([0.0, 0.5 / N, -0.5 / N]))
    fr.append(node + np.array([0.5 / N, 0.5 / N, -1.0 / N]))               # fu + fv == 1 inside a cell
    fr.append(node + np.array([0.75 / N, 0.5 / N, -1.25 / N]))             # the downward triangle
    return np.concatenate(fr)


def exact(values, cell, k):
    """the definition in exact rationals on the header's own (i, j, fu, fv, up) of row k, and the bound's sum of magnitudes"""
    ta, tb, tc = (Fraction(float(values[a])) for a in cell["at"][k])
    fu, fv = Fraction(float(cell["fu"][k])), Fraction(float(cell["fv"][k]))
    if not cell["up"][k]:
        fu, fv = 1 - fu, 1 - fv
    return ta + fu * (tb - ta) + fv * (tc - ta), abs(ta) + abs(tb) + abs(tc)


@pytest.mark.parametrize("N", SIDES)
def test_header_against_exact_rationals(N):
    values = random_table(N, 100 + N)
    fr = compositions(N, 200 + N)
    cell = TH.host_locate(N, fr)
    got = TH.host_lookup(values, N, fr)
    assert np.all(cell["ok"] == 1)
    ups = 0
    for k in range(len(fr)):
        i, j = int(cell["i"][k]), int(cell["j"][k])
        assert 0 <= i <= N - 1 and 0 <= j <= N - 1 - i
        assert 0.0 <= cell["fu"][k] <= 1.0 and 0.0 <= cell["fv"][k] <= 1.0
        a00 = int(llh.TabulatedLikelihood.node_index(N, i, j))
        a10 = int(llh.TabulatedLikelihood.node_index(N, i + 1, j))
        if cell["up"][k]:
            assert list(cell["at"][k]) == [a00, a10, a00 + 1]
            ups += 1
        else:
            assert j <= N - 2 - i and cell["fu"][k] + cell["fv"][k] > 1.0
            assert list(cell["at"][k]) == [a10 + 1, a00 + 1, a10]
        ref, mag = exact(values, cell, k)
        assert abs(Fraction(float(got[k])) - ref) <= Fraction(16 * U) * mag, (N, k, fr[k], float(got[k]), float(ref))
    assert 0 < ups and (ups < len(fr) or N == 1)                           # both triangles are exercised


@pytest.mark.parametrize("N", SIDES)
def test_node_layout_and_nodes_reproduce_themselves(N):
    L = TH.build()
    n = llh.TabulatedLikelihood.node_count(N)
    assert L.tabh_node_count(N) == n == (N + 1) * (N + 2) // 2
    i, j = llh.TabulatedLikelihood.node_ij(N)
    at = llh.TabulatedLikelihood.node_index(N, i, j)
    assert np.array_equal(at, np.arange(n))                                # storage order, no gaps
    for k in (0, 1, n // 2, n - 2, n - 1):
        assert L.tabh_node_at(N, int(i[k]), int(j[k])) == k == int(i[k]) * (2 * N + 3 - int(i[k])) // 2 + int(j[k])
    # a node whose composition gives fu = fv = 0 reproduces its value bit for bit
    t = llh.TabulatedLikelihood(random_table(N, 300 + N))
    fr = t.node_fr()
    cell = TH.host_locate(N, fr)
    zero = (cell["fu"] == 0.0) & (cell["fv"] == 0.0) & (cell["i"] == i) & (cell["j"] == j)
    assert np.count_nonzero(zero) >= min(n - (N + 1), n // 2) or N <= 2
    got = TH.host_lookup(t.values, N, fr)
    assert TH.same_bits(got[zero], t.values[zero])
    assert np.all(np.abs(got - t.values) <= 16 * U * 3 * 50.0)             # the clamped nodes of the hypotenuse and of i = N: within the bound


@pytest.mark.parametrize("N", SIDES)
def test_crafted_compositions(N):
    values = random_table(N, 400 + N)
    T = lambda i, j: values[int(llh.TabulatedLikelihood.node_index(N, i, j))]      # noqa: E731
    look = lambda *fr: float(TH.host_lookup(values, N, [fr])[0])                  # noqa: E731
    # every corner
    assert look(0.0, 0.0, 1.0) == T(0, 0)
    corner_e, corner_mu = look(1.0, 0.0, 0.0), look(0.0, 1.0, 0.0)
    for got, want, other in ((corner_e, T(N, 0), T(N - 1, 0)), (corner_mu, T(0, N), T(0, N - 1))):
        assert abs(got - want) <= 16 * U * (abs(want) + 2 * abs(other) + abs(T(N - 1, 1) if N > 1 else 0.0) + 50.0)
    # fr_e == 1 is cell (N - 1, 0) with fu = 1, fv = 0
    c = TH.host_locate(N, [[1.0, 0.0, 0.0]])
    assert (c["i"][0], c["j"][0], c["fu"][0], c["fv"][0], c["up"][0]) == (N - 1, 0, 1.0, 0.0, 1)
    # components slightly outside the triangle are clamped onto it
    assert look(-1e-17, 0.25, 0.75) == look(0.0, 0.25, 0.75)
    assert look(0.25, -1e-17, 0.75) == look(0.25, 0.0, 0.75)
    assert look(1.0 + 1e-16, 0.0, 0.0) == corner_e and look(1.0 + 2.3e-16, -1e-17, 0.0) == corner_e
    assert look(0.0, 1.0 + 2.3e-16, 0.0) == corner_mu
    assert look(0.75, 0.5, -0.25) == look(0.75, 0.25, 0.0)                 # v is clamped to N - u
    assert look(-3.0, 7.0, 0.0) == corner_mu and look(np.inf, 0.3, 0.0) == corner_e and look(-np.inf, -np.inf, 0.0) == T(0, 0)
    # a NaN component in fr_e or fr_mu; fr_tau is not read
    assert np.isnan(look(np.nan, 0.2, 0.3)) and np.isnan(look(0.2, np.nan, 0.3)) and look(0.25, 0.25, np.nan) == look(0.25, 0.25, 0.5)
    # points on each edge and on the hypotenuse: the value is the linear interpolation of the edge's two nodes alone
    for s in (0.0, 0.125, 0.5, 0.8125, 1.0):
        for fr, ends in (((s, 0.0, 1 - s), lambda k: (T(k, 0), T(k + 1, 0))), ((0.0, s, 1 - s), lambda k: (T(0, k), T(0, k + 1))),
                         ((s, 1 - s, 0.0), lambda k: (T(k, N - k), T(k + 1, N - k - 1)))):
            k = min(int(np.floor(s * N)), N - 1)
            f = Fraction(s) * N - k
            a, b = ends(k)
            ref = Fraction(float(a)) + f * (Fraction(float(b)) - Fraction(float(a)))
            assert abs(Fraction(look(*fr)) - ref) <= Fraction(16 * U) * Fraction(3 * 50.0), (N, s, fr)
    # fu + fv == 1 exactly takes the upward triangle
    if N >= 2:
        c = TH.host_locate(N, [[0.5 / N, 0.5 / N, 1 - 1.0 / N]])
        assert (c["i"][0], c["j"][0], c["fu"][0] + c["fv"][0], c["up"][0]) == (0, 0, 1.0, 1)


@pytest.mark.parametrize("N", SIDES)
def test_linear_table_is_reproduced(N):
    a, b, c = 1.5, -7.25, 3.0
    t = llh.TabulatedLikelihood.from_function(lambda fr: a + b * fr[:, 0] + c * fr[:, 1], N)
    fr = compositions(N, 500 + N)
    fr = fr[(fr[:, 0] >= 0) & (fr[:, 1] >= 0) & (fr[:, 0] + fr[:, 1] <= 1)]
    got = TH.host_lookup(t.values, N, fr)
    cell = TH.host_locate(N, fr)
    for k in range(len(fr)):
        # the exact interpolant of the ROUNDED node values at the rounded (u, v), which is the linear function up to the rounding of
        # the nodes (<= 2**-53 * 3 * magnitude each) and of u, v (2**-53 relative each)
        ref, mag = exact(t.values, cell, k)
        assert abs(Fraction(float(got[k])) - ref) <= Fraction(16 * U) * mag
        lin = a + b * fr[k, 0] + c * fr[k, 1]
        assert abs(got[k] - lin) <= (16 + 16) * U * 3 * (abs(a) + abs(b) + abs(c)), (N, k, fr[k])


@pytest.mark.parametrize("N", (2, 3, 64))
def test_minus_infinity_rule(N):
    values = random_table(N, 600 + N)
    hole = int(llh.TabulatedLikelihood.node_index(N, 1, 0))
    values[hole] = -np.inf
    t = llh.TabulatedLikelihood(values)
    fr = compositions(N, 700 + N, n=2000)
    cell = TH.host_locate(N, fr)
    got = TH.host_lookup(values, N, fr)
    touches = np.any(cell["at"] == hole, axis=1)
    assert np.count_nonzero(touches) >= 5 and np.count_nonzero(~touches) >= 5
    assert np.all(got[touches] == -np.inf)                                 # never NaN ...
    assert np.all(np.isfinite(got[~touches]))                              # ... and every other triangle is finite
    # also at the edge opposite the -inf node, where its weight is exactly zero: cell (0, 0) upward has nodes (0,0), (1,0), (0,1)
    for fr0 in ([0.0, 0.0, 1.0], [0.0, 0.5 / N, 1 - 0.5 / N], [0.0, 1.0 / N, 1 - 1.0 / N]):
        c = TH.host_locate(N, [fr0])
        if hole in c["at"][0]:
            assert c["fu"][0] == 0.0
            assert TH.host_lookup(values, N, [fr0])[0] == -np.inf and t.lnl(fr0) == -np.inf
    assert TH.host_lookup(values, N, [[0.0, 0.0, 1.0]])[0] == -np.inf


@pytest.mark.parametrize("N", SIDES)
def test_python_lnl_is_the_host_build_bit_for_bit(N):
    rng = np.random.default_rng(800 + N)
    values = random_table(N, 900 + N)
    values[rng.integers(0, len(values), max(1, len(values) // 50))] = -np.inf
    if not np.any(np.isfinite(values)):
        values[0] = 0.0
    t = llh.TabulatedLikelihood(values)
    fr = np.concatenate([rng.dirichlet((1, 1, 1), size=9000), rng.normal(1 / 3, 0.5, (900, 3)), compositions(N, 1000 + N, n=20)])[:10000]
    assert len(fr) == 10000
    fr[17] = np.nan
    fr[18, 1] = np.nan
    fr[19, 0] = np.inf
    assert TH.same_values(t.lnl(fr), TH.host_lookup(values, N, fr))
    assert isinstance(t.lnl(fr[0]), float)


def test_tabulated_likelihood_plumbing(tmp_path):
    N = 5
    t = llh.TabulatedLikelihood(random_table(N, 7))
    assert t.nside == N and t.values.shape == (21,)
    fr = t.node_fr()
    assert fr.shape == (21, 3) and np.allclose(fr.sum(axis=1), 1.0, atol=1e-15) and np.array_equal(fr[0], [0, 0, 1]) and np.array_equal(fr[-1], [1, 0, 0])
    assert np.array_equal(fr[N], [0, 1, 0])
    # from_ternary and node_fr round-trip
    d = t.to_ternary()
    assert set(d) == {(i, j, N - i - j) for i in range(N + 1) for j in range(N + 1 - i)}
    back = llh.TabulatedLikelihood.from_ternary(d, N)
    assert TH.same_bits(back.values, t.values)
    for (i, j, k), v in d.items():
        assert t.lnl([i / N, j / N, k / N]) == pytest.approx(v, abs=16 * U * 150) and np.array_equal(fr[int(t.node_index(N, i, j))] * N, [i, j, k])
    assert TH.same_bits(llh.TabulatedLikelihood.from_ternary({k[:2]: v for k, v in d.items()}, N).values, t.values)
    assert TH.same_bits(llh.TabulatedLikelihood.from_ternary({k: np.array(v) for k, v in d.items()}, N).values, t.values)   # as plot.heatmap leaves it
    for bad in ({**d, (6, 0, -1): 1.0}, {**d, (1, 1, 1): 1.0}, {k: v for k, v in d.items() if k != (2, 2, 1)}):
        with pytest.raises(ValueError):
            llh.TabulatedLikelihood.from_ternary(bad, N)
    # save / load
    f = tmp_path / "t.npy"
    t.save(str(f))
    assert TH.same_bits(llh.TabulatedLikelihood.load(str(f)).values, t.values) and TH.same_bits(np.load(f), t.values)
    # from_function / from_gaussian: multi_gaussian's arithmetic node by node
    g = llh.TabulatedLikelihood.from_gaussian((0.3, 0.3, 0.4), 0.05, 12, offset=-320.0)
    ref = np.array([llh.multi_gaussian(x, (0.3, 0.3, 0.4), 0.05, offset=-320.0) for x in g.node_fr()])
    assert TH.same_bits(g.values, ref) and g.nside == 12
    assert TH.same_bits(llh.TabulatedLikelihood.from_gaussian((0.3, 0.3, 0.4), 0.05, 12).values,
                        llh.multi_gaussian(g.node_fr(), (0.3, 0.3, 0.4), 0.05, offset=0.0))                       # the default offset is 0
    assert np.any(np.isneginf(llh.TabulatedLikelihood.from_gaussian((0.3, 0.3, 0.4), 0.01, 12).values))      # the underflow wall
    # the refusals of bad tables
    for bad in (np.zeros(4), np.zeros(2), np.zeros((3, 2)), [0.0, np.nan, 0.0], [0.0, np.inf, 0.0], [-np.inf] * 3):
        with pytest.raises(ValueError):
            llh.TabulatedLikelihood(bad)
    assert llh.TabulatedLikelihood([0.0, -np.inf, -np.inf]).nside == 1
    with pytest.raises(ValueError):
        llh.TabulatedLikelihood.from_function(lambda fr: fr[:, 0], 0)
    with pytest.raises(ValueError):
        llh.TabulatedLikelihood.from_function(lambda fr: fr[:, 0], _lib.GF_TABLE_MAX_NSIDE + 1)


def test_abi_header_binding_and_export():
    with open(HEADER) as fh:
        h = fh.read()
    assert re.search(r"^#define\s+GF_ABI_VERSION\s+5\s*$", h, re.M) and _lib.GF_ABI_VERSION == 5
    assert C.sizeof(_lib.GfModelDesc) == 1480 and _lib.lib().gf_sizeof_model_desc() == 1480
    assert re.search(r"^#define\s+GF_TABLE_MAX_NSIDE\s+2048\s*$", h, re.M) and _lib.GF_TABLE_MAX_NSIDE == 2048
    assert TH.build().tabh_nside_limit() == 2048
    assert re.search(r"int\s+gf_model_set_table_likelihood\(gf_model\*\s*m,\s*int\s+nside,\s*const\s+double\*\s*values\);", h)
    assert re.search(r"int\s+gf_model_table_nside\(const\s+gf_model\*\s*m\);", h)
    assert _lib.SIGNATURES["gf_model_set_table_likelihood"] == (C.c_int, [C.c_void_p, C.c_int, _lib._dp])
    assert _lib.SIGNATURES["gf_model_table_nside"] == (C.c_int, [C.c_void_p])
    L = _lib.lib()
    for name in ("gf_model_set_table_likelihood", "gf_model_table_nside"):
        assert hasattr(L, name)                                            # exported
    assert L.gf_model_table_nside(None) == 0
    assert L.gf_model_set_table_likelihood(None, 1, None) == _lib.GF_ERR_INVALID_ARG


def test_sens_arguments_and_file_names(tmp_path):
    f = tmp_path / "table.npy"
    llh.TabulatedLikelihood.from_gaussian((1 / 3, 1 / 3, 1 / 3), 0.02, 8).save(str(f))
    plain = sens.parse_args(["--datadir", "/d"])
    assert plain.likelihood_table is None and sens.likelihood_table(plain) is None
    a = sens.parse_args(["--datadir", "/d", "--likelihood-table", str(f)])
    stat0, llh0 = sens.output_paths(plain)
    assert sens.output_paths(a) == (stat0 + "_ltab", llh0 + "_ltab")
    assert sens.posterior_path(a, -30.0) == sens.posterior_path(plain, -30.0).replace("_scale_", "_ltab_scale_")
    assert sens.likelihood_table(a).nside == 8
    fq = sens.parse_args(["--datadir", "/d", "--likelihood-table", str(f), "--stat-method", "frequentist"])
    assert sens.output_paths(fq)[1].endswith("_ltab")
    for bad in (["--energy-resolved"], ["--binned-measurement", "m.npy"], ["--stat-method", "frequentist", "--realisations", "4"],
                ["--evidence-realisations", "4"]):
        with pytest.raises(SystemExit):
            sens.parse_args(["--datadir", "/d", "--likelihood-table", str(f)] + bad)
    # a file that holds no table ends the command with status 2 before anything is launched
    np.save(tmp_path / "bad.npy", np.zeros(4))
    assert sens.main(["--datadir", str(tmp_path / "out"), "--likelihood-table", str(tmp_path / "bad.npy")]) == 2


def test_standalone_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "table_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DTABLE_HOST_MAIN", "-o", exe, TH.SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "bad 0", (out.stdout, out.stderr)
