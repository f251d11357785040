"""Host side of the posterior marginals (golemflavor_amd.marginals, the --marginals options of the scan): no GPU needed.

  * the percentile rule (two order statistics and numpy's `linear` interpolation) equals np.percentile with ==, the order
    statistics taken with np.partition, never with the package;
  * the edges are np.histogram_bin_edges', radius and weights are scipy's;
  * argument validation, the pair ordering, the .npz layout of a hand-made result;
  * the new entry points are declared in the header, bound and exported by the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.ndimage import _filters as scipy_filters

from golemflavor_amd import _lib, contour, marginals
from golemflavor_amd import configs as Cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (2.5, 5, 16, 50, 84, 90, 95, 99, 99.5)


def columns():
    rng = np.random.default_rng(11)
    out = [("n=%d" % n, rng.normal(size=n)) for n in (1000, 102400, 512000, 2048001)]
    out.append(("repeated", rng.integers(0, 7, 5000).astype(np.float64)))
    out.append(("n=2", np.array([3.25, -1.5])))
    out.append(("n=1", np.array([0.1])))
    return out


@pytest.mark.parametrize("name,x", columns(), ids=[n for n, _ in columns()])
def test_percentile_rule_equals_numpy(name, x):
    n = len(x)
    for q in QS:
        lo, hi, gamma = marginals.percentile_ranks(n, q)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0. <= gamma
        part = np.partition(x, sorted({lo, hi}))
        got = marginals.percentile_from_order_statistics(n, q, part[lo], part[hi])
        assert got == np.percentile(x, q), (name, q, got, np.percentile(x, q))
    assert marginals.percentile_ranks(n, 0.)[:2] == (0, min(1, n - 1)) or n == 1
    assert marginals.percentile_ranks(n, 100.)[:2] == (n - 1, n - 1)
    assert np.isnan(marginals.percentile_from_order_statistics(0, 50., np.nan, np.nan))


def test_edges_are_numpys_and_weights_scipys():
    ranges = [(0., 1.), tuple(Cf.SCALE_BOUNDARIES[6]), (0., 2 * np.pi), (-3.7, 11.3), (1e-3, 1e-2)]
    for nb in (10, 50, 51, 100, 126):
        e = marginals.bin_edges(ranges, nb)
        assert e.shape == (len(ranges), nb + 1)
        for c, r in enumerate(ranges):
            assert np.array_equal(e[c], np.histogram_bin_edges(np.zeros(1), bins=nb, range=r))
            assert e[c, 0] == r[0] and e[c, -1] == r[1]
    for sigma in (0.05, 0.6, 1.5):
        prep = marginals.prepare(2, [(0, 1), (0, 1)], hist_smooth=sigma)
        r = int(4.0 * sigma + 0.5)
        assert prep["radius"] == r == contour.gaussian_radius(sigma)
        assert np.array_equal(prep["weights"], scipy_filters._gaussian_kernel1d(sigma, 0, r))
    # plot_Tchain's settings are the defaults (golemflavor/plot.py:456-459)
    prep = marginals.prepare(2, [(0, 1), (0, 1)])
    assert (prep["bins_1d"], prep["bins_2d"], list(prep["coverage"]), list(prep["q"]), prep["radius"]) == (100, 50, [90., 99.], [5., 50., 95.], 0)


def test_pair_ordering_and_tree_depth():
    assert marginals.pair_list(1) == []
    assert marginals.pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert len(marginals.pair_list(12)) == 66
    for W in (2, 7, 12, 19):
        for p, (i, j) in enumerate(marginals.pair_list(W)):
            assert p == i * (2 * W - i - 1) // 2 + (j - i - 1)       # the closed form the kernel uses
    assert marginals.moment_tree_depth(1) == 16 + 6 + 3 + 1 + 6 + 3
    assert marginals.moment_tree_depth(4096 * 256 + 1) == 16 + 6 + 3 + 2 + 6 + 3


def test_argument_validation():
    ok = [(0., 1.), (-1., 1.)]
    with pytest.raises(ValueError):
        marginals.prepare(3, ok)                                      # ranges for another width
    for bad in ([(0., 1.), (1., 1.)], [(0., 1.), (2., 1.)], [(0., np.inf), (0., 1.)], [(0., 1.), (np.nan, 1.)], [0., 1.]):
        with pytest.raises(ValueError):
            marginals.prepare(2, bad)
    for kw in (dict(bins_1d=0), dict(bins_2d=1025), dict(coverage=[0.]), dict(coverage=[101.]), dict(coverage=list(range(1, 10))),
               dict(percentiles=[-1.]), dict(percentiles=[100.5]), dict(percentiles=list(range(9))), dict(ranks=list(range(11))),
               dict(names=["a"])):
        with pytest.raises(ValueError):
            marginals.prepare(2, ok, **kw)
    assert marginals.prepare(2, ok, percentiles=[], ranks=list(range(16)))["ranks"].dtype == np.int64
    with pytest.raises(ValueError):
        marginals.chain_marginals(np.zeros(5), ok, model=None)


def test_npz_layout(tmp_path):
    W, nb1, nb2, cov = 3, 4, 2, np.array([90., 99.])
    pairs = marginals.pair_list(W)

    def reg(cls, nb, n):
        return [cls(nb, c, n, 0, 0.25, 0.125, 0.5, np.arange(n)[::-1], np.linspace(1, 0.5, n)) for c in cov]
    r = marginals.MarginalResult(
        names=["a", "b", "c"], ranges=np.array([(0., 1.)] * W), edges1=marginals.bin_edges([(0, 1)] * W, nb1),
        edges2=marginals.bin_edges([(0, 1)] * W, nb2), pairs=np.array(pairs), counts1=np.ones((W, nb1), np.uint64),
        counts2=np.ones((len(pairs), nb2, nb2), np.uint64), nvalid=4, mean=np.zeros(W), cov=np.eye(W), ncol=np.full(W, 4),
        order_ranks=np.zeros((W, 6), np.int64), order_stats=np.zeros((W, 6)), percentile_q=np.array([5., 50., 95.]),
        percentiles=np.zeros((W, 3)), coverage=cov, regions1=[reg(marginals._Region1, nb1, 3) for _ in range(W)],
        regions2=[reg(marginals._Region2, nb2, 4) for _ in pairs])
    assert r.regions1[0][0].cells.shape == (3, 1) and r.regions2[0][0].cells.tolist() == [[1, 1], [1, 0], [0, 1], [0, 0]]
    path = str(tmp_path / "m.npz")
    r.save(path)
    z = np.load(path)
    want = {"names": (W,), "ranges": (W, 2), "edges1": (W, nb1 + 1), "edges2": (W, nb2 + 1), "pairs": (3, 2), "counts1": (W, nb1),
            "counts2": (3, nb2, nb2), "nvalid": (), "mean": (W,), "cov": (W, W), "ncol": (W,), "order_ranks": (W, 6),
            "order_stats": (W, 6), "percentile_q": (3,), "percentiles": (W, 3), "coverage": (2,),
            "r1_thres": (W, 2), "r1_saturated": (W, 2), "r1_level_in": (W, 2), "r1_level_out": (W, 2), "r1_mass": (W, 2),
            "r1_cells": (W, 3), "r1_density": (W, 3), "r2_thres": (3, 2), "r2_saturated": (3, 2), "r2_level_in": (3, 2),
            "r2_level_out": (3, 2), "r2_mass": (3, 2), "r2_cells": (3, 4), "r2_density": (3, 4)}
    assert {k: z[k].shape for k in z.files} == want
    assert z["names"].tolist() == ["a", "b", "c"] and z["r2_cells"][0].tolist() == [3, 2, 1, 0] and z["counts1"].dtype == np.uint64


def test_marginal_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "golemflavor_hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ("gf_marginals_device", "gf_marginals", "gf_sampler_marginals"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        res, args = _lib.SIGNATURES[name]
        proto = header[header.index("int %s(" % name):]
        proto = proto[:proto.index(";")]
        assert len(args) == proto.count(",") + 1, name
        assert hasattr(L, name)
    assert re.search(r"#define\s+GF_MARGINAL_MAX_RANKS\s+%d\b" % _lib.GF_MARGINAL_MAX_RANKS, header)
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", header)             # additive: the ABI version stays
    # the structs, field for field: every member the header declares, in order
    for struct, cls in (("gf_marginal_spec", _lib.GfMarginalSpec), ("gf_marginal_out", _lib.GfMarginalOut)):
        body = header[header.index("typedef struct %s {" % struct):header.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.findall(r"[A-Za-z_0-9]+", d)[-1] for d in decl.split(",")]
        assert fields == [n for n, _ in cls._fields_], struct
    assert C.sizeof(_lib.GfMarginalOut) == 22 * C.sizeof(C.c_void_p)
    with open(os.path.join(ROOT, "golemflavor_amd", "csrc", "Makefile")) as f:
        assert "gf_marginal.hip" in f.read()
    # nothing undeclared was exported for it
    with open(_lib.LIB_PATH, "rb") as f:
        assert not re.search(rb"gf_internal_\w*margin", f.read())


def test_scan_refuses_marginals_without_datadir(capsys):
    from golemflavor_amd import scan
    with pytest.raises(SystemExit):
        scan.main(["--config", "C4", "--points", "1", "--marginals"])
    assert "--marginals needs --datadir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        scan.main(["--config", "C4", "--points", "1", "--datadir", "x", "--marginals", "--marginal-coverage", "0"])
