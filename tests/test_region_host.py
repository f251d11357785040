"""Host side of the credible regions (golemflavor_amd.contour, the --regions options of the scan): no GPU needed.

  * `gaussian_weights` is scipy's own kernel, bit for bit, on both sides of every radius change up to GF_REGION_MAX_RADIUS;
  * the new entry points are declared in the header and bound;
  * RegionResult's plumbing (index unravelling, as_dict) on a hand-made array;
  * the scan refuses --regions without --datadir or with --config C5."""
import os
import re

import numpy as np
import pytest
from scipy.ndimage import _filters as scipy_filters

from golemflavor_amd import _lib, contour

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sigmas_around_radius_changes():
    """The radius int(4 sigma + 0.5) steps from r - 1 to r at sigma = (r - 0.5) / 4, which is a double: that sigma, the doubles on
    both sides of it, and a sigma inside every radius."""
    out = [0.05, 0.124, 0.125]
    for r in range(1, _lib.GF_REGION_MAX_RADIUS + 2):
        s = (r - 0.5) / 4.
        out += [np.nextafter(s, 0.), s, np.nextafter(s, np.inf), r / 4.]
    return out


def test_gaussian_weights_are_scipys_bit_for_bit():
    seen = set()
    for sigma in sigmas_around_radius_changes():
        w = contour.gaussian_weights(sigma)
        r = int(4.0 * float(sigma) + 0.5)
        assert contour.gaussian_radius(sigma) == r and len(w) == 2 * r + 1
        want = scipy_filters._gaussian_kernel1d(float(sigma), 0, r)
        assert np.array_equal(w, want) and w.dtype == np.float64, sigma
        assert np.array_equal(w, w[::-1])                # symmetric exactly: scipy takes its symmetric branch
        seen.add(r)
    assert seen >= set(range(0, _lib.GF_REGION_MAX_RADIUS + 1))
    assert contour.gaussian_radius(0.05) == 0 and contour.gaussian_radius(0.124) == 0 and contour.gaussian_radius(0.125) == 1
    assert np.array_equal(contour.gaussian_weights(0.05), [1.0])
    # another truncate, as gaussian_filter(truncate=...) would use it
    assert np.array_equal(contour.gaussian_weights(1.0, truncate=3.0), scipy_filters._gaussian_kernel1d(1.0, 0, 3))


def test_region_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "golemflavor_hip.h")) as f:
        header = f.read()
    for name in ("gf_flavor_region_device", "gf_flavor_region", "gf_sampler_regions"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        res, args = _lib.SIGNATURES[name]
        proto = header[header.index("int %s(" % name):]
        proto = proto[:proto.index(";")]
        assert len(args) == proto.count(",") + 1, name      # one ctypes type per declared parameter
    assert re.search(r"#define\s+GF_REGION_MAX_RADIUS\s+%d\b" % _lib.GF_REGION_MAX_RADIUS, header)
    assert re.search(r"#define\s+GF_REGION_MAX_COVERAGES\s+%d\b" % _lib.GF_REGION_MAX_COVERAGES, header)
    assert re.search(r"#define\s+GF_ABI_VERSION\s+5\b", header)             # additive: the ABI version stays
    with open(os.path.join(ROOT, "golemflavor_amd", "csrc", "Makefile")) as f:
        assert "gf_region.hip" in f.read()


def test_region_result_plumbing():
    nb = 7
    cells = np.array([[6, 5, 4], [0, 0, 0], [0, 0, 6], [3, 0, 1], [6, 6, 6]])
    flat = (cells[:, 0] * nb + cells[:, 1]) * nb + cells[:, 2]
    assert np.array_equal(contour.unravel_cells(flat, nb), cells)
    assert np.array_equal(contour.unravel_cells(flat, nb), np.stack(np.unravel_index(flat, (nb, nb, nb)), axis=1))
    dens = np.array([0.4, 0.3, 0.15, 0.1, 0.05])
    r = contour.RegionResult(nb, 90., 5, 0, 0.05, 0.01, 1.0 - 1e-3, flat.astype(np.int32), dens)
    assert r.thres == 5 and r.saturated is False and r.nbins == nb and r.coverage == 90.
    assert np.array_equal(r.cells, cells) and r.cells.shape == (5, 3)
    d = r.as_dict()
    assert d == {(6, 5, 4): 0.4, (0, 0, 0): 0.3, (0, 0, 6): 0.15, (3, 0, 1): 0.1, (6, 6, 6): 0.05}
    assert all(isinstance(k, tuple) and all(isinstance(x, int) for x in k) for k in d)
    empty = contour.RegionResult(nb, 50., 0, 0, np.nan, 1.0, 0.0, np.empty(0, dtype=np.int32), np.empty(0))
    assert empty.cells.shape == (0, 3) and empty.as_dict() == {}
    # the coverage argument: a number or 1..8 numbers
    assert contour._coverages(90)[0] is True and contour._coverages([90, 99])[0] is False
    for bad in ([], list(range(1, 10))):
        with pytest.raises(ValueError):
            contour._coverages(bad)


@pytest.mark.parametrize("argv", [["--config", "C4", "--regions", "90", "99"],
                                  ["--config", "C5", "--datadir", "somewhere", "--regions", "90"],
                                  ["--config", "C4", "--datadir", "somewhere", "--regions", "0"],
                                  ["--config", "C4", "--datadir", "somewhere", "--regions", "101"]])
def test_scan_refuses_regions_it_cannot_save(argv, capsys):
    from golemflavor_amd import scan
    with pytest.raises(SystemExit) as exc:
        scan.main(argv)
    assert exc.value.code == 2                               # argparse's error exit, before anything touches a device
    assert "--regions" in capsys.readouterr().err
