#!/usr/bin/env python3
"""Generate tests/golden/golden_interval.npz by calling the reference's `misc.interval` and `misc.calc_nbins`
(golemflavor/misc.py:174-213) on seeded columns.

Run where the reference is available (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_interval.py

Nothing from the reference is copied: its functions are called, and inputs and outputs are stored as plain arrays (loadable with
allow_pickle=False).  Harness-side shims, none of which edits a reference file:
  * `fractions.gcd` / `collections.Sequence` aliases so the py2-era modules import (as tests/golden/make_golden.py);
  * `np.linspace` is given `num=int(num)`: `calc_nbins` returns a float and numpy >= 1.18 refuses a float `num`.  int() of a NaN
    raises ValueError and of an infinity OverflowError, which is recorded like every other exception.

Per case NAME the file holds NAME_x (the column), NAME_pct (the percentiles), NAME_low / NAME_center / NAME_up (per percentile, NaN
where the reference raised), NAME_exc (per percentile, the exception's class name or ''), NAME_nbins (calc_nbins' value, NaN where it
is not a number) and `cases`, the names in order.
"""
import collections
import collections.abc
import fractions
import math
import os
import sys
import warnings

fractions.gcd = math.gcd
collections.Sequence = collections.abc.Sequence
sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("GOLEMFLAVOR_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

_linspace = np.linspace


def _linspace_int_num(start, stop, num=50, *args, **kw):
    return _linspace(start, stop, int(num), *args, **kw)


np.linspace = _linspace_int_num

from golemflavor import misc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PERCENTILES = (68., 90., 99., 100.)


def columns():
    rng = np.random.default_rng(20240611)
    c = {}
    c["normal"] = rng.standard_normal(4096)
    c["uniform"] = rng.uniform(-1., 3., 4095)
    # the mode sits in a narrow cluster at the top: the walk reaches the upper end and goes on downward
    c["bimodal"] = np.concatenate([rng.normal(0., 1., 2096), rng.normal(6., 0.05, 2000)])
    c["rounded"] = np.round(rng.normal(0., 1., 4096), 1)                     # ties and long runs of duplicates
    c["zeros_uniform"] = np.concatenate([np.zeros(500), rng.uniform(0., 1., 3000)])   # mode bin at the edge, window from index 0
    c["negative"] = -rng.lognormal(0., 0.5, 4096)
    c["mixed"] = rng.normal(0.5, 3., 4096)
    c["magnitudes"] = 10. ** rng.uniform(-6., 6., 4096)                      # twelve decades; thousands of bins
    c["constant"] = np.full(100, 3.5)
    c["n1"] = np.array([0.25])
    c["n2"] = np.array([2., 1.])
    c["n3"] = np.array([0.5, -1.5, 4.])
    for k in ("normal", "bimodal", "rounded", "zeros_uniform"):
        c[k] = rng.permutation(c[k])
    return c


def main():
    out = {"cases": np.array(list(columns()))}
    for name, x in columns().items():
        low, cen, up, exc = [], [], [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                nb = float(misc.calc_nbins(x))
            except Exception:                                                # noqa: BLE001
                nb = float("nan")
            for p in PERCENTILES:
                try:
                    a, c, b = misc.interval(x, p)
                    low.append(a); cen.append(c); up.append(b); exc.append("")
                except Exception as e:                                       # noqa: BLE001
                    low.append(np.nan); cen.append(np.nan); up.append(np.nan); exc.append(type(e).__name__)
        out[name + "_x"] = np.asarray(x, dtype=np.float64)
        out[name + "_pct"] = np.array(PERCENTILES)
        out[name + "_low"], out[name + "_center"], out[name + "_up"] = np.array(low, dtype=np.float64), np.array(cen, dtype=np.float64), np.array(up, dtype=np.float64)
        out[name + "_exc"] = np.array(exc)
        out[name + "_nbins"] = np.float64(nb)
        print("%-14s n %5d nbins %-8g %s" % (name, len(x), nb, " ".join(e or "ok" for e in exc)))
    path = os.path.join(HERE, "golden_interval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; reference:", misc.__file__, "numpy", np.__version__)


if __name__ == "__main__":
    main()
