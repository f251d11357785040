"""Time a realisation ensemble of the energy-resolved likelihood (golemflavor_amd.realisations.binned_realisation_scan) on
the sens.py frequentist scan at its defaults with --energy-resolved (d = 6, texture OET, 10 segments, 20 energy bins, 8192 seed points
per scale, scipy's tolerances, one restart, adaptive coefficients): T realisations, K starts each, against what it replaces -- one
profile_scan(binned=realisation) per realisation at the same K and seed points, each drawing and propagating its own seeds
(--parent-toys realisations of it; its seconds per realisation are what compares).  Also the seeding, the selection call
(k_toyb_select, k_toy_merge and the copies of its inputs and outputs; repeated --select-repeats times) and the polish on their own.
Host clocks around synchronous calls; the first scan is a warm-up.  One JSON line; --out also writes it to a file
(profiles/binned_realisations/)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import configs as Cf  # noqa: E402
from golemflavor_amd import nested, profile_llh, sens  # noqa: E402
from golemflavor_amd import realisations as R  # noqa: E402
from golemflavor_amd.llh import BinnedMeasurement  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--toys", type=int, default=256)
    ap.add_argument("--starts", type=int, default=R.DEFAULT_TOY_STARTS)
    ap.add_argument("--parent-toys", type=int, default=8, help="realisations the profile_scan path is timed on (0: skip)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--select-repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    args = sens.parse_args(["--segments", str(a.segments), "--stat-method", "frequentist", "--energy-resolved"])
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    scales = nested.sens_scales(args.dimension, a.segments)
    S = len(scales)
    binned = sens.binned_measurement(args, asimov)
    meas = R.draw_binned_realisations(binned, a.toys, seed=0)
    nseed = args.pl_seed_points
    kw = dict(nstarts=a.starts, nseed=nseed, run_ids=np.arange(S), on_nonunitary="-inf")
    runs = []
    for rep in range(a.repeats + 1):                       # the first is a warm-up (code objects, allocations)
        t0 = time.perf_counter()
        res = R.binned_realisation_scan(args, asimov, ps, scales, binned, measurements=meas, **kw)
        res["wall"] = time.perf_counter() - t0                # with the scales' models built, as profile_scan's figure has its models
        if rep:
            runs.append(res)
    last = runs[-1]
    med = {k: float(np.median([r[k] for r in runs])) for k in ("seconds", "seconds_seed", "seconds_select", "seconds_polish", "wall")}
    cols, models, bases, _ = nested._scan_models(args, asimov, ps, scales, args.smearing, args.device, binned=binned)
    try:
        with R.BinnedToySeeds(models, cols, bases, nseed=nseed, seed=args.seed, run_ids=np.arange(S)) as seeds:
            seeds.select(meas, binned.sigma, a.starts)
            sel = []
            for _ in range(a.select_repeats):
                t0 = time.perf_counter()
                seeds.select(meas, binned.sigma, a.starts)
                sel.append(time.perf_counter() - t0)
    finally:
        for m in models:
            m.close()
    band = R.sensitivity_band(last["limits"])
    line = {"tool": "bench_binned_realisations", "dimension": args.dimension, "texture": args.texture.name, "segments": a.segments,
            "nbins": binned.nbins, "toys": a.toys, "starts": a.starts, "seed_points": nseed, "restarts": args.pl_restarts,
            "adaptive": bool(args.pl_adaptive), "seconds_per_scan": [r["seconds"] for r in runs], "seconds_median": med["seconds"],
            "wall_seconds_median": med["wall"], "seconds_seed_median": med["seconds_seed"], "seconds_select_median": med["seconds_select"],
            "seconds_polish_median": med["seconds_polish"], "wall_seconds_per_realisation": med["wall"] / a.toys,
            "select_call_seconds": sel, "select_call_median": float(np.median(sel)),
            "bin_terms_per_select": int(a.toys) * S * int(nseed) * binned.nbins, "nfev": int(last["nfev"].sum()), "niter": int(last["niter"].sum()),
            "nonunitary_seeds": last["nonunitary_seeds"].tolist(), "band_quantiles": band["quantiles"].tolist(),
            "band_limits": band["limits"].tolist(), "without_limit": band["n_without_limit"],
            "ts_q95": R.ts_quantiles(last["ts"], 95.).tolist(),
            "bitwise_repeatable": all(np.array_equal(r["max_lnl"], last["max_lnl"]) for r in runs)}
    pt = min(a.parent_toys, a.toys)
    if pt > 0:
        def parent(t):
            return profile_llh.profile_scan(args, asimov, ps, scales, binned=BinnedMeasurement(meas[t], binned.sigma), **kw)
        parent(0)                                              # warm-up
        t0 = time.perf_counter()
        ml = np.stack([parent(t)["max_lnl"] for t in range(pt)])
        wall = time.perf_counter() - t0
        d = last["max_lnl"][:pt] - ml
        line.update({"parent_toys": pt, "parent_wall_seconds": wall, "parent_wall_seconds_per_realisation": wall / pt,
                     "ratio_per_realisation": (wall / pt) / (med["wall"] / a.toys),
                     "max_lnl_minus_parent_min": float(np.nanmin(d)), "max_lnl_minus_parent_max": float(np.nanmax(d)),
                     "max_lnl_equal_share": float(np.mean(d == 0.0))})
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
