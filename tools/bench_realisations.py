"""Time a realisation ensemble (golemflavor_amd.realisations.realisation_scan) on the sens.py frequentist scan at its
defaults (d = 6, texture OET, 10 segments, 8192 seed points per scale, scipy's tolerances, one restart, adaptive coefficients): T = 256
realisations, K = 8 starts each, against the only way without the shared seeding -- one Model per (realisation, scale) in one
SimplexMaximizer with its own seeding at the same K and seed points (--parent-toys realisations of it; its seconds per realisation are
what compares).  Also: the seeding, the selection call (k_toy_select, k_toy_merge and the copies of its small inputs and outputs, on a
synchronised host clock; repeated --select-repeats times) and the polish on their own.  Host clocks around synchronous calls; the
first scan is a warm-up.  One JSON line; --out also writes it to a file (profiles/realisations/).  Per-kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/bench_realisations.py --repeats 1 --parent-toys 0` run."""
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
from golemflavor_amd import fr as fr_utils  # noqa: E402
from golemflavor_amd import nested, profile_llh, sens  # noqa: E402
from golemflavor_amd import realisations as R  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.enums import ParamTag  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


def parent_path(args, asimov, ps, scales, meas, K, nseed):
    """One Model per (realisation, scale), every run with its own seeding: (seconds of building the models, seconds of the maximiser,
    max_lnl [T][S])."""
    T, S = len(meas), len(scales)
    t0 = time.perf_counter()
    models, bases = [], []
    cols = None
    try:
        for t in range(T):
            for sc in scales:
                sp = nested._scale_paramset(ps, float(sc))
                names = list(sp.names)
                cols = [i for i in range(len(names)) if names[i] != "logLam"]
                models.append(Model(compile_model(sp, "BSM_GAUSS", bestfit_fr=meas[t], smearing=args.smearing, source_ratio=args.source_ratio,
                                                  texture=args.texture, dimension=args.dimension, binning=args.binning)))
                bases.append(np.array(sp.values, dtype=np.float64))
        t1 = time.perf_counter()
        with profile_llh.SimplexMaximizer(models, cols, bases, nstarts=K, nseed=nseed, seed=args.seed, on_nonunitary="-inf",
                                          adaptive=bool(args.pl_adaptive), restarts=args.pl_restarts,
                                          run_ids=np.tile(np.arange(S), T)) as mx:
            res = mx.run()
        t2 = time.perf_counter()
    finally:
        for m in models:
            m.close()
    return t1 - t0, t2 - t1, res["max_lnl"].reshape(T, S)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--toys", type=int, default=256)
    ap.add_argument("--starts", type=int, default=R.DEFAULT_TOY_STARTS)
    ap.add_argument("--parent-toys", type=int, default=None, help="realisations the parent path is timed on (default --toys; 0: skip)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--select-repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    args = sens.parse_args(["--segments", str(a.segments), "--stat-method", "frequentist"])
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    scales = nested.sens_scales(args.dimension, a.segments)
    S = len(scales)
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    meas = R.draw_realisations(bf, args.smearing, a.toys, seed=0)
    nseed = args.pl_seed_points
    kw = dict(measurements=meas, nstarts=a.starts, nseed=nseed, run_ids=np.arange(S), on_nonunitary="-inf")
    runs = []
    for rep in range(a.repeats + 1):                       # the first is a warm-up (code objects, allocations)
        t0 = time.perf_counter()
        res = R.realisation_scan(args, asimov, ps, scales, **kw)
        res["wall"] = time.perf_counter() - t0                # with the scales' models built, as the parent path's figure has its models
        if rep:
            runs.append(res)
    last = runs[-1]
    med = {k: float(np.median([r[k] for r in runs])) for k in ("seconds", "seconds_seed", "seconds_select", "seconds_polish", "wall")}
    # the selection call on its own, on seeds that stay on the device
    cols, models, bases, _ = nested._scan_models(args, asimov, ps, scales, args.smearing, args.device)
    try:
        with R.ToySeeds(models, cols, bases, nseed=nseed, seed=args.seed, run_ids=np.arange(S)) as seeds:
            seeds.select(meas, args.smearing, a.starts)
            sel = []
            for _ in range(a.select_repeats):
                t0 = time.perf_counter()
                seeds.select(meas, args.smearing, a.starts)
                sel.append(time.perf_counter() - t0)
    finally:
        for m in models:
            m.close()
    band = R.sensitivity_band(last["limits"])
    line = {"tool": "bench_realisations", "dimension": args.dimension, "texture": args.texture.name, "segments": a.segments,
            "toys": a.toys, "starts": a.starts, "seed_points": nseed, "restarts": args.pl_restarts, "adaptive": bool(args.pl_adaptive),
            "seconds_per_scan": [r["seconds"] for r in runs], "seconds_median": med["seconds"], "wall_seconds_median": med["wall"],
            "seconds_seed_median": med["seconds_seed"],
            "seconds_select_median": med["seconds_select"], "seconds_polish_median": med["seconds_polish"],
            "seconds_per_realisation": med["seconds"] / a.toys, "wall_seconds_per_realisation": med["wall"] / a.toys,
            "select_call_seconds": sel, "select_call_median": float(np.median(sel)),
            "scores_per_select": int(a.toys) * S * int(nseed), "nfev": int(last["nfev"].sum()), "niter": int(last["niter"].sum()),
            "nonunitary_seeds": last["nonunitary_seeds"].tolist(), "band_quantiles": band["quantiles"].tolist(),
            "band_limits": band["limits"].tolist(), "without_limit": band["n_without_limit"],
            "ts_q95": R.ts_quantiles(last["ts"], 95.).tolist(),
            "bitwise_repeatable": all(np.array_equal(r["max_lnl"], last["max_lnl"]) for r in runs)}
    pt = a.toys if a.parent_toys is None else a.parent_toys
    if pt > 0:
        parent_path(args, asimov, ps, scales, meas[:1], a.starts, nseed)             # warm-up
        build_s, run_s, ml = parent_path(args, asimov, ps, scales, meas[:pt], a.starts, nseed)
        d = last["max_lnl"][:pt] - ml
        line.update({"parent_toys": pt, "parent_seconds_models": build_s, "parent_seconds_maximiser": run_s,
                     "parent_seconds_per_realisation": (build_s + run_s) / pt, "parent_maximiser_seconds_per_realisation": run_s / pt,
                     "ratio_per_realisation": ((build_s + run_s) / pt) / (med["wall"] / a.toys),
                     "ratio_per_realisation_device_calls": (run_s / pt) / (med["seconds"] / a.toys),
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
