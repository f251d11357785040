"""Time the device profile-likelihood maximiser on the sens.py frequentist scan at its defaults (d = 6, texture OET, 10
segments, 64 starts from 8192 seed points, scipy's tolerances, 200 n iterations, one restart, adaptive coefficients): seconds
per scan on a synchronised host clock (gf_simplex_run returns when every start is done), device evaluations per second, and
the starts that agree with each scale's best.  --nested also runs the nested sampler's default scan and sets its max lnL (the
`fr_maxllh` the Bayesian path writes) beside the profile maximum.  One JSON line; --out also writes it to a file
(profiles/profile_llh/).  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python
tools/bench_profile.py --repeats 1` run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import nested, profile_llh  # noqa: E402
from golemflavor_amd import sens  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nested", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    args = sens.parse_args(["--segments", str(a.segments), "--stat-method", "frequentist"])
    from golemflavor_amd import configs as Cf
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    scales = nested.sens_scales(args.dimension, args.segments)
    runs = []
    for rep in range(a.repeats + 1):                       # the first is a warm-up (code objects, allocations)
        res = profile_llh.profile_scan(args, asimov, ps, scales, run_ids=np.arange(len(scales)))
        if rep:
            runs.append(res)
    secs = [r["seconds"] for r in runs]
    last = runs[-1]
    ev = int(last["nevals"].sum())
    line = {"tool": "bench_profile", "dimension": args.dimension, "texture": args.texture.name, "segments": a.segments,
            "starts": args.pl_starts, "seed_points": args.pl_seed_points, "restarts": args.pl_restarts,
            "adaptive": bool(args.pl_adaptive), "seconds_per_scan": secs, "seconds_median": float(np.median(secs)),
            "nevals": ev, "evals_per_s": ev / float(np.median(secs)), "nfev": last["nfev"].tolist(),
            "niter": last["niter"].tolist(), "starts_used": last["nstarts"].tolist(),
            "starts_agreeing": last["starts_agreeing"].tolist(), "max_lnl": last["max_lnl"].tolist(),
            "nonunitary": last["nonunitary"].tolist(), "scales": scales.tolist(),
            "bitwise_repeatable": all(np.array_equal(r["max_lnl"], last["max_lnl"]) for r in runs)}
    if a.nested:
        nargs = sens.parse_args(["--segments", str(a.segments)])
        nres = nested.evidence_scan(nargs, asimov, ps, scales, run_ids=np.arange(len(scales)))
        line["nested_max_lnl"] = nres["max_lnl"].tolist()
        line["profile_minus_nested"] = (last["max_lnl"] - nres["max_lnl"]).tolist()
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
