"""Time the device nested sampler on the sens.py scan at its defaults (d = 6, texture OET, 10 segments, nlive 3000, tol 0.01,
batch nlive / 8, 25 walk steps): seconds per scan on a synchronised host clock (gf_nested_run returns when every run is done)
and likelihood evaluations per second.  One JSON line; --out also writes it to a file (profiles/nested/).  Per-kernel times come
from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_nested.py --repeats 1` run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import _lib, nested  # noqa: E402
from golemflavor_amd import sens  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--nlive", type=int, default=nested.DEFAULT_NLIVE)
    ap.add_argument("--walks", type=int, default=nested.DEFAULT_WALKS)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    args = sens.parse_args(["--segments", str(a.segments), "--mn-live-points", str(a.nlive), "--mn-walks", str(a.walks)])
    from golemflavor_amd import configs as Cf
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    scales = nested.sens_scales(args.dimension, args.segments)
    runs = []
    for rep in range(a.repeats + 1):                       # the first is a warm-up (code objects, allocations)
        res = nested.evidence_scan(args, asimov, ps, scales, run_ids=np.arange(len(scales)))
        if rep:
            runs.append(res)
    secs = [r["seconds"] for r in runs]
    ev = int(runs[-1]["nevals"].sum())
    line = {"tool": "bench_nested", "device": _lib.lib().gf_abi_version() and "gfx950", "dimension": args.dimension,
            "texture": args.texture.name, "segments": a.segments, "nlive": a.nlive, "batch": a.nlive // 8, "walks": a.walks,
            "seconds_per_scan": secs, "seconds_median": float(np.median(secs)), "nevals": ev,
            "evals_per_s": ev / float(np.median(secs)), "niter": runs[-1]["niter"].tolist(),
            "lnz": runs[-1]["lnz"].tolist(), "lnz_err": runs[-1]["lnz_err"].tolist(),
            "nonunitary": runs[-1]["nonunitary"].tolist(), "scales": scales.tolist()}
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
