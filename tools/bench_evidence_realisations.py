"""Time a Bayesian realisation ensemble (golemflavor_amd.realisations.evidence_realisation_scan) on the sens.py evidence
scan (d = 6, texture OET; --segments, --nlive, --smearing): T realisations reweighted from the one Asimov scan, against the
alternative the reweighting replaces -- one nested scan per realisation, taken as T x the measured Asimov scan of the same run -- and
against --reruns genuine re-runs on models compiled with the realisation, whose ln Z the reweighted ones are also compared with.  The
reweighting call is repeated --repeats times on the same sampler (host clock around the synchronous call: the gather, one propagation
of every run's points, the kernels and the copies).  One JSON line; --out also writes it to a file and, with --readme, a README.txt
beside it (profiles/evidence_realisations/).  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_evidence_realisations.py --repeats 1 --reruns 0` run."""
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
from golemflavor_amd import nested, sens  # noqa: E402
from golemflavor_amd import realisations as R  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.enums import ParamTag  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


TESTS_MARKER = "---- measured by the tests"


def rerun(args, ps, scales, m, nlive, run_ids):
    """A genuine nested scan under measurement m: (seconds of the scan, lnz [S], lnz_err [S])"""
    models, bases = [], []
    cols = None
    try:
        for sc in scales:
            sp = nested._scale_paramset(ps, float(sc))
            names = list(sp.names)
            cols = [i for i in range(len(names)) if names[i] != "logLam"]
            models.append(Model(compile_model(sp, "BSM_GAUSS", bestfit_fr=m, smearing=args.smearing, source_ratio=args.source_ratio,
                                              texture=args.texture, dimension=args.dimension, binning=args.binning)))
            bases.append(np.array(sp.values, dtype=np.float64))
        with nested.NestedSampler(models, cols, bases, nlive=nlive, seed=args.seed, on_nonunitary="-inf", tol=args.mn_tolerance,
                                  walks=args.mn_walks, run_ids=run_ids) as s:
            t0 = time.perf_counter()
            res = s.run()
            dt = time.perf_counter() - t0
    finally:
        for mm in models:
            mm.close()
    return dt, res["lnz"], res["lnz_err"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--nlive", type=int, default=nested.DEFAULT_NLIVE)
    ap.add_argument("--smearing", type=float, default=0.02)
    ap.add_argument("--toys", type=int, default=1024)
    ap.add_argument("--reruns", type=int, default=3, help="genuine re-runs under the first realisations (0: skip)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", action="store_true", help="with --out: also write README.txt beside it")
    a = ap.parse_args(argv)
    args = sens.parse_args(["--segments", str(a.segments), "--mn-live-points", str(a.nlive), "--smearing", str(a.smearing)])
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    scales = nested.sens_scales(args.dimension, a.segments)
    S = len(scales)
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    meas = R.draw_realisations(bf, args.smearing, a.toys, seed=0)
    nested.evidence_scan(args, asimov, ps, scales[:1], run_ids=[0], nlive=64, on_nonunitary="-inf")       # warm-up (code objects)
    t0 = time.perf_counter()
    run = nested.evidence_scan(args, asimov, ps, scales, run_ids=np.arange(S), on_nonunitary="-inf", return_sampler=True)
    wall_scan = time.perf_counter() - t0
    s = run["sampler"]
    try:
        npoints = s.posterior()["npoints"]
        rw, secs = None, []
        for _ in range(a.repeats + 1):                         # the first is a warm-up
            t0 = time.perf_counter()
            out = s.reweight_evidence(meas)
            secs.append(time.perf_counter() - t0)
            assert rw is None or all(np.array_equal(out[k], rw[k], equal_nan=True) for k in out)
            rw = out
        secs = secs[1:]
        ess_run = s.posterior()["ess"]
    finally:
        s.close()
        for m in run["models"]:
            m.close()
    lim = R.evidence_limits(scales, rw["lnz"])
    band = R.sensitivity_band(lim["limits"])
    med = float(np.median(secs))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = rw["ess"] / ess_run[None, :]
    line = {"tool": "bench_evidence_realisations", "dimension": args.dimension, "texture": args.texture.name, "segments": a.segments,
            "nlive": a.nlive, "smearing": a.smearing, "toys": a.toys, "points_per_scale": npoints.tolist(), "points": int(npoints.sum()),
            "asimov_scan_seconds": run["seconds"], "asimov_scan_wall_seconds": wall_scan, "reweight_seconds": secs,
            "reweight_seconds_median": med, "reweight_seconds_per_realisation": med / a.toys,
            "point_realisations_per_second": float(npoints.sum()) * a.toys / med,
            "one_scan_per_realisation_seconds": run["seconds"] * a.toys, "ratio_to_one_scan_per_realisation": run["seconds"] * a.toys / med,
            "lowest_ess_fraction_per_scale": [None if not np.isfinite(v) else float(v) for v in np.min(np.where(np.isnan(frac), np.inf, frac), axis=0)],
            "band_quantiles": band["quantiles"].tolist(), "band_limits": [None if not np.isfinite(v) else float(v) for v in band["limits"]],
            "without_limit": band["n_without_limit"], "discovered": int(lim["discovered"].sum())}
    if a.reruns > 0:
        dts, devs = [], []
        for t in range(a.reruns):
            dt, lnz2, err2 = rerun(args, ps, scales, meas[t], a.nlive, 1000 * (t + 1) + np.arange(S))
            dts.append(dt)
            with np.errstate(invalid="ignore"):
                devs.append(((rw["lnz"][t] - lnz2) / np.sqrt(run["lnz_err"] ** 2 + err2 ** 2)).tolist())
        line.update({"reruns": a.reruns, "rerun_scan_seconds": dts,
                     "rerun_deviation_in_sigma": [[None if not np.isfinite(v) else float(v) for v in row] for row in devs]})
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        if a.readme:
            readme = os.path.join(os.path.dirname(a.out) or ".", "README.txt")
            kept = ""
            if os.path.exists(readme):                         # what the tests measured stays: everything from the marker line on
                with open(readme) as f:
                    old = f.read()
                kept = old[old.index(TESTS_MARKER):] if TESTS_MARKER in old else ""
            with open(readme, "w") as f:
                f.write("Bayesian realisation ensembles (gf_ns_toys.hip; DESIGN.md 6k), tools/bench_evidence_realisations.py on one MI355X:\n"
                        "d = 6, texture OET, %d segments, nlive %d, smearing %g, T = %d realisations (default_rng(0)).\n"
                        "Asimov evidence scan %.3f s (%d points kept); the reweighting of all T realisations at all scales %.4f s (median of "
                        "%d calls, host clock\naround the synchronous call: gather, one propagation of the points, kernels, copies), %.3g "
                        "(point, realisation) pairs a second.\nOne nested scan per realisation, taken as T x the Asimov scan: %.1f s.\n"
                        "%s holds the whole line.\n"
                        % (a.segments, a.nlive, a.smearing, a.toys, run["seconds"], int(npoints.sum()), med, len(secs),
                           line["point_realisations_per_second"], line["one_scan_per_realisation_seconds"], os.path.basename(a.out)))
                f.write(("\n" + kept) if kept else "")
    return 0


if __name__ == "__main__":
    sys.exit(main())
