"""Time the tabulated flavour-plane likelihood (k_bsm_table, csrc/gf_table.hip) against the flux-averaged Gaussian one, in
one process:

  bulk    Model.lnprob_device of a model with a table against the same model without one, on the same rows, with and without a status
          array: 7 columns (the texture posterior) and 12 (the sens posterior), 20 energy bins, --rows rows around the seeds' box with
          the scale below where the reference starts raising.  Device events around each launch, medians of --repeats after a warm-up.
  scan    nested.evidence_scan at sens defaults (dimension 6, --segments scales, nlive and walks as `python -m golemflavor_amd.sens`) with
          a Gaussian table of side --nside against the Gaussian itself, each --scan-repeats times after a warm-up, host clock.

One JSON line; --out also appends it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import configs as Cf  # noqa: E402
from golemflavor_amd import fr as fr_utils  # noqa: E402
from golemflavor_amd import llh, nested, sens  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.enums import ParamTag, Texture  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402

BF = (1 / 3, 1 / 3, 1 / 3)


def timed(model, run, repeats):
    ev = [model.event() for _ in range(2)]
    ts = []
    for _ in range(repeats + 1):
        ev[0].record()
        run()
        ev[1].record()
        model.sync()
        ts.append(ev[0].elapsed_ms(ev[1]))
    return {"median_ms": float(np.median(ts[1:])), "min_ms": float(min(ts[1:])), "max_ms": float(max(ts[1:]))}


def bulk(width, n, nside, smearing, repeats):
    ps = Cf.texture_paramset(6) if width == 7 else Cf.fr_paramsets(6, (0.4444, 0.0))[1]
    desc = compile_model(ps, "BSM_GAUSS", texture=Texture.OET, dimension=6, binning=Cf.default_bin_edges(), source_ratio=(0., 1., 0.),
                         bestfit_fr=BF, smearing=smearing)
    rng = np.random.default_rng(width)
    box = np.array(ps.seeds, dtype=float)
    theta = rng.uniform(box[:, 0], box[:, 1], size=(n, width))
    b = Cf.SCALE_BOUNDARIES[6]
    theta[:, -1] = rng.uniform(b[0], b[0] + 0.6 * (b[1] - b[0]), n)
    theta = np.ascontiguousarray(theta)
    out = {"ndim": width, "rows": n, "nbins": 20}
    with Model(desc) as gauss, Model(desc) as table:
        table.set_table_likelihood(llh.TabulatedLikelihood.from_gaussian(BF, smearing, nside, offset=float(desc.offset)))
        for name, m in (("gaussian", gauss), ("table", table)):
            d_th, d_lp, d_st = m.alloc(theta.nbytes).upload(theta), m.alloc(8 * n), m.alloc(4 * n)
            out[name + "_no_status"] = timed(m, lambda: m.lnprob_device(d_th.ptr, n, d_lp.ptr), repeats)
            out[name + "_with_status"] = timed(m, lambda: m.lnprob_device(d_th.ptr, n, d_lp.ptr, None, d_st.ptr), repeats)
            m.sync()
            out[name + "_rows_finite"] = int(np.isfinite(d_lp.download((n,))).sum())
            for d in (d_th, d_lp, d_st):
                d.free()
    out["table_over_gaussian_no_status"] = out["table_no_status"]["median_ms"] / out["gaussian_no_status"]["median_ms"]
    out["table_over_gaussian_with_status"] = out["table_with_status"]["median_ms"] / out["gaussian_with_status"]["median_ms"]
    return out


def scans(segments, nside, repeats):
    args = sens.parse_args(["--segments", str(segments)])
    scales = nested.sens_scales(args.dimension, args.segments)
    asimov, ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    table = llh.TabulatedLikelihood.from_gaussian(bf, args.smearing, nside, offset=-320.0)
    out = {"segments": segments, "nlive": args.mn_live_points, "nside": nside}
    for name, kw in (("gaussian", {}), ("table", {"table": table})):
        secs, evals = [], []
        for _ in range(repeats + 1):
            res = nested.evidence_scan(args, asimov, ps, scales, run_ids=np.arange(len(scales)), on_nonunitary="-inf", **kw)
            secs.append(res["seconds"])
            evals.append(int(res["nevals"].sum()))
        out[name] = {"median_s": float(np.median(secs[1:])), "min_s": float(min(secs[1:])), "max_s": float(max(secs[1:])), "nevals": evals[-1],
                     "evals_per_s": evals[-1] / float(np.median(secs[1:])), "lnz": res["lnz"].tolist()}
    out["table_over_gaussian_s_per_eval"] = (out["table"]["median_s"] / out["table"]["nevals"]) / (out["gaussian"]["median_s"] / out["gaussian"]["nevals"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512 * 1000)
    ap.add_argument("--nside", type=int, default=512)
    ap.add_argument("--smearing", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--scan-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = {"tool": "bench_table_llh", "nside": a.nside, "repeats": a.repeats,
           "bulk": [bulk(w, a.rows, a.nside, a.smearing, a.repeats) for w in (7, 12)],
           "scan": scans(a.segments, a.nside, a.scan_repeats)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
