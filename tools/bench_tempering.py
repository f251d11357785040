"""The tempered ensemble sampler on the 12-column sens posterior:

1. us per step of an ngroups x ntemps tempered run (--groups scales as groups, geometric_ladder(--temperatures, --beta-min)) with
   swap_every 0 and 8, beside the untempered multi-model sampler with the same number of chains and walkers in the grid shape
   (GF_SAMPLER_CHAIN=0) -- the measurement a tree without the tempered sampler can run too (--untempered-only).  Wall-clock seconds
   around synchronous stored runs of --steps steps after a warm-up run; the --reps runs and their median.  Nothing is gated.
2. ln Z of --scales scales by `tempering.evidence_scan_tempered` beside `nested.evidence_scan`, both error bars (--compare).

--likelihood binned | table: both under the energy-resolved likelihood (a measurement per energy bin at the equal-information widths of
--smearing, around the injected composition) or the tabulated one (the Gaussian of --smearing tabulated at side 64) instead of the
flux-averaged Gaussian; every line names the likelihood.

    python tools/bench_tempering.py [--groups 5] [--temperatures 8] [--beta-min 1e-3] [--nwalkers 256] [--steps 200] [--reps 5]
                                    [--smearing 0.1] [--untempered-only] [--compare] [--scales 5] [--out FILE.jsonl]
                                    [--likelihood flux|binned|table]

One JSON line per measurement; with --out they are appended to the file as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golemflavor_amd import configs as Cf  # noqa: E402
from golemflavor_amd import fr as fr_utils  # noqa: E402
from golemflavor_amd import llh  # noqa: E402
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import nested  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.enums import ParamTag, Texture  # noqa: E402


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def sens_args(a):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=Texture.OET, binning=Cf.default_bin_edges(),
                              smearing=a.smearing, seed=25)


def likelihood(a):
    """(the sampler's keywords, evidence_scan's keywords) of --likelihood"""
    asimov, _ = Cf.sens_paramsets(6, (1., 1., 1.))
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    if a.likelihood == "binned":
        edges = Cf.default_bin_edges()
        return dict(energy_resolved=True), dict(binned=llh.BinnedMeasurement(np.tile(np.asarray(bf, dtype=float), (len(edges) - 1, 1)), a.smearing,
                                                                             binning=edges))
    if a.likelihood == "table":
        return dict(tabulated=True), dict(table=llh.TabulatedLikelihood.from_gaussian(bf, a.smearing, 64))
    return {}, {}


def scale_posteriors(a, scales):
    """one 11-column posterior per scale (the scale fixed), as evidence_scan_tempered builds them"""
    asimov, llh_ps = Cf.sens_paramsets(6, (1., 1., 1.))
    ps = llh_ps.from_tag(ParamTag.SCALE, invert=True)
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    args = sens_args(a)
    fns = [llh.LnProb(compile_model(ps, "BSM_GAUSS", bestfit_fr=bf, smearing=a.smearing, source_ratio=args.source_ratio, texture=args.texture,
                                    dimension=6, binning=args.binning, scale_fixed=float(sc)), on_nonunitary="-inf") for sc in scales]
    scan_kw = likelihood(a)[1]
    for f in fns:
        if "binned" in scan_kw:
            f.model.set_binned_measurement(scan_kw["binned"])
        if "table" in scan_kw:
            f.model.set_table_likelihood(scan_kw["table"])
    return fns, ps


def timed(smp, p0, a):
    smp.run_mcmc(p0, a.steps, storechain=False)                        # burn-in
    smp.reset()
    smp.run_mcmc(None, a.steps)                                        # warm-up of the stored run: buffers, graph
    us = []
    for _ in range(a.reps):
        smp.reset()
        t0 = time.perf_counter()
        smp.run_mcmc(None, a.steps)
        us.append(1e6 * (time.perf_counter() - t0) / a.steps)
    return us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--temperatures", type=int, default=8)
    ap.add_argument("--beta-min", type=float, default=1e-3)
    ap.add_argument("--nwalkers", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--smearing", type=float, default=0.1)
    ap.add_argument("--untempered-only", action="store_true")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--likelihood", choices=["flux", "binned", "table"], default="flux")
    a = ap.parse_args(argv)
    smp_kw, scan_kw = likelihood(a)
    b = Cf.SCALE_BOUNDARIES[6]
    scales = np.linspace(b[0], b[1], a.groups)
    fns, ps = scale_posteriors(a, scales)
    ndim = len(ps)
    try:
        if not a.untempered_only:
            from golemflavor_amd import tempering
            betas = tempering.geometric_ladder(a.temperatures, a.beta_min)
            nchains = a.groups * len(betas)
            rng = np.random.default_rng(1)
            p0 = tempering.prior_draws(ps, nchains * a.nwalkers, rng).reshape(nchains, a.nwalkers, ndim)
            for swap_every in (0, 8):
                smp = mcmc_utils.DeviceEnsembleSampler(a.nwalkers, ndim, fns, seed=25, betas=betas, swap_every=swap_every, ngroups=a.groups, **smp_kw)
                us = timed(smp, p0, a)
                emit({"what": "tempered", "likelihood": a.likelihood, "chains": nchains, "groups": a.groups, "rungs": len(betas), "nwalkers": a.nwalkers, "swap_every": swap_every,
                      "steps": a.steps, "us_per_step": [round(u, 2) for u in us], "median_us_per_step": round(float(np.median(us)), 2),
                      "lanes_per_walker": smp.launch_shape()["lanes_per_walker"],
                      "swap_fraction_min": None if not swap_every else round(float(np.nanmin(smp.swap_fraction)), 3)}, a.out)
                smp.close()
        else:
            nchains = a.groups * (a.temperatures + 1)
            box = np.array(ps.ranges, dtype=float)
            p0 = np.random.default_rng(1).uniform(box[:, 0], box[:, 1], size=(nchains, a.nwalkers, ndim))
        old = os.environ.get("GF_SAMPLER_CHAIN")
        os.environ["GF_SAMPLER_CHAIN"] = "0"
        try:
            smp = mcmc_utils.DeviceEnsembleSampler(a.nwalkers, ndim, [fns[ch % a.groups] for ch in range(nchains)], seed=25, **smp_kw)
            us = timed(smp, p0, a)
            emit({"what": "untempered multi-model sampler, grid shape", "likelihood": a.likelihood, "chains": nchains, "nwalkers": a.nwalkers, "steps": a.steps,
                  "us_per_step": [round(u, 2) for u in us], "median_us_per_step": round(float(np.median(us)), 2),
                  "lanes_per_walker": smp.launch_shape()["lanes_per_walker"]}, a.out)
            smp.close()
        finally:
            os.environ.pop("GF_SAMPLER_CHAIN", None)
            if old is not None:
                os.environ["GF_SAMPLER_CHAIN"] = old
    finally:
        for f in fns:
            f.close()
    if a.compare and not a.untempered_only:
        from golemflavor_amd import tempering
        asimov, llh_ps = Cf.sens_paramsets(6, (1., 1., 1.))
        args = sens_args(a)
        sc = np.linspace(b[0], b[1], a.scales)
        ss = tempering.evidence_scan_tempered(args, asimov, llh_ps, sc, ntemps=a.temperatures, beta_min=a.beta_min, nwalkers=a.nwalkers,
                                              on_nonunitary="-inf", smearing=a.smearing, seed=25, **scan_kw)
        ns = nested.evidence_scan(args, asimov, llh_ps, sc, on_nonunitary="-inf", smearing=a.smearing, seed=25, **scan_kw)
        emit({"what": "ln Z per scale, stepping-stone beside the nested sampler", "likelihood": a.likelihood, "smearing": a.smearing, "scales": sc.tolist(),
              "ln_z_stepping_stone": ss["ln_z"].tolist(), "ln_z_err_stepping_stone": ss["ln_z_err"].tolist(),
              "lnz_nested": ns["lnz"].tolist(), "lnz_err_nested": ns["lnz_err"].tolist(),
              "difference": (ss["ln_z"] - ns["lnz"]).tolist(),
              "difference_in_sigma": ((ss["ln_z"] - ns["lnz"]) / np.sqrt(ss["ln_z_err"] ** 2 + ns["lnz_err"] ** 2)).tolist(),
              "swap_fraction_min": float(np.nanmin(ss["swap_fraction"])), "nonunitary_stepping_stone": int(ss["nonunitary"]),
              "nonunitary_nested": np.asarray(ns["nonunitary"]).tolist(), "start_ess_min": float(ss["start_ess"].min()),
              "seconds_stepping_stone": round(ss["seconds"], 3), "seconds_nested": round(ns["seconds"], 3)}, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
