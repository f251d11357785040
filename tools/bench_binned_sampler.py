"""The C5-shaped stacked sampler (256 grid points x 512 walkers, 12 columns) under the energy-resolved likelihood:

1. us per half-step of the energy-resolved sampler (gf_sampler_create_binned: the grid kernels at one lane per walker) against the
   flux-averaged sampler on the same start positions, forced to the same shape (GF_SAMPLER_CHAIN=0 GF_SAMPLER_LPW=1) and at its own
   best shape (no override).  HIP events around stored runs of --steps steps after a warm-up, the median of --reps runs.
2. What reweighting would have cost: the Kish effective sample size of `reweight([binned model])` on the flux-averaged chain, per
   grid point, as a fraction of its n rows -- beside the n of the directly sampled chain and its `diagnostics()` ESS (nwalkers n /
   tau, the smallest over the columns).

    python tools/bench_binned_sampler.py [--points 256] [--nwalkers 512] [--burnin 100] [--steps 200] [--reps 5] [--out FILE.jsonl]

One JSON line per measurement; with --out they are appended to the file as well."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import scan  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402

FORCED = {"GF_SAMPLER_CHAIN": "0", "GF_SAMPLER_LPW": "1"}


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed_runs(jobs, order, energy_resolved, env, a):
    """(us per half-step of every timed run, launch shape, the sampler -- its last stored run kept)"""
    old = {k: os.environ.pop(k, None) for k in FORCED}
    os.environ.update(env)
    try:
        smp = mcmc_utils.DeviceEnsembleSampler(a.nwalkers, 12, [j.f for j in jobs], seed=25, stream_ids=order, energy_resolved=energy_resolved)
        smp.on_nonunitary = "-inf"
        smp.run_mcmc(np.stack([j.p0 for j in jobs]), a.burnin, storechain=False)          # burn-in
        smp.reset()
        smp.run_mcmc(None, a.steps)                                                        # warm-up of the stored run: buffers, graph, probe
        model = jobs[0].f.model
        us = []
        for _ in range(a.reps):
            smp.reset()
            e0, e1 = model.event(), model.event()
            e0.record()
            smp.run_async(None, a.steps)
            e1.record()
            smp.wait()
            us.append(1e3 * e0.elapsed_ms(e1) / (2 * a.steps))
        return us, smp.launch_shape(), smp
    finally:
        for k in FORCED:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--nwalkers", type=int, default=512)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 200 or a.reps < 5:
        print("note: fewer than 200 steps or 5 runs: not the protocol profiles/binned_sampler/README.txt records", file=sys.stderr)
    pts = scan.sens_grid()[:a.points]
    order = list(range(len(pts)))
    meas = scan.binned_measurements(argparse.Namespace(binned_smearing=None, binned_measurement=None), sorted({p[0] for p in pts}))
    flux = [scan._SensPoint(p, g, nwalkers=a.nwalkers, device=0) for g, p in enumerate(pts)]
    binned = [scan._SensPoint(p, g, nwalkers=a.nwalkers, device=0, binned=meas[p[0]]) for g, p in enumerate(pts)]
    assert all(np.array_equal(x.p0, y.p0) for x, y in zip(flux, binned))
    head = {"points": len(pts), "walkers": a.nwalkers, "burnin": a.burnin, "steps": a.steps}

    keep = {}
    for name, jobs, er, env in (("energy-resolved", binned, True, {}), ("flux-averaged, same shape (GF_SAMPLER_CHAIN=0 GF_SAMPLER_LPW=1)", flux, False, FORCED),
                                ("flux-averaged, its own shape", flux, False, {})):
        us, shape, smp = timed_runs(jobs, order, er, env, a)
        emit({"measurement": "us_per_half_step", "sampler": name, **head, "runs": [round(x, 3) for x in us], "median": round(float(np.median(us)), 3),
              "launch_shape": shape, "nonunitary_proposals_last_run": smp.nonunitary_proposals}, a.out)
        if name.startswith("energy") or name.endswith("own shape"):
            keep[er] = smp
        else:
            smp.close()

    # the flux-averaged chain reweighted to the binned models, against the chain sampled under them
    fs, bs = keep[False], keep[True]
    targets = [Model(j.f.model.desc, device=0) for j in flux]
    try:
        for t, p in zip(targets, pts):
            t.set_binned_measurement(meas[p[0]])
        summ = fs.reweight([[t] for t in targets], on_nonunitary="-inf").summary()
        ess, n = np.atleast_2d(summ["ess"])[:, 0], np.atleast_1d(summ["n"])
        frac = ess / n
        # why a row has no weight: it was stored at -inf (a start the reference would have raised on and that never moved), it is
        # non-unitary under the target, or the target's lnprob is -inf / NaN there
        counts = {k: (np.atleast_2d(summ[k])[:, 0] if k != "bad_base" else np.atleast_1d(summ[k])) for k in ("bad_base", "nonunitary", "outside")}
        facc = np.atleast_2d(fs.acceptance_fraction).mean(axis=1)
        diag = bs.diagnostics()
        diag = diag if isinstance(diag, list) else [diag]
        dess = np.array([np.nanmin(d.ess) for d in diag])
        nb = bs.nstored * bs.k
        emit({"measurement": "reweight_ess", **head, "rows_per_chain": int(n[0]),
              "kish_ess_over_n": {"min": float(frac.min()), "p10": float(np.percentile(frac, 10)), "median": float(np.median(frac)),
                                  "p90": float(np.percentile(frac, 90)), "max": float(frac.max())},
              "points_with_ess_over_n_below_0.1": int(np.sum(frac < 0.1)), "points_with_ess_over_n_below_0.01": int(np.sum(frac < 0.01)),
              "points_without_a_weighted_row": int(np.sum(ess == 0.0)),
              "rows_without_weight": {k: int(v.sum()) for k, v in counts.items()},
              "direct_chain_rows": int(nb),
              "direct_chain_diagnostics_ess_min_column": {"min": float(np.nanmin(dess)), "median": float(np.nanmedian(dess)), "max": float(np.nanmax(dess))},
              "per_point": [{"g": g, "dim": p[0], "texture": p[1].name, "source_x": round(p[2][0], 4), "logLam": p[3],
                             "kish_ess_over_n": round(float(frac[g]), 5), "direct_ess_min_column": round(float(dess[g]), 1),
                             "flux_chain_acceptance": round(float(facc[g]), 4), **{k: int(v[g]) for k, v in counts.items()}}
                            for g, p in enumerate(pts)]}, a.out)
    finally:
        for t in targets:
            t.close()
        fs.close()
        bs.close()
        for j in flux + binned:
            j.close()


if __name__ == "__main__":
    main()
