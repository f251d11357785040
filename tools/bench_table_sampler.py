"""The C5-shaped stacked sampler (256 grid points x 512 walkers, 12 columns) under a tabulated flavour-plane likelihood:

1. us per half-step of the table sampler (gf_sampler_create_table: the grid kernels) at the lane count its rule gives and at
   GF_SAMPLER_LPW=1, beside the flux-averaged sampler on the same start positions in the grid shape (GF_SAMPLER_CHAIN=0) at the same
   two settings.  The table is `TabulatedLikelihood.from_gaussian` of the scan's own measurement and width, side --nside.  HIP events
   around stored runs of --steps steps after a warm-up run; the --reps runs and their median.
2. What reweighting would have cost: the Kish effective sample size of `reweight([table model])` on the flux-averaged chain, per
   grid point, as a fraction of its n rows -- beside the n of the directly sampled chain and its `diagnostics()` ESS (nwalkers n /
   tau, the smallest over the columns).

    python tools/bench_table_sampler.py [--points 256] [--nwalkers 512] [--burnin 100] [--steps 200] [--reps 5] [--nside 512]
                                        [--flux-only] [--out FILE.jsonl]

--flux-only: the two flux-averaged measurements alone (what a tree without the table sampler can run).  One JSON line per
measurement; with --out they are appended to the file as well."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golemflavor_amd import fr as fr_utils  # noqa: E402
from golemflavor_amd import llh  # noqa: E402
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import scan  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402

OVERRIDES = ("GF_SAMPLER_CHAIN", "GF_SAMPLER_LPW")
GRID = {"GF_SAMPLER_CHAIN": "0"}
GRID_ONE_LANE = {"GF_SAMPLER_CHAIN": "0", "GF_SAMPLER_LPW": "1"}


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed_runs(jobs, order, tabulated, env, a):
    """(us per half-step of every timed run, launch shape, the sampler -- its last stored run kept)"""
    old = {k: os.environ.pop(k, None) for k in OVERRIDES}
    os.environ.update(env)
    try:
        kw = {"tabulated": True} if tabulated else {}
        smp = mcmc_utils.DeviceEnsembleSampler(a.nwalkers, 12, [j.f for j in jobs], seed=25, stream_ids=order, **kw)
        smp.on_nonunitary = "-inf"
        smp.run_mcmc(np.stack([j.p0 for j in jobs]), a.burnin, storechain=False)          # burn-in
        smp.reset()
        smp.run_mcmc(None, a.steps)                                                        # warm-up of the stored run: buffers, graph
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
        for k in OVERRIDES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def gaussian_tables(dims, nside):
    """{dimension: the scan's Gaussian measurement of that dimension as a table of side nside}"""
    out = {}
    for dim in dims:
        asimov = scan._SensPoint.asimov(dim, scan.C5_SMEARING)
        bf = fr_utils.angles_to_fr(asimov.from_tag(llh.ParamTag.BESTFIT, values=True))
        out[dim] = llh.TabulatedLikelihood.from_gaussian(bf, scan.C5_SMEARING, nside)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--nwalkers", type=int, default=512)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nside", type=int, default=512)
    ap.add_argument("--flux-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 200 or a.reps < 5:
        print("note: fewer than 200 steps or 5 runs: not the protocol profiles/table_sampler/README.txt records", file=sys.stderr)
    pts = scan.sens_grid()[:a.points]
    order = list(range(len(pts)))
    flux = [scan._SensPoint(p, g, nwalkers=a.nwalkers, device=0) for g, p in enumerate(pts)]
    head = {"points": len(pts), "walkers": a.nwalkers, "burnin": a.burnin, "steps": a.steps}
    runs = [("flux-averaged, grid, the rule's lanes (GF_SAMPLER_CHAIN=0)", flux, False, GRID),
            ("flux-averaged, grid, one lane (GF_SAMPLER_CHAIN=0 GF_SAMPLER_LPW=1)", flux, False, GRID_ONE_LANE)]
    tabled, tables = [], {}
    if not a.flux_only:
        tables = gaussian_tables(sorted({p[0] for p in pts}), a.nside)
        tabled = [scan._SensPoint(p, g, nwalkers=a.nwalkers, device=0, table=tables[p[0]]) for g, p in enumerate(pts)]
        assert all(np.array_equal(x.p0, y.p0) for x, y in zip(flux, tabled))
        head["nside"] = a.nside
        runs = [("tabulated, the rule's lanes", tabled, True, {}), runs[0], ("tabulated, one lane (GF_SAMPLER_LPW=1)", tabled, True, {"GF_SAMPLER_LPW": "1"}),
                runs[1]]

    keep = {}
    try:
        for name, jobs, tab, env in runs:
            us, shape, smp = timed_runs(jobs, order, tab, env, a)
            emit({"measurement": "us_per_half_step", "sampler": name, **head, "runs": [round(x, 3) for x in us], "median": round(float(np.median(us)), 3),
                  "min": round(min(us), 3), "max": round(max(us), 3), "launch_shape": shape,
                  "nonunitary_proposals_last_run": smp.nonunitary_proposals}, a.out)
            if "one lane" in name or a.flux_only:
                smp.close()
            else:
                keep[tab] = smp
        if a.flux_only:
            return
        # the flux-averaged chain reweighted to the table models, against the chain sampled under them
        fs, ts = keep[False], keep[True]
        targets = [Model(j.f.model.desc, device=0) for j in flux]
        try:
            for t, p in zip(targets, pts):
                t.set_table_likelihood(tables[p[0]])
            summ = fs.reweight([[t] for t in targets], on_nonunitary="-inf").summary()
            ess, n = np.atleast_2d(summ["ess"])[:, 0], np.atleast_1d(summ["n"])
            frac = ess / n
            diag = ts.diagnostics()
            diag = diag if isinstance(diag, list) else [diag]
            dess = np.array([np.nanmin(d.ess) for d in diag])
            emit({"measurement": "reweight_ess", **head, "rows_per_chain": int(n[0]),
                  "kish_ess_over_n": {"min": float(frac.min()), "p10": float(np.percentile(frac, 10)), "median": float(np.median(frac)),
                                      "p90": float(np.percentile(frac, 90)), "max": float(frac.max())},
                  "points_with_ess_over_n_below_0.1": int(np.sum(frac < 0.1)), "points_without_a_weighted_row": int(np.sum(ess == 0.0)),
                  "direct_chain_rows": int(ts.nstored * ts.k),
                  "direct_chain_diagnostics_ess_min_column": {"min": float(np.nanmin(dess)), "median": float(np.nanmedian(dess)), "max": float(np.nanmax(dess))}},
                 a.out)
        finally:
            for t in targets:
                t.close()
    finally:
        for smp in keep.values():
            smp.close()
        for j in flux + tabled:
            j.close()


if __name__ == "__main__":
    main()
