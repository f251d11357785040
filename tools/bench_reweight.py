"""Time the reweighting of a scan's stored chains to other measurements (golemflavor_amd.reweight), for one shape per process:

  --shape C4   64 chains x 2048 walkers x 1000 stored steps, 6 sampled columns.  The C4 scan's own chains sample the priors only and
               carry no measurement to replace, so this shape samples the grid points' BSM posteriors themselves (6 columns, scale and
               source fixed per point, 20 diagonalisations per row)
  --shape C5   256 chains x 512 walkers x 1000 stored steps, the 12-column BSM posterior

  device:   sampler.reweight(8 measurement targets).summary() -- only the summaries come back;
  split:    the propagate step alone (sampler.postprocess_to_device of the same chains into a scratch buffer) and, by difference,
            everything after it (k_rw_gauss, the weight pipeline of 8 targets per chain, the read-back of the summaries);
  host:     the path it replaces: chain_to_host plus lnprobability, the rows' compositions by Model.propagate from the host, then
            `reweight.reweight_host` per (chain, target), one chain per task on at most 16 threads.  --host-chains limits the chains
            reduced on the host and the figure is scaled to all of them (stated in the output).

Synchronous host-clock time with one warm-up.  One JSON line; --out also appends it."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import scan  # noqa: E402
from golemflavor_amd import llh as llh_utils  # noqa: E402
from golemflavor_amd.enums import Texture  # noqa: E402
from golemflavor_amd.reweight import Measurement, reweight_host  # noqa: E402

INJECTED = [(0.30, 0.36, 0.34), (1., 1., 1.), (1., 2., 0.), (0.36, 0.33, 0.31)]
SMEARING = [0.05, 0.02]


def gauss_mg(fr, bf, smearing, offset):
    s = smearing ** 2
    return -0.5 * (3.0 * np.log(2.0 * np.pi) + 3.0 * np.log(s) + ((fr - np.asarray(bf)) ** 2).sum(axis=1) / s) + offset


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["C4", "C5"], default="C5")
    ap.add_argument("--nchains", type=int, default=None)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-chains", type=int, default=None, help="chains reduced on the host (default: all)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.shape == "C4":
        pts = scan.texture_grid(6)
        nchains, nw, ndim = a.nchains or len(pts), 2048, 6
        jobs = [scan._TexturePoint(p, g, dimension=6, texture=Texture.OET, nwalkers=nw, device=0) for g, p in enumerate(pts[:nchains])]
        fns = [llh_utils.LnProb(j.post_model.desc, device=0, on_nonunitary="-inf") for j in jobs]
    else:
        pts = scan.sens_grid()
        nchains, nw, ndim = a.nchains or len(pts), 512, 12
        jobs = [scan._SensPoint(p, g, nwalkers=nw, device=0) for g, p in enumerate(pts[:nchains])]
        fns = [j.f for j in jobs]
    s = mcmc_utils.DeviceEnsembleSampler(nw, ndim, fns, seed=25, stream_ids=list(range(nchains)))
    s.on_nonunitary = "-inf"
    s.run_mcmc(np.stack([j.p0 for j in jobs]), a.nsteps)
    per_chain = nw * a.nsteps
    targets = [Measurement(injected_ratio=f, smearing=sm) for f in INJECTED for sm in SMEARING]
    t_dev, t_prop, t_host, summ = [], [], [], None
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter()
        summ = s.reweight(targets, on_nonunitary="-inf").summary()
        t_dev.append(time.perf_counter() - t0)
    m0 = fns[0].model
    d_fr, d_st = m0.alloc(8 * 3 * per_chain * nchains), m0.alloc(4 * per_chain * nchains)
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter()
        s.postprocess_to_device(d_fr.ptr, d_st.ptr)
        t_prop.append(time.perf_counter() - t0)
    d_fr.free()
    d_st.free()
    med = lambda t: float(np.median(t[1:]))  # noqa: E731
    ess = np.atleast_2d(summ["ess"])
    out = {"tool": "bench_reweight", "shape": a.shape, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps, "ndim": ndim, "ntargets": len(targets),
           "rows_per_chain": per_chain, "repeats": a.repeats,
           "reweight_summary_s": {"median": med(t_dev), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
           "propagate_only_s": {"median": med(t_prop), "min": min(t_prop[1:]), "max": max(t_prop[1:])},
           "after_propagate_s": med(t_dev) - med(t_prop),
           "ess_min_median_max": [float(ess.min()), float(np.median(ess)), float(ess.max())],
           "nonunitary_rows": int(np.sum(summ["nonunitary"])), "outside_rows": int(np.sum(summ["outside"]))}
    if not a.skip_host:
        pool = ThreadPoolExecutor(min(a.threads, 16))
        nhost = min(a.host_chains or nchains, nchains)
        models = [f.model for f in fns]
        for _ in range(2):
            t0 = time.perf_counter()
            rows = s.chain_to_host(np.empty((nchains, a.nsteps, nw, ndim))).reshape(nchains, per_chain, ndim)
            lp = s._fetch(lnprob=True)[1].reshape(nchains, per_chain)
            t1 = time.perf_counter()

            def one(ch):
                fr, st = models[ch].propagate(rows[ch])
                d = models[ch].desc
                base = gauss_mg(fr, [d.bestfit_fr[k] for k in range(3)], d.smearing, d.offset)
                return [reweight_host(rows[ch], base, gauss_mg(fr, t.bestfit_fr, t.smearing, d.offset), status=st)["ess"] for t in targets]
            host = list(pool.map(one, range(nhost)))
            t2 = time.perf_counter()
            t_host.append((t1 - t0) + (t2 - t1) * nchains / nhost)
            del rows, lp
        pool.shutdown()
        out.update(host_threads=min(a.threads, 16), host_chains_timed=nhost, host_readback_s=t1 - t0, host_s_scaled_to_all_chains=t_host[-1],
                   host_over_device=t_host[-1] / out["reweight_summary_s"]["median"],
                   host_ess_relative_difference_max=float(np.max(np.abs(np.array(host) - ess[:nhost]) / np.maximum(ess[:nhost], 1.0))))
    s.close()
    for j in jobs:
        j.close()
    if a.shape == "C4":
        for f in fns:
            f.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
