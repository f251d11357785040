"""Time the shortest intervals around the mode of a scan's chains (golemflavor_amd.intervals: percentiles 68 and 90, every column)
two ways, for one shape per process:

  --shape C4   64 chains x 2048 walkers x 1000 stored steps x 7 columns
  --shape C5   256 chains x 512 walkers x 1000 stored steps x 12 columns, the reference's length

  (a) host:   sampler.flat_steps() -- the chain crosses PCIe, what the parent of this feature offers -- then
              `intervals.interval_host` (np.sort, the histogram by searchsorted, the walk as a Python loop) per column and percentile,
              one chain per task on at most 16 threads.  The walk is a Python loop, so the threads share the interpreter; --host-chains
              limits the chains timed on the host and the figure is scaled to all of them (stated in the output);
  (b) device: sampler.intervals() -- only the results come back.

The chains are PRIOR_ONLY posteriors of the right width (the reduction does not depend on what was sampled).  Both ways are
synchronous, so the host clock around them includes the device's work; one warm-up each.  One JSON line; --out also writes it.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_intervals.py --repeats 1 --skip-host`
run."""
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

from golemflavor_amd import configs as Cf  # noqa: E402
from golemflavor_amd import intervals as iv  # noqa: E402
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402

PCT = (68., 90.)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["C4", "C5"], default="C4")
    ap.add_argument("--nchains", type=int, default=None)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-chains", type=int, default=None, help="chains timed on the host (default: all)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    np.random.seed(3)
    if a.shape == "C5":
        nchains, nw, ndim = a.nchains or 256, 512, 12
        ps = Cf.fr_paramsets(6, (0.5, 0.5, 0.5, 0.5))[1]
    else:
        nchains, nw, ndim = a.nchains or 64, 2048, 7
        ps = Cf.texture_paramset(6)
    m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=(1., 0., 0.), flat_llh=1.0))
    p0 = np.stack([mcmc_utils.flat_seed(ps, nw) for _ in range(nchains)])
    s = mcmc_utils.DeviceEnsembleSampler(nw, ndim, m, nchains=nchains, seed=5)
    s.run_mcmc(p0, a.nsteps)
    pool = ThreadPoolExecutor(min(a.threads, 16))
    nhost = min(a.host_chains or nchains, nchains)
    t_host, t_dev, host, res = [], [], None, None
    for rep in range(a.repeats + 1):                       # the first round is a warm-up (code objects, allocations, page maps)
        t0 = time.perf_counter()
        res = s.intervals(percentiles=PCT)
        t_dev.append(time.perf_counter() - t0)
    if not a.skip_host:
        for rep in range(2):                               # the chains all cross PCIe; nhost of them are reduced
            t0 = time.perf_counter()
            x = s.flat_steps().reshape(nchains, a.nsteps * nw, ndim)
            t1 = time.perf_counter()
            host = list(pool.map(lambda rows: iv.rows_intervals_host(rows, PCT), x[:nhost]))
            t2 = time.perf_counter()
            t_host.append((t1 - t0) + (t2 - t1) * nchains / nhost)
            del x
    res = {k: (v[None] if nchains == 1 and k != "percentiles" else v) for k, v in res.items()}
    out = {"tool": "bench_intervals", "shape": a.shape, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps, "ndim": ndim,
           "chain_bytes": 8 * ndim * nchains * nw * a.nsteps, "percentiles": list(PCT), "repeats": a.repeats,
           "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
           "status_not_ok": int(np.count_nonzero(res["status"])), "nunique_min": int(res["nunique"].min())}
    if not a.skip_host:
        out["host_threads"], out["host_chains_timed"] = min(a.threads, 16), nhost
        out["host_s_scaled_to_all_chains"] = t_host[-1]
        out["host_over_device"] = t_host[-1] / out["device_s"]["median"]
        out["equal_on_timed_chains"] = bool(all(iv_equal(host[ch], {k: res[k][ch] for k in iv.FIELDS}) for ch in range(nhost)))
    pool.shutdown()
    s.close()
    m.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def iv_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in iv.FIELDS)


if __name__ == "__main__":
    main()
