"""Time the convergence diagnostics of a scan's chains (golemflavor_amd.diagnostics: c = 5, every lag) two ways, for one shape per
process:

  --shape C4   64 chains x 2048 walkers x 1000 stored steps x 7 columns
  --shape C5   256 chains x 512 walkers x 1000 stored steps x 12 columns, the reference's length

  (a) host:   sampler.flat_steps() -- the chain crosses PCIe, what the parent of this feature offers -- then the same definitions in
              numpy (per-walker autocovariance by FFT, walker-averaged, Sokal's window; the ensemble-mean series; split R-hat), one
              chain per task on at most 16 threads;
  (b) device: sampler.diagnostics() -- only the results come back.

The chains are PRIOR_ONLY posteriors of the right width (the reduction does not depend on what was sampled).  Both ways are
synchronous, so the host clock around them includes the device's work; one warm-up each.  One JSON line; --out also writes it.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_diagnostics.py --repeats 1
--skip-host` run."""
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
from golemflavor_amd import diagnostics as dg  # noqa: E402
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


def host_diagnostics(x, c=5):
    """the definitions on one chain (n, nwalkers, ndim) in numpy; the autocovariances through the FFT"""
    n, nw, nd = x.shape
    size = 1 << (2 * n - 1).bit_length()
    y = x - x.mean(axis=0)
    f = np.fft.rfft(y, n=size, axis=0)
    acf = np.fft.irfft(f * np.conjugate(f), axis=0)[:n]
    ok = acf[0] > 0
    rho = np.where(ok, acf / np.where(ok, acf[0], 1.0), 0.0).sum(axis=1) / ok.sum(axis=0)
    tau = np.empty(nd)
    for d in range(nd):
        taus = 2.0 * np.cumsum(rho[:, d]) - 1.0
        tau[d] = taus[dg.sokal_window(taus, c)]
    tau_mean = mcmc_utils.integrated_time(x.mean(axis=1), c=c, tol=0)
    h = n // 2
    seq = np.concatenate([x[:h], x[n - h:]], axis=1)
    W = seq.var(axis=0, ddof=1).mean(axis=0)
    bh = seq.mean(axis=0).var(axis=0, ddof=1)
    return tau, tau_mean, np.sqrt(((h - 1) / h * W + bh) / W)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["C4", "C5"], default="C4")
    ap.add_argument("--nchains", type=int, default=None)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
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
    t_host, t_dev, tau_host, res = [], [], None, None
    for rep in range(a.repeats + 1):                       # the first round is a warm-up (code objects, allocations, page maps)
        if not a.skip_host:
            t0 = time.perf_counter()
            x = s.flat_steps().reshape(nchains, a.nsteps, nw, ndim)
            tau_host = np.array([r[0] for r in pool.map(host_diagnostics, x)])
            t_host.append(time.perf_counter() - t0)
            del x
        t0 = time.perf_counter()
        res = s.diagnostics()
        t_dev.append(time.perf_counter() - t0)
    res = [res] if nchains == 1 else res
    out = {"tool": "bench_diagnostics", "shape": a.shape, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps, "ndim": ndim,
           "chain_bytes": 8 * ndim * nchains * nw * a.nsteps, "host_threads": min(a.threads, 16), "repeats": a.repeats,
           "products": nchains * nw * ndim * a.nsteps * (a.nsteps + 1) // 2,
           "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
           "not_converged_50": int(sum(not r.converged(50) for r in res))}
    if not a.skip_host:
        out["host_s"] = {"median": float(np.median(t_host[1:])), "min": min(t_host[1:]), "max": max(t_host[1:])}
        out["host_over_device"] = out["host_s"]["median"] / out["device_s"]["median"]
        out["tau_max_abs_diff"] = float(np.abs(tau_host - np.array([r.tau for r in res])).max())
    pool.shutdown()
    s.close()
    m.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
