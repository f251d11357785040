"""Time the posterior of an evidence scan's runs (golemflavor_amd.nested: posterior() and marginals() of every run) two ways:

  (a) host:   dead(r) for every run -- the points cross PCIe in three small copies per iteration and run, what the parent of this
              feature offers -- then the same definitions in numpy (weights, Kish ess, np.average, np.cov, np.cumsum, np.searchsorted,
              np.histogram / np.histogram2d of the resampled rows), one run per task on at most 16 threads;
  (b) device: sampler.posterior() and sampler.marginals(nrows) -- only the results come back.

The runs are the sens.py scan's (Cf.sens_paramsets, d = 6, OET, --segments scales).  Both ways are synchronous, so the host clock
around them includes the device's work; one warm-up each.  One JSON line; --out also writes it."""
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
from golemflavor_amd import fr as fr_utils  # noqa: E402
from golemflavor_amd import nested  # noqa: E402
from golemflavor_amd.enums import Texture  # noqa: E402


def host_posterior(d, nrows, u, ranges, bins_1d=100, bins_2d=50):
    """the definitions on one run's dead() arrays in numpy"""
    lnw, theta = d["lnw"], d["theta"]
    with np.errstate(all="ignore"):
        e = np.where(np.isneginf(lnw), 0.0, np.exp(lnw - lnw.max()))
    p = e / e.sum()
    ess = e.sum() ** 2 / (e * e).sum()
    mean = np.average(theta, axis=0, weights=p)
    cov = np.cov(theta.T, aweights=p)
    t = (np.arange(nrows) + u) / nrows
    rows = theta[np.minimum(np.searchsorted(np.cumsum(p), t, side="right"), len(p) - 1)]
    W = rows.shape[1]
    h1 = [np.histogram(rows[:, c], bins_1d, ranges[c])[0] for c in range(W)]
    h2 = [np.histogram2d(rows[:, i], rows[:, j], bins_2d, (ranges[i], ranges[j]))[0] for i in range(W) for j in range(i + 1, W)]
    return ess, mean, cov, h1, h2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--nlive", type=int, default=1000)
    ap.add_argument("--nrows", type=int, default=16384)
    ap.add_argument("--smearing", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    args = argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=Texture.OET, binning=Cf.default_bin_edges(),
                              smearing=a.smearing, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    scales = nested.sens_scales(6, a.segments)
    res = nested.evidence_scan(args, asimov, ps, scales, nlive=a.nlive, seed=3, on_nonunitary="-inf", return_sampler=True)
    s = res["sampler"]
    ranges = [tuple(float(v) for v in p.ranges) for p in ps]
    pool = ThreadPoolExecutor(min(a.threads, 16))
    t_host, t_dev, host, post = [], [], None, None
    for rep in range(a.repeats + 1):                       # the first round is a warm-up
        t0 = time.perf_counter()
        dead = [s.dead(r) for r in range(s.nruns)]
        host = list(pool.map(lambda d: host_posterior(d, a.nrows, 0.5, ranges), dead))
        t_host.append(time.perf_counter() - t0)
        del dead
        t0 = time.perf_counter()
        post = s.posterior()
        s.marginals(a.nrows, ranges=ranges)
        t_dev.append(time.perf_counter() - t0)
    out = {"tool": "bench_nested_posterior", "nruns": s.nruns, "nlive": a.nlive, "nrows": a.nrows, "ndim": len(ps),
           "npoints": post["npoints"].tolist(), "niter": res["niter"].tolist(), "host_threads": min(a.threads, 16), "repeats": a.repeats,
           "host_s": {"median": float(np.median(t_host[1:])), "min": min(t_host[1:]), "max": max(t_host[1:])},
           "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
           "ess_max_rel_diff": float(np.nanmax(np.abs(np.array([h[0] for h in host]) / post["ess"] - 1.0)))}
    out["host_over_device"] = out["host_s"]["median"] / out["device_s"]["median"]
    pool.shutdown()
    s.close()
    for m in res["models"]:
        m.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
