"""Time the credible regions of a grid scan's chains (plot.flavor_contour's reduction, golemflavor/plot.py:365-392) two ways, for
the C4 shape -- 64 chains x 2048 walkers x 200 stored steps -- at 126 bins per axis (nbins 25, oversample 5), coverages 90 and
99, hist_smooth 0.05 (nothing smoothed, the reference's default) and 0.6 (radius 2):

  (a) host:   sampler.postprocess(nbins=126) -- the counts of every chain cross PCIe -- then the reference's lines in numpy /
              scipy, one chain per task on at most 16 threads;
  (b) device: sampler.regions(...) -- only the regions come back.

(a) and (b) alternate within one process, after one warm-up each; both are synchronous, so the host clock around them includes
the device's work.  One JSON line with the median and the spread of each and their ratio; --out also writes it to a file
(profiles/regions/).  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_regions.py
--repeats 1 --skip-host` run."""
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
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


def host_region(counts, coverage, sigma):
    """plot.py:371-383 on one chain's counts"""
    from scipy.ndimage import gaussian_filter
    H = counts.astype(np.float64)
    H = H / np.sum(H)
    H_s = gaussian_filter(H, sigma=sigma)
    H_r = np.ravel(H_s)
    H_rs = np.argsort(H_r)[::-1]
    H_crs = np.cumsum(H_r[H_rs])
    return [int(np.searchsorted(H_crs, c / 100.)) for c in coverage]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchains", type=int, default=64)
    ap.add_argument("--nwalkers", type=int, default=2048)
    ap.add_argument("--nsteps", type=int, default=200)
    ap.add_argument("--nbins", type=int, default=25)
    ap.add_argument("--oversample", type=float, default=5.)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    coverage = [90., 99.]
    nb = int(a.nbins * a.oversample) + 1
    ps = Cf.unitary_paramset()
    m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    np.random.seed(3)
    p0 = np.stack([mcmc_utils.flat_seed(ps, a.nwalkers) for _ in range(a.nchains)])
    s = mcmc_utils.DeviceEnsembleSampler(a.nwalkers, 4, m, nchains=a.nchains, seed=5)
    s.run_mcmc(p0, a.nsteps)
    pool = ThreadPoolExecutor(min(a.threads, 16))
    out = {"tool": "bench_regions", "nchains": a.nchains, "nwalkers": a.nwalkers, "nsteps": a.nsteps, "bins_per_axis": nb,
           "coverage": coverage, "host_threads": min(a.threads, 16), "repeats": a.repeats, "cases": []}
    for sigma in (0.05, 0.6):
        t_host, t_dev, thres_host, thres_dev = [], [], None, None
        for rep in range(a.repeats + 1):                   # the first round is a warm-up (code objects, allocations, page maps)
            if not a.skip_host:
                t0 = time.perf_counter()
                hist = s.postprocess(want_fr=False, nbins=nb)["hist"].reshape(a.nchains, nb, nb, nb)
                thres_host = list(pool.map(lambda c: host_region(c, coverage, sigma), hist))
                t_host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            res = s.regions(a.nbins, coverage, hist_smooth=sigma, oversample=a.oversample)
            t_dev.append(time.perf_counter() - t0)
            res = [res] if a.nchains == 1 else res
            thres_dev = [[r.thres for r in row] for row in res]
        case = {"hist_smooth": sigma, "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
                "thres_chain0": thres_dev[0]}
        if not a.skip_host:
            case["host_s"] = {"median": float(np.median(t_host[1:])), "min": min(t_host[1:]), "max": max(t_host[1:])}
            case["host_over_device"] = case["host_s"]["median"] / case["device_s"]["median"]
            case["thres_equal"] = thres_host == thres_dev
        out["cases"].append(case)
    pool.shutdown()
    s.close()
    m.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
