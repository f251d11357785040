"""Time the posterior marginals of a scan's chains (golemflavor_amd.marginals: 100 / 50 bins, coverages 90 and 99, percentiles 5, 50,
95 -- plot_Tchain's settings, golemflavor/plot.py:456-459) two ways, for one shape per process:

  --shape C5   256 chains x 512 walkers x 1000 stored steps x 12 columns (12.6 GB), the reference's length; --with-fr does not apply
  --shape C4   64 chains x 2048 walkers x 1000 stored steps x 6 columns, and with --with-fr the 9-column rows a scan saves

  (a) host:   sampler.flat_steps() -- the chain crosses PCIe, what the parent of this feature offers -- then the same reduction in
              numpy / scipy (np.histogram, np.histogram2d, np.percentile, mean, np.cov, plot.py:371-383 per marginal), one chain
              per task on at most 16 threads;
  (b) device: sampler.marginals(...) -- only the results come back.

The chains are PRIOR_ONLY posteriors of the right width (the reduction does not depend on what was sampled).  Both ways are
synchronous, so the host clock around them includes the device's work; one warm-up each.  One JSON line; --out also writes it.
`hbm_row_passes` is the number of times the device path reads the rows from memory as launched: 1 (histograms; the other pair
groups of a slab follow it through L2) + 1 (sums) + 1 (centred products; the other columns through L2) + 8 (select passes).
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_marginals.py --repeats 1
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
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import scan  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, the device-to-device copy rate measured on an MI355X
HBM_ROW_PASSES = 11


def host_marginals(x, ranges, nb1=100, nb2=50, coverage=(90., 99.), q=(5., 50., 95.)):
    """the reduction on one chain's rows in numpy / scipy"""
    from scipy.ndimage import gaussian_filter
    W = x.shape[1]

    def region(H):
        H = H / np.sum(H)
        H_r = np.ravel(gaussian_filter(H, sigma=0.05))
        H_crs = np.cumsum(H_r[np.argsort(H_r)[::-1]])
        return [int(np.searchsorted(H_crs, c / 100.)) for c in coverage]
    out = []
    for c in range(W):
        out.append(region(np.histogram(x[:, c], bins=nb1, range=ranges[c])[0].astype(np.float64)))
    for i in range(W):
        for j in range(i + 1, W):
            out.append(region(np.histogram2d(x[:, i], x[:, j], bins=nb2, range=[ranges[i], ranges[j]])[0]))
    ok = ~np.isnan(x).any(axis=1)
    return out, np.nanpercentile(x, q, axis=0), x[ok].mean(axis=0), np.cov(x[ok], rowvar=False)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["C4", "C5"], default="C4")
    ap.add_argument("--with-fr", action="store_true")
    ap.add_argument("--nchains", type=int, default=None)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    np.random.seed(3)
    models = None
    if a.shape == "C5":
        nchains, nw, ndim = a.nchains or 256, 512, 12
        ps = Cf.fr_paramsets(6, (0.5, 0.5, 0.5, 0.5))[1]
        m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=(1., 0., 0.), flat_llh=1.0))
        fns, with_fr = m, False
    else:
        nchains, nw, ndim = a.nchains or 64, 2048, 6
        with_fr = a.with_fr
        jobs = [scan._TexturePoint(p, g, dimension=6, texture=scan.Texture.OET, nwalkers=nw, device=0)
                for g, p in enumerate(scan.texture_grid(6)[:nchains])]
        ps, m = jobs[0].ps6, jobs[0].f.model
        fns = [j.f for j in jobs]
        models = [j.post_model for j in jobs] if with_fr else None
    p0 = np.stack([mcmc_utils.flat_seed(ps, nw) for _ in range(nchains)])
    s = mcmc_utils.DeviceEnsembleSampler(nw, ndim, fns, nchains=nchains, seed=5)
    s.on_nonunitary = "-inf"
    s.run_mcmc(p0, a.nsteps)
    width = ndim + (3 if with_fr else 0)
    ranges = ([(0., 1.)] * 3 if with_fr else []) + [(m.desc.lo[c], m.desc.hi[c]) for c in range(ndim)]
    row_bytes = 8 * width * nchains * nw * a.nsteps
    pool = ThreadPoolExecutor(min(a.threads, 16))
    t_host, t_dev, thres_host, thres_dev = [], [], None, None
    for rep in range(a.repeats + 1):                       # the first round is a warm-up (code objects, allocations, page maps)
        if not a.skip_host:
            t0 = time.perf_counter()
            rows = s.postprocess_rows(models=models) if with_fr else s.flat_steps()
            rows = rows.reshape(nchains, -1, width)
            thres_host = [r[0] for r in pool.map(lambda x: host_marginals(x, ranges), rows)]
            t_host.append(time.perf_counter() - t0)
            del rows
        t0 = time.perf_counter()
        res = s.marginals(with_fr=with_fr, models=models)
        t_dev.append(time.perf_counter() - t0)
        res = [res] if nchains == 1 else res
        thres_dev = [[[r.thres for r in row] for row in list(x.regions1) + list(x.regions2)] for x in res]
    out = {"tool": "bench_marginals", "shape": a.shape, "with_fr": with_fr, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps,
           "width": width, "row_bytes": row_bytes, "bins": [100, 50], "coverage": [90., 99.], "percentiles": [5., 50., 95.],
           "host_threads": min(a.threads, 16), "repeats": a.repeats, "hbm_row_passes": HBM_ROW_PASSES,
           "floor_s": row_bytes * HBM_ROW_PASSES / COPY_RATE,
           "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])}}
    if not a.skip_host:
        out["host_s"] = {"median": float(np.median(t_host[1:])), "min": min(t_host[1:]), "max": max(t_host[1:])}
        out["host_over_device"] = out["host_s"]["median"] / out["device_s"]["median"]
        out["thres_equal"] = thres_host == thres_dev
    pool.shutdown()
    s.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
