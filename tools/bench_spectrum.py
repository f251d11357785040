"""Time the energy-resolved composition of a scan's chains (golemflavor_amd.spectrum), for one shape per process:

  --shape C4   64 chains x 2048 walkers x 1000 stored steps, 6 sampled columns, post-processed with the grid points' BSM models
  --shape C5   256 chains x 512 walkers x 1000 stored steps, the 12-column BSM posterior itself

  device:  sampler.spectrum() -- only the results come back;
  (a) the path it replaces: sampler.postprocess_rows() to the host, Model.propagate_bins of the rows from the host, numpy
      reductions (`spectrum.rows_spectrum_host`), one chain per task on at most 16 threads.  --host-chains limits the chains reduced
      on the host and the figure is scaled to all of them (stated in the output);
  (b) the neighbouring on-device product: sampler.marginals(with_fr=True) of the same sampler;
  kernel:  k_bsm_bins alone on one chain's rows in both layouts (events on the model's stream), its store bandwidth
           24 nbins bytes x rows / time, and its time relative to the values-only propagate (k_bsm<UNI_NONE>) of the same rows.

Everything but the kernel figures is synchronous host-clock time with one warm-up.  One JSON line; --out also appends it."""
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
from golemflavor_amd import spectrum as sp  # noqa: E402
from golemflavor_amd.enums import Texture  # noqa: E402

Q = (5., 16., 50., 84., 95.)


def kernel_times(model, theta, repeats):
    """ms of k_bsm_bins (row-major, bin-major) and of the values-only propagate on the device rows `theta`"""
    n, nb = theta.shape[0], model.nbins
    d_th = model.alloc(theta.nbytes).upload(theta)
    d_out = model.alloc(8 * 3 * nb * n)
    d_fr = model.alloc(8 * 3 * n)
    ev = [model.event() for _ in range(2)]
    out = {}
    try:
        for name, run in (("bins_row_major_ms", lambda: model.propagate_bins_device(d_th.ptr, n, d_out.ptr, None, bin_major=False)),
                          ("bins_bin_major_ms", lambda: model.propagate_bins_device(d_th.ptr, n, d_out.ptr, None, bin_major=True)),
                          ("propagate_values_ms", lambda: model.propagate_device(d_th.ptr, n, d_fr.ptr, None))):
            ts = []
            for _ in range(repeats + 1):
                ev[0].record()
                run()
                ev[1].record()
                ts.append(ev[0].elapsed_ms(ev[1]))
            out[name] = float(np.median(ts[1:]))
    finally:
        for b in (d_th, d_out, d_fr):
            b.free()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["C4", "C5"], default="C4")
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
        models = [j.post_model for j in jobs]
    else:
        pts = scan.sens_grid()
        nchains, nw, ndim = a.nchains or len(pts), 512, 12
        jobs = [scan._SensPoint(p, g, nwalkers=nw, device=0) for g, p in enumerate(pts[:nchains])]
        models = None
    s = mcmc_utils.DeviceEnsembleSampler(nw, ndim, [j.f for j in jobs], seed=25, stream_ids=list(range(nchains)))
    s.on_nonunitary = "-inf"
    s.run_mcmc(np.stack([j.p0 for j in jobs]), a.nsteps)
    eval_models = models if models is not None else [j.f.model for j in jobs]
    nbins, per_chain = eval_models[0].nbins, nw * a.nsteps
    t_dev, t_marg, t_host, res, host = [], [], [], None, None
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter()
        res = s.spectrum(percentiles=Q, bins=50, models=models)
        t_dev.append(time.perf_counter() - t0)
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter()
        s.marginals(with_fr=True, models=models)
        t_marg.append(time.perf_counter() - t0)
    res = [res] if nchains == 1 else res
    out = {"tool": "bench_spectrum", "shape": a.shape, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps, "ndim": ndim, "nbins": nbins,
           "slab_bytes_per_chain": 24 * nbins * per_chain, "repeats": a.repeats,
           "spectrum_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])},
           "marginals_with_fr_s": {"median": float(np.median(t_marg[1:])), "min": min(t_marg[1:]), "max": max(t_marg[1:])},
           "samples_without_composition": int(sum(per_chain - int(r.nvalid[0]) for r in res))}
    if not a.skip_host:
        pool = ThreadPoolExecutor(min(a.threads, 16))
        nhost = min(a.host_chains or nchains, nchains)
        edges = sp.model_edges(eval_models[0])
        for _ in range(2):
            t0 = time.perf_counter()
            rows = s.postprocess_rows(models=models)
            t1 = time.perf_counter()
            frs = [eval_models[ch].propagate_bins(np.ascontiguousarray(rows[ch][:, 3:]))[0] for ch in range(nhost)]
            host = list(pool.map(lambda f: sp.rows_spectrum_host(f, edges, Q, 50), frs))
            t2 = time.perf_counter()
            t_host.append((t1 - t0) + (t2 - t1) * nchains / nhost)
            del rows, frs
        pool.shutdown()
        out.update(host_threads=min(a.threads, 16), host_chains_timed=nhost, host_s_scaled_to_all_chains=t_host[-1],
                   host_over_device=t_host[-1] / out["spectrum_s"]["median"],
                   counts_and_percentiles_equal_on_timed_chains=bool(all(
                       np.array_equal(host[ch].counts, res[ch].counts) and np.array_equal(host[ch].percentiles, res[ch].percentiles, equal_nan=True)
                       for ch in range(nhost))))
    theta = np.ascontiguousarray(s.flat_steps().reshape(nchains, per_chain, ndim)[0])
    k = kernel_times(eval_models[0], theta, max(a.repeats, 3))
    out["kernel"] = dict(k, rows=per_chain,
                         store_GBps_row_major=24e-9 * nbins * per_chain / (k["bins_row_major_ms"] * 1e-3),
                         store_GBps_bin_major=24e-9 * nbins * per_chain / (k["bins_bin_major_ms"] * 1e-3),
                         bin_major_over_propagate=k["bins_bin_major_ms"] / k["propagate_values_ms"])
    s.close()
    for j in jobs:
        j.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
