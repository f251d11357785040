"""Time the fused energy-resolved likelihood kernel (k_bsm_binned, csrc/gf_binned.hip) against the two-step path it replaces and
against the flux-averaged lnprob of the same rows, at C5's shape: the 12-column BSM posterior of a grid point of the sens scan,
512 walkers x 1000 steps = 512 000 rows, 20 energy bins.

  fused           Model.lnprob_device of the model with a binned measurement, no status array (k_bsm_binned alone), and with one
                  (the propagate launch for the verdict first: a second pass over the bins);
  two-step        Model.propagate_bins_device into the [n][K][3] slab (device events: the first step alone, a lower bound of the
                  path), then the slab brought to the host and reduced there with numpy (host clock around both steps);
  flux-averaged   Model.lnprob_device of the same model without the measurement, with and without a status array.

Device figures are medians of --repeats launches between two events on the model's stream after one warm-up.  One JSON line;
--out also appends it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from golemflavor_amd import llh, scan  # noqa: E402
from golemflavor_amd import spectrum as sp  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


def timed(model, run, repeats):
    ev = [model.event() for _ in range(2)]
    ts = []
    for _ in range(repeats + 1):
        ev[0].record()
        run()
        ev[1].record()
        model.sync()
        ts.append(ev[0].elapsed_ms(ev[1]))
    return {"median_ms": float(np.median(ts[1:])), "min_ms": float(min(ts[1:])), "max_ms": float(max(ts[1:]))}


def host_reduction(slab, meas, offset):
    """the second step on the host: sum_k fma-free logpdf_k of the slab (values above the underflow wall), vectorised"""
    d = slab - meas.fr_bins[None]
    r2 = np.einsum("nkc,nkc->nk", d, d)
    k = -0.5 * (3 * np.log(2 * np.pi) + 6 * np.log(meas.sigma))
    return np.sum(k[None] - r2 / (2 * meas.sigma[None] ** 2), axis=1) + offset


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512 * 1000)
    ap.add_argument("--point", type=int, default=100, help="grid point of the sens scan whose model is evaluated")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    job = scan._SensPoint(scan.sens_grid()[a.point], a.point, nwalkers=512, device=0)
    flux = job.f.model
    twin = Model(flux.desc, device=0)
    try:
        edges = sp.model_edges(flux)
        K, n, ndim = flux.nbins, int(a.rows), flux.ndim
        meas = llh.BinnedMeasurement.constant([flux.desc.bestfit_fr[i] for i in range(3)], float(flux.desc.smearing), edges)
        twin.set_binned_measurement(meas)
        rng = np.random.default_rng(25)
        idx = rng.integers(0, job.p0.shape[0], n)
        theta = np.ascontiguousarray(job.p0[idx] * (1.0 + 1e-3 * rng.standard_normal((n, ndim))))      # around the point's seeds
        lo, hi = np.asarray(flux.desc.lo)[:ndim], np.asarray(flux.desc.hi)[:ndim]
        theta = np.clip(theta, lo, hi)
        d_th = flux.alloc(theta.nbytes).upload(theta)
        d_lp, d_st, d_slab = flux.alloc(8 * n), flux.alloc(4 * n), flux.alloc(24 * K * n)
        d_th2 = twin.alloc(theta.nbytes).upload(theta)
        d_lp2, d_st2 = twin.alloc(8 * n), twin.alloc(4 * n)
        out = {"tool": "bench_binned_llh", "rows": n, "ndim": ndim, "nbins": K, "repeats": a.repeats, "slab_bytes": 24 * K * n}
        out["fused_no_status"] = timed(twin, lambda: twin.lnprob_device(d_th2.ptr, n, d_lp2.ptr), a.repeats)
        out["fused_with_status"] = timed(twin, lambda: twin.lnprob_device(d_th2.ptr, n, d_lp2.ptr, None, d_st2.ptr), a.repeats)
        out["flux_averaged_no_status"] = timed(flux, lambda: flux.lnprob_device(d_th.ptr, n, d_lp.ptr), a.repeats)
        out["flux_averaged_with_status"] = timed(flux, lambda: flux.lnprob_device(d_th.ptr, n, d_lp.ptr, None, d_st.ptr), a.repeats)
        out["two_step_slab_kernel"] = timed(flux, lambda: flux.propagate_bins_device(d_th.ptr, n, d_slab.ptr, None), a.repeats)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            flux.propagate_bins_device(d_th.ptr, n, d_slab.ptr, None)
            slab = d_slab.download((n, K, 3))
            two = host_reduction(slab, meas, float(flux.desc.offset))
            ts.append(time.perf_counter() - t0)
        out["two_step_with_host_reduction_s"] = float(np.median(ts[1:]))
        twin.lnprob_device(d_th2.ptr, n, d_lp2.ptr)
        twin.sync()
        fused = d_lp2.download((n,))
        # the host reduction carries no prior: the fused values are compared with it through the flux-averaged model's prior-only part
        out["rows_finite"] = int(np.isfinite(fused).sum())
        out["host_reduction_rows_finite"] = int(np.isfinite(two).sum())
        out["fused_over_flux_averaged"] = out["fused_no_status"]["median_ms"] / out["flux_averaged_no_status"]["median_ms"]
        out["fused_over_slab_kernel"] = out["fused_no_status"]["median_ms"] / out["two_step_slab_kernel"]["median_ms"]
    finally:
        twin.close()
        job.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
