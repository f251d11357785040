"""Time the marginals of a scan's chains in element space (DeviceEnsembleSampler.marginals(space="elements"): moduli |U_ij| in place
of the mixing columns, plot.chainer_plot's --plot-elements table; plot_Tchain's settings) two ways, for one shape per process:

  --shape C5   256 chains x 512 walkers x 1000 stored steps x 12 columns -> 17 (12.6 GB read, 17.8 GB written)
  --shape C4   64 chains x 2048 walkers x 1000 stored steps x 6 columns -> 11

  (a) host:   sampler.flat_steps() -- the chain crosses PCIe -- then the transform in numpy (the formulas of csrc/gf_elements.hpp,
              vectorised, one chain per task on at most 16 threads; the reference maps a Python function over every row instead),
              then marginals.chain_marginals of the uploaded result;
  (b) device: sampler.marginals(space="elements", llh_paramset=ps) -- only the results come back.

Both ways are synchronous, so the host clock around them includes the device's work; the first round is a warm-up.  One JSON line;
--out also appends it to a file.  `kernel_bytes` is what k_element_rows moves: 8 (width_in + width_out) bytes per row.  The kernel's
own time comes from a separate run, `rocprofv3 --kernel-trace --stats -- python tools/bench_elements.py --repeats 1 --skip-host
--join-rows` (--shape C4): --join-rows also assembles the rows a C4 scan saves once, so that k_join_rows (pure data movement,
8 (3 + 6) bytes read and as many written per row) is in the same trace.  `--stats-csv FILE --calls N` then reads that run's
kernel_stats.csv (no device needed: together with the JSON line of the traced run given by --line) and prints each kernel's achieved
bytes per second: bytes per call from the shape, over the kernel's average duration in the trace."""
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
from golemflavor_amd import elements as el  # noqa: E402
from golemflavor_amd import marginals as mg  # noqa: E402
from golemflavor_amd import mcmc as mcmc_utils  # noqa: E402
from golemflavor_amd import scan  # noqa: E402
from golemflavor_amd.descriptor import compile_model  # noqa: E402
from golemflavor_amd.model import Model  # noqa: E402


def numpy_moduli(a, x, b, d):
    """|U_ij| (n, 9) float32-rounded, the formulas of gf_elements.hpp on whole columns"""
    s12, c12 = np.sqrt(a), np.sqrt(1 - a)
    y = np.sqrt(x)
    c13, s13 = np.sqrt(y), np.sqrt((1 - x) / (1 + y))
    s23, c23 = np.sqrt(b), np.sqrt(1 - b)
    e = np.exp(1j * d)
    u = np.stack([c12 * c13, s12 * c13, s13,
                  np.abs(c23 * s12 + s23 * s13 * c12 * e), np.abs(c23 * c12 - s23 * s13 * s12 * e), s23 * c13,
                  np.abs(s23 * s12 - c23 * s13 * c12 * e), np.abs(s23 * c12 + c23 * s13 * s12 * e), c23 * c13], axis=1)
    return u.astype(np.float32).astype(np.float64)


def numpy_rows(x, groups):
    """one chain's rows (n, width_in) in element space by the plan's groups [(kind, columns)]"""
    cols = []
    for kind, c in groups:
        if kind == el.GF_ELEMENT_U9:
            cols.append(numpy_moduli(x[:, c[0]], x[:, c[1]], x[:, c[2]], x[:, c[3]]))
        elif kind == el.GF_ELEMENT_FR3:
            s2, p2 = np.sqrt(x[:, c[0]]), 0.5 * (1 - x[:, c[1]])
            cols.append(np.abs(np.stack([s2 * (1 - p2), s2 * p2, 1 - s2], axis=1)))
        else:
            cols.append(x[:, c[0]][:, None])
    return np.concatenate(cols, axis=1)


def rates_from_stats(csv_path, line):
    """{kernel: bytes per second} of k_element_rows and k_join_rows from a rocprofv3 kernel_stats.csv (columns Name and
    AverageNs, or TotalDurationNs and Calls) and the JSON line of the traced run"""
    import csv
    per_call = {"k_element_rows<": line["kernel_bytes"], "k_join_rows": line.get("join_rows_bytes")}
    out = {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key, nbytes in per_call.items():
                if key in name and "exact" not in name and nbytes:
                    avg = float(row["AverageNs"]) if row.get("AverageNs") else float(row["TotalDurationNs"]) / float(row["Calls"])
                    out[name] = nbytes / (avg * 1e-9)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats-csv", default=None, help="a traced run's kernel_stats.csv: print the kernels' bytes per second and exit")
    ap.add_argument("--line", default=None, help="with --stats-csv: the file holding the traced run's JSON line (its last line is read)")
    ap.add_argument("--shape", choices=["C4", "C5"], default="C4")
    ap.add_argument("--nchains", type=int, default=None)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--join-rows", action="store_true", help="C4: also assemble the saved rows once (k_join_rows in the trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.stats_csv:
        if not a.line:
            ap.error("--stats-csv needs --line")
        with open(a.line) as f:
            line = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        print(json.dumps({"tool": "bench_elements", "shape": line["shape"], "bytes_per_s": rates_from_stats(a.stats_csv, line)}))
        return
    if a.join_rows and a.shape != "C4":
        ap.error("--join-rows needs --shape C4 (the C5 rows carry no composition to join)")
    np.random.seed(3)
    jobs = []
    if a.shape == "C5":
        nchains, nw, ndim = a.nchains or 256, 512, 12
        ps = Cf.fr_paramsets(6, (0.5, 0.5))[1]
        m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=(1., 0., 0.), flat_llh=1.0))
        fns = m
    else:
        nchains, nw, ndim = a.nchains or 64, 2048, 6
        jobs = [scan._TexturePoint(p, g, dimension=6, texture=scan.Texture.OET, nwalkers=nw, device=0)
                for g, p in enumerate(scan.texture_grid(6)[:nchains])]
        ps, m = jobs[0].ps6, jobs[0].f.model
        fns = [j.f for j in jobs]
    plan, names, ranges = el.element_plan(ps)
    n = {el.GF_ELEMENT_COPY: 1, el.GF_ELEMENT_U9: 4, el.GF_ELEMENT_FR3: 2}
    groups = [(plan.group[g].kind, list(plan.group[g].col[:n[plan.group[g].kind]])) for g in range(plan.ngroups)]
    p0 = np.stack([mcmc_utils.flat_seed(ps, nw) for _ in range(nchains)])
    s = mcmc_utils.DeviceEnsembleSampler(nw, ndim, fns, nchains=nchains, seed=5)
    s.on_nonunitary = "-inf"
    s.run_mcmc(p0, a.nsteps)
    nrows = nchains * nw * a.nsteps
    pool = ThreadPoolExecutor(min(a.threads, 16))
    t_host, t_dev, c_host, c_dev = [], [], None, None
    for rep in range(a.repeats + 1):
        if not a.skip_host:
            t0 = time.perf_counter()
            x = s.flat_steps().reshape(nchains, -1, ndim)
            rows = np.stack(list(pool.map(lambda c: numpy_rows(c, groups), x)))
            res = mg.chain_marginals(rows, ranges, model=m, names=names)
            t_host.append(time.perf_counter() - t0)
            c_host = [r.counts1.sum() for r in res]
            del x, rows
        t0 = time.perf_counter()
        res = s.marginals(space="elements", llh_paramset=ps)
        t_dev.append(time.perf_counter() - t0)
        c_dev = [r.counts1.sum() for r in ([res] if nchains == 1 else res)]
    if a.join_rows and jobs:
        s.postprocess_rows(models=[j.post_model for j in jobs])
    out = {"tool": "bench_elements", "shape": a.shape, "nchains": nchains, "nwalkers": nw, "nsteps": a.nsteps, "width_in": ndim,
           "width_out": len(names), "kernel_bytes": 8 * (ndim + len(names)) * nrows,
           "host_threads": min(a.threads, 16), "repeats": a.repeats,
           "device_s": {"median": float(np.median(t_dev[1:])), "min": min(t_dev[1:]), "max": max(t_dev[1:])}}
    if a.join_rows:
        out["join_rows_bytes"] = 16 * (3 + ndim) * nw * a.nsteps             # per call: one chain's rows
        out["kernel_bytes_note"] = "k_element_rows: one call for all chains; k_join_rows: one call per chain"
    if not a.skip_host:
        out["host_s"] = {"median": float(np.median(t_host[1:])), "min": min(t_host[1:]), "max": max(t_host[1:])}
        out["host_over_device"] = out["host_s"]["median"] / out["device_s"]["median"]
        out["histogram_totals_equal"] = [int(v) for v in c_host] == [int(v) for v in c_dev]
    pool.shutdown()
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
