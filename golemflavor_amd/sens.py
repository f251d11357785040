"""`python -m golemflavor_amd.sens`: scripts/sens.py on the device nested sampler (golemflavor_amd.nested) or, with
--stat-method frequentist, on the device profile-likelihood maximiser (golemflavor_amd.profile_llh).

Same arguments as the reference's driver for what applies here (the likelihood is the package's Gaussian substitute,
README.md:70-74), same scale list ([-100] + linspace over SCALE_BOUNDARIES[d] in segments - 1 steps, sens.py:226-229) and the
same two output arrays, {datadir}/{stat_method}/{data}/fr_stat{identifier}.npy and fr_maxllh{identifier}.npy of shape
(segments, 2) -- (1, 2) with --eval-segment, whose files carry `_scale_{10^scale:.0E}` (sens.py:232-258).  All scales run in
one device call.  Prints one JSON summary line.  --posterior also writes every scale's posterior summary and marginals,
posterior_<identifier>_scale_<10^scale:.0E>.npz beside the arrays (INTEGRATION.md has the layout).  --energy-resolved (or
--binned-measurement FILE.npy, --binned-smearing) fits the composition of every energy bin instead of the flux average; every
file name then carries `_ebins` behind the identifier.  The frequentist arrays hold [scale, profile max lnL] in both files: the
statistic golemflavor/plot.py:605-608 (plot_statistic) receives.  --stat-method frequentist --realisations T also profiles T mock
measurements thrown around the injected composition (with --energy-resolved a throw per energy bin) and
writes fr_realisations{identifier}.npz beside fr_maxllh.
--evidence-realisations T (the Bayesian method) reweights the evidence scan's own points to T such measurements and
writes fr_evidence_realisations{identifier}.npz beside fr_stat; the Asimov arrays are what the command writes without the option.
--evidence-method stepping-stone [--temperatures N --beta-min B --swap-every S --tempered-steps K] gives ln Z of every scale from
tempered chains with replica exchange instead and writes fr_evidence_tempered{identifier}.npz beside fr_stat, which it
neither writes nor replaces.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import configs as Cf
from . import fr as fr_utils
from . import nested
from . import profile_llh
from . import realisations as realisations_mod
from .enums import DataType, ParamTag, StatCateg, Texture
from .llh import BinnedMeasurement, TabulatedLikelihood
from .mcmc import chain_identifier


DEFAULT_POSTERIOR_ROWS = 16384


def _enum(E):
    def parse(s):
        return E[str(s).rsplit(".", 1)[-1].upper()]
    return parse


def _bool(s):
    return str(s).lower() in ("true", "1", "yes", "y")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m golemflavor_amd.sens", description="BSM flavor ratio evidence scan "
                                 "(scripts/sens.py) on the device nested sampler")
    ap.add_argument("--seed", type=int, default=25, help="random seed")
    ap.add_argument("--datadir", type=str, default=None, help="where the arrays are written (default ./untitled)")
    ap.add_argument("--segments", type=int, default=10, help="number of new physics scales to evaluate (with the null point)")
    ap.add_argument("--eval-segment", type=str, default="all", help="which point to evaluate ('all' or an index)")
    ap.add_argument("--overwrite", type=_bool, default=False, help="overwrite existing arrays")
    ap.add_argument("--dimension", type=int, default=6, choices=sorted(Cf.SCALE_BOUNDARIES))
    ap.add_argument("--texture", type=_enum(Texture), default=Texture.OET)
    ap.add_argument("--source-ratio", type=float, nargs=3, default=[0, 1, 0])
    ap.add_argument("--injected-ratio", type=float, nargs=3, default=[1, 1, 1])
    ap.add_argument("--data", type=_enum(DataType), default=DataType.ASIMOV)
    ap.add_argument("--stat-method", type=_enum(StatCateg), default=StatCateg.BAYESIAN)
    ap.add_argument("--binning", type=float, nargs=3, default=list(Cf.DEFAULT_BINNING))
    ap.add_argument("--smearing", type=float, default=0.02, help="width of the Gaussian substitute likelihood")
    ap.add_argument("--mn-live-points", type=int, default=nested.DEFAULT_NLIVE)
    ap.add_argument("--mn-tolerance", type=float, default=nested.DEFAULT_TOL)
    ap.add_argument("--mn-batch", type=int, default=None, help="live points replaced per iteration (default nlive // 8)")
    ap.add_argument("--mn-walks", type=int, default=nested.DEFAULT_WALKS, help="Metropolis steps per replacement")
    ap.add_argument("--pl-starts", type=int, default=profile_llh.DEFAULT_STARTS,
                    help="frequentist: Nelder-Mead starts per scale (the best seed points)")
    ap.add_argument("--pl-seed-points", type=int, default=profile_llh.DEFAULT_SEED_POINTS,
                    help="frequentist: uniform points per scale the starts are picked from")
    ap.add_argument("--pl-xatol", type=float, default=profile_llh.DEFAULT_XATOL, help="frequentist: scipy's xatol")
    ap.add_argument("--pl-fatol", type=float, default=profile_llh.DEFAULT_FATOL, help="frequentist: scipy's fatol")
    ap.add_argument("--pl-maxiter", type=int, default=None, help="frequentist: iterations per start (default 200 n)")
    ap.add_argument("--pl-restarts", type=int, default=profile_llh.DEFAULT_RESTARTS,
                    help="frequentist: restarts of a converged start from its best vertex")
    ap.add_argument("--pl-adaptive", type=_bool, default=True, help="frequentist: scipy's adaptive coefficients")
    ap.add_argument("--realisations", type=int, default=None, metavar="T",
                    help="frequentist: also profile T mock measurements m = injected composition + smearing z, z ~ N(0, I), at every "
                         "scale, and write fr_realisations<identifier>.npz (max lnL, the statistic and the limit of every realisation, "
                         "the band of the limits); with --energy-resolved a mock measurement of every energy bin, m_k + sigma_k z")
    ap.add_argument("--realisation-seed", type=int, default=0,
                    help="with --realisations or --evidence-realisations: the seed the realisations are thrown with")
    ap.add_argument("--evidence-realisations", type=int, default=None, metavar="T",
                    help="bayesian: also give the evidence of T mock measurements m = injected composition + smearing z, z ~ N(0, I), at "
                         "every scale by reweighting the scan's own dead points (no further nested runs), and write "
                         "fr_evidence_realisations<identifier>.npz (ln Z, ESS and the Bayes-factor limit of every realisation, the band "
                         "of the limits)")
    ap.add_argument("--realisation-starts", type=int, default=realisations_mod.DEFAULT_TOY_STARTS,
                    help="with --realisations: Nelder-Mead starts per (realisation, scale), 1 to %d" % realisations_mod.MAX_TOY_STARTS)
    ap.add_argument("--on-nonunitary", choices=["raise", "-inf"], default="raise")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--posterior", action="store_true",
                    help="also save every scale's posterior (effective sample size, mean, covariance and the marginals of its "
                         "equal-weight rows), posterior_<identifier>_scale_<...>.npz beside fr_stat; needs --datadir")
    ap.add_argument("--posterior-rows", type=int, default=DEFAULT_POSTERIOR_ROWS,
                    help="with --posterior: equal-weight rows resampled per scale (default %d, this package's choice)"
                         % DEFAULT_POSTERIOR_ROWS)
    ap.add_argument("--posterior-elements", action="store_true",
                    help="with --posterior: also save the marginals in element space, posterior_elements_<...>.npz")
    ap.add_argument("--posterior-spectrum", type=float, nargs="*", default=None, metavar="Q",
                    help="with --posterior: also save every scale's composition per energy bin (mean, covariance, percentiles Q -- "
                         "default 5 16 50 84 95 -- and histograms of the equal-weight rows), posterior_spectrum_<...>.npz")
    ap.add_argument("--energy-resolved", action="store_true",
                    help="fit the composition of every energy bin (the energy-resolved Gaussian likelihood) instead of the flux "
                         "average: the measurement of every bin is the injected ratio, the null truth; the output files carry _ebins")
    ap.add_argument("--binned-measurement", type=str, default=None, metavar="FILE.npy",
                    help="energy-resolved with this measurement: an array [K, 3], one composition per energy bin of --binning")
    ap.add_argument("--binned-smearing", type=float, nargs="+", default=None, metavar="S",
                    help="energy-resolved: ONE value is the width of the flux-averaged likelihood to be comparable with, "
                         "sigma_k = S / sqrt(w_k) (default: --smearing); K values are the widths of the bins themselves")
    ap.add_argument("--likelihood-table", type=str, default=None, metavar="FILE.npy",
                    help="a tabulated flavour-plane likelihood in place of the Gaussian: the flat array of ln L at the (N + 1)(N + 2) / 2 "
                         "nodes of the flavour triangle's lattice (llh.TabulatedLikelihood.save); the output files carry _ltab")
    ap.add_argument("--evidence-method", choices=["nested", "stepping-stone"], default="nested",
                    help="bayesian: 'stepping-stone' gives ln Z of every scale from tempered chains with replica exchange instead "
                         "(DESIGN.md 6n), an estimate independent of the nested sampler's, and writes fr_evidence_tempered<identifier>.npz "
                         "beside fr_stat, which it neither writes nor replaces")
    ap.add_argument("--temperatures", type=int, default=8, metavar="N", help="stepping-stone: geometric rungs from 1 down to --beta-min (the prior's rung 0 is added)")
    ap.add_argument("--beta-min", type=float, default=1e-3, metavar="B", help="stepping-stone: the smallest positive beta")
    ap.add_argument("--swap-every", type=int, default=8, metavar="S", help="stepping-stone: a replica-exchange round every S steps (0: never)")
    ap.add_argument("--tempered-steps", type=int, default=1500, metavar="K", help="stepping-stone: stored steps per chain, after K // 3 of burn-in")
    ap.add_argument("--tempered-walkers", type=int, default=256, help="stepping-stone: walkers per chain")
    args = ap.parse_args(argv)
    if args.evidence_method == "stepping-stone":
        if args.stat_method is not StatCateg.BAYESIAN:
            ap.error("--evidence-method stepping-stone is an evidence: it needs the Bayesian method")
        if args.energy_resolved or args.binned_measurement is not None or args.likelihood_table is not None:
            ap.error("--evidence-method stepping-stone samples the flux-averaged likelihood only: it does not combine with "
                     "--energy-resolved or --likelihood-table")
        if args.realisations is not None or args.evidence_realisations is not None or args.posterior:
            ap.error("--evidence-method stepping-stone does not combine with --realisations, --evidence-realisations or --posterior")
        if args.temperatures < 1 or args.temperatures > 63 or not 0. < args.beta_min < 1. or args.swap_every < 0 or args.tempered_steps < 16:
            ap.error("--temperatures takes 1 to 63, --beta-min a value in (0, 1), --swap-every S >= 0, --tempered-steps K >= 16")
        if args.tempered_walkers < 24 or args.tempered_walkers % 2:
            ap.error("--tempered-walkers takes an even number, at least twice the columns (24)")
    if args.likelihood_table is not None:
        if args.energy_resolved or args.binned_measurement is not None or args.binned_smearing is not None:
            ap.error("--likelihood-table replaces the flux-averaged likelihood: it does not combine with --energy-resolved")
        if args.realisations is not None or args.evidence_realisations is not None:
            ap.error("a realisation of a table is not defined: --likelihood-table does not combine with --realisations or "
                     "--evidence-realisations")
    if args.binned_measurement is not None:
        args.energy_resolved = True
    if args.binned_smearing is not None:
        if not args.energy_resolved:
            ap.error("--binned-smearing needs --energy-resolved or --binned-measurement")
        K = int(args.binning[2])
        if len(args.binned_smearing) not in (1, K) or not all(s > 0. for s in args.binned_smearing):
            ap.error("--binned-smearing takes one positive value or one per energy bin (%d)" % K)
    if args.realisations is not None:
        if args.stat_method is not StatCateg.FREQUENTIST:
            ap.error("--realisations needs --stat-method frequentist (it profiles mock measurements)")
        if args.realisations < 1 or not 1 <= args.realisation_starts <= realisations_mod.MAX_TOY_STARTS:
            ap.error("--realisations takes T >= 1 and --realisation-starts 1 to %d" % realisations_mod.MAX_TOY_STARTS)
        if args.eval_segment.lower() != "all":
            ap.error("--realisations needs every scale (a limit per realisation): it does not combine with --eval-segment")
    if args.evidence_realisations is not None:
        if args.stat_method is not StatCateg.BAYESIAN:
            ap.error("--evidence-realisations needs the Bayesian method (it reweights the nested runs' points); "
                     "--stat-method frequentist has --realisations")
        if args.evidence_realisations < 1:
            ap.error("--evidence-realisations takes T >= 1")
        if args.energy_resolved:
            ap.error("--evidence-realisations are of the flux-averaged likelihood: it does not combine with --energy-resolved")
        if args.eval_segment.lower() != "all":
            ap.error("--evidence-realisations needs every scale (a limit per realisation): it does not combine with --eval-segment")
    if args.posterior_elements and not args.posterior:
        ap.error("--posterior-elements needs --posterior (it adds the element-space marginals to it)")
    if args.posterior_spectrum is not None:
        if not args.posterior:
            ap.error("--posterior-spectrum needs --posterior (it adds the composition per energy bin to it)")
        args.posterior_spectrum = args.posterior_spectrum or [5., 16., 50., 84., 95.]
        if not 1 <= len(args.posterior_spectrum) <= 8 or not all(0. <= q <= 100. for q in args.posterior_spectrum):
            ap.error("--posterior-spectrum takes up to 8 percentiles in [0, 100]")
    if args.posterior:
        if not args.datadir:
            ap.error("--posterior needs --datadir (the posteriors are saved beside the fr_stat arrays)")
        if args.stat_method is StatCateg.FREQUENTIST:
            ap.error("--posterior needs the nested sampler: it does not combine with --stat-method frequentist")
        if args.posterior_rows < 1:
            ap.error("--posterior-rows must be at least 1")
    if args.datadir is None:
        args.datadir = "./untitled"
    if args.texture is Texture.NONE:
        ap.error("Must assume a BSM texture")                         # sens.py:145-146
    args.source_ratio = fr_utils.normalize_fr(args.source_ratio)
    if args.data is not DataType.REAL:
        args.injected_ratio = fr_utils.normalize_fr(args.injected_ratio)
    args.binning = Cf.default_bin_edges((args.binning[0], args.binning[1], int(args.binning[2])))
    args.eval_segment = None if args.eval_segment.lower() == "all" else int(args.eval_segment)
    return args


def identifier(args):
    """The reference's file-name stem (`chain_identifier`); `_ebins` appended for the energy-resolved likelihood, whose results never
    overwrite the flux-averaged ones."""
    return (chain_identifier(args) + ("_ebins" if getattr(args, "energy_resolved", False) else "")
            + ("_ltab" if getattr(args, "likelihood_table", None) is not None else ""))


def likelihood_table(args):
    """The `TabulatedLikelihood` of --likelihood-table, None without it."""
    if getattr(args, "likelihood_table", None) is None:
        return None
    return TabulatedLikelihood.load(args.likelihood_table)


def binned_measurement(args, asimov_paramset):
    """The `BinnedMeasurement` of --energy-resolved / --binned-measurement / --binned-smearing, None without them.  Without a file the
    measurement of every bin is the composition the flux-averaged likelihood is centred on (the injected ratio: the null truth)."""
    if not getattr(args, "energy_resolved", False):
        return None
    edges = np.asarray(args.binning, dtype=np.float64)
    sm = args.binned_smearing if getattr(args, "binned_smearing", None) is not None else [args.smearing]
    sm = sm[0] if len(sm) == 1 else sm
    if getattr(args, "binned_measurement", None) is not None:
        return BinnedMeasurement(np.load(args.binned_measurement), sm, binning=edges)
    bf = fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    return BinnedMeasurement.constant(bf, sm, edges)


def output_paths(args, scales=None):
    """sens.py:235-240, 247-250: (fr_stat, fr_maxllh) file names without '.npy'."""
    base = os.path.join(args.datadir, args.stat_method.name.lower(), args.data.name.lower())
    ident = identifier(args)
    stat, llh = os.path.join(base, "fr_stat" + ident), os.path.join(base, "fr_maxllh" + ident)
    if args.eval_segment is not None:
        sc = (scales if scales is not None else nested.sens_scales(args.dimension, args.segments))[args.eval_segment]
        tail = "_scale_{0:.0E}".format(np.power(10., sc))
        stat, llh = stat + tail, llh + tail
    return stat, llh


def posterior_path(args, scale, elements=False):
    """posterior[_elements]<identifier>_scale_<10^scale:.0E>.npz beside fr_stat<identifier>.npy."""
    base = os.path.join(args.datadir, args.stat_method.name.lower(), args.data.name.lower())
    return os.path.join(base, "posterior{0}{1}_scale_{2:.0E}.npz".format("_elements" if elements else "", identifier(args),
                                                                       np.power(10., scale)))


def spectrum_path(args, scale):
    """posterior_spectrum<identifier>_scale_<10^scale:.0E>.npz beside the posterior files."""
    base = os.path.join(args.datadir, args.stat_method.name.lower(), args.data.name.lower())
    return os.path.join(base, "posterior_spectrum{0}_scale_{1:.0E}.npz".format(identifier(args), np.power(10., scale)))


def save_spectra(args, scales, res):
    """One .npz per scale: `SpectrumResult.as_arrays()` plus the scale."""
    files = []
    for k, sc in enumerate(scales):
        arrays = res["spectrum"][k].as_arrays()
        arrays.update(scale=np.float64(sc))
        f = spectrum_path(args, sc)
        os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
        with open(f, "wb") as fh:
            np.savez(fh, **arrays)
        files.append(f)
    return files


def save_posteriors(args, scales, res):
    """One .npz per scale: `MarginalResult.as_arrays()` plus ess, npoints, mean, cov (and lnz_check, scale)."""
    files = []
    for k, sc in enumerate(scales):
        for key, elements in (("marginals", False), ("marginals_elements", True)):
            if key not in res:
                continue
            arrays = res[key][k].as_arrays()
            arrays.update({f: res["posterior"][f][k] for f in ("ess", "npoints", "lnz_check")})
            arrays.update(mean=res["posterior"]["mean"][k], cov=res["posterior"]["cov"][k], scale=np.float64(sc))
            f = posterior_path(args, sc, elements)
            os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
            with open(f, "wb") as fh:
                np.savez(fh, **arrays)
            files.append(f)
    return files


def main(argv=None):
    args = parse_args(argv)
    scales = nested.sens_scales(args.dimension, args.segments)
    outfile, outfile_llh = output_paths(args, scales)
    if getattr(args, "evidence_method", "nested") == "stepping-stone":
        return _stepping_stone(args, scales)
    for f in (outfile, outfile_llh):
        if not args.overwrite and os.path.isfile(f + ".npy") and np.all(np.isfinite(np.load(f + ".npy"))):
            print("FILE EXISTS {0}".format(f + ".npy"))
            return 0
    idx = np.arange(len(scales)) if args.eval_segment is None else np.array([args.eval_segment])
    asimov, llh_ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    try:
        binned = binned_measurement(args, asimov)
        table = likelihood_table(args)
    except (ValueError, OSError) as exc:
        print("golemflavor_amd.sens: %s" % exc, file=sys.stderr)
        return 2
    if args.stat_method is StatCateg.FREQUENTIST:
        return _frequentist(args, scales, idx, asimov, llh_ps, outfile, outfile_llh, binned, table)
    post = dict(nrows=args.posterior_rows, elements=args.posterior_elements) if args.posterior else None
    if post is not None and args.posterior_spectrum is not None:
        post["spectrum"] = args.posterior_spectrum
    toys = None
    if getattr(args, "evidence_realisations", None) is not None:
        ens = realisations_mod.evidence_realisation_scan(args, asimov, llh_ps, scales[idx], ntoys=args.evidence_realisations,
                                                         toy_seed=args.realisation_seed, run_ids=idx, on_nonunitary=args.on_nonunitary,
                                                         device=args.device, posterior=post)
        res = ens["asimov"]
        toys = _evidence_realisations(args, ens)
    else:
        res = nested.evidence_scan(args, asimov, llh_ps, scales[idx], run_ids=idx, on_nonunitary=args.on_nonunitary,
                                   device=args.device, posterior=post, binned=binned, **({"table": table} if table is not None else {}))
    evidence_arr = np.stack([scales[idx], res["lnz"]], axis=1)
    maxllh_arr = np.stack([scales[idx], res["max_lnl"]], axis=1)
    for f, arr in ((outfile, evidence_arr), (outfile_llh, maxllh_arr)):
        os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
        np.save(f + ".npy", arr)
    posterior_files = save_posteriors(args, scales[idx], res) if args.posterior else None
    if posterior_files is not None and "spectrum" in res:
        posterior_files += save_spectra(args, scales[idx], res)
    print(json.dumps({
        **({"evidence_realisations": toys} if toys is not None else {}),
        **({"posterior": posterior_files} if posterior_files is not None else {}),
        **({"likelihood": "energy-resolved"} if binned is not None else {}),
        **({"likelihood": "table", "table_nside": table.nside} if table is not None else {}),
        "tool": "golemflavor_amd.sens", "dimension": args.dimension, "texture": args.texture.name,
        "segments": args.segments, "nlive": args.mn_live_points, "scales": scales[idx].tolist(),
        "lnz": res["lnz"].tolist(), "lnz_err": res["lnz_err"].tolist(), "max_lnl": res["max_lnl"].tolist(),
        "niter": res["niter"].tolist(), "nevals": int(res["nevals"].sum()), "nonunitary": res["nonunitary"].tolist(),
        "seconds": round(res["seconds"], 4), "evals_per_s": float(res["nevals"].sum() / max(res["seconds"], 1e-12)),
        "fr_stat": outfile + ".npy", "fr_maxllh": outfile_llh + ".npy"}))
    return 0


def evidence_tempered_path(args):
    """fr_evidence_tempered<identifier>.npz beside fr_stat<identifier>.npy (with --eval-segment: its `_scale_` tail too)."""
    stat = output_paths(args)[0]
    return os.path.join(os.path.dirname(stat), os.path.basename(stat).replace("fr_stat", "fr_evidence_tempered", 1) + ".npz")


def _stepping_stone(args, scales):
    """--evidence-method stepping-stone: ln Z of every scale from tempered chains (`tempering.evidence_scan_tempered`), its file, the
    JSON line.  fr_stat and fr_maxllh are neither read nor written: `nested.bayes_factor_limit` takes this file's ln_z as it takes theirs."""
    from . import tempering
    idx = np.arange(len(scales)) if args.eval_segment is None else np.array([args.eval_segment])
    asimov, llh_ps = Cf.sens_paramsets(args.dimension, args.injected_ratio, data=args.data)
    res = tempering.evidence_scan_tempered(args, asimov, llh_ps, scales[idx], ntemps=args.temperatures, beta_min=args.beta_min,
                                           swap_every=args.swap_every, nwalkers=args.tempered_walkers, burnin=args.tempered_steps // 3,
                                           nsteps=args.tempered_steps, seed=args.seed, on_nonunitary=args.on_nonunitary, device=args.device)
    f = evidence_tempered_path(args)
    os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
    with open(f, "wb") as fh:
        np.savez(fh, scales=res["scales"], ln_z=res["ln_z"], ln_z_err=res["ln_z_err"], ln_ratio=res["ln_ratio"], ln_ratio_ti=res["ln_ratio_ti"],
                 swap_fraction=res["swap_fraction"], nonunitary=np.int64(res["nonunitary"]), nonfinite_fraction=res["nonfinite_fraction"],
                 betas=res["betas"])

    def clean(a):
        return [None if not np.isfinite(v) else float(v) for v in np.asarray(a, dtype=np.float64).ravel()]

    print(json.dumps({"tool": "golemflavor_amd.sens", "evidence_method": "stepping-stone", "dimension": args.dimension, "texture": args.texture.name,
                      "segments": args.segments, "scales": scales[idx].tolist(), "ln_z": clean(res["ln_z"]), "ln_z_err": clean(res["ln_z_err"]),
                      "ln_z_thermodynamic_minus_ln_z0": clean(res["ln_ratio_ti"]), "betas": res["betas"].tolist(),
                      "lowest_swap_fraction": clean([np.nanmin(res["swap_fraction"]) if np.isfinite(res["swap_fraction"]).any() else np.nan])[0],
                      "nonunitary": int(res["nonunitary"]), "seconds": round(res["seconds"], 4), "fr_evidence_tempered": f}))
    return 0


def evidence_realisations_path(args):
    """fr_evidence_realisations<identifier>.npz beside fr_stat<identifier>.npy (the evidence array)."""
    base = os.path.join(args.datadir, args.stat_method.name.lower(), args.data.name.lower())
    return os.path.join(base, "fr_evidence_realisations" + identifier(args) + ".npz")


def _evidence_realisations(args, ens):
    """--evidence-realisations: the ensemble's file, and what the JSON line says of it."""
    f = evidence_realisations_path(args)
    os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
    band = realisations_mod.save_evidence_realisations(f, ens)

    def clean(a):
        return [None if not np.isfinite(v) else float(v) for v in np.asarray(a, dtype=np.float64).ravel()]

    return {"file": f, "n": args.evidence_realisations, "seed": args.realisation_seed, "band_quantiles": band["quantiles"].tolist(),
            "band_limits": clean(band["limits"]), "without_limit": band["n_without_limit"], "discovered": int(ens["discovered"].sum()),
            "lowest_ess_fraction": clean([np.min(np.where(np.isnan(ens["ess_fraction"]), np.inf, ens["ess_fraction"]))])[0], "seconds_nested": round(ens["seconds_nested"], 4),
            "seconds_reweight": round(ens["seconds_reweight"], 4)}


def realisations_path(args):
    """fr_realisations<identifier>.npz beside fr_maxllh<identifier>.npy."""
    base = os.path.join(args.datadir, args.stat_method.name.lower(), args.data.name.lower())
    return os.path.join(base, "fr_realisations" + identifier(args) + ".npz")


def _realisations(args, scales, idx, asimov, llh_ps, binned=None):
    """--realisations: the scan (of the energy-resolved likelihood with `binned`), its file, and what the JSON line says of it."""
    kw = dict(ntoys=args.realisations, toy_seed=args.realisation_seed, nstarts=args.realisation_starts, run_ids=idx,
              on_nonunitary=args.on_nonunitary, device=args.device)
    if binned is not None:
        res = realisations_mod.binned_realisation_scan(args, asimov, llh_ps, scales[idx], binned, **kw)
    else:
        res = realisations_mod.realisation_scan(args, asimov, llh_ps, scales[idx], **kw)
    f = realisations_path(args)
    os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
    band = realisations_mod.save_realisations(f, res)
    crit = realisations_mod.ts_quantiles(res["ts"], 95.)
    return {"file": f, "n": args.realisations, "seed": args.realisation_seed, "starts": args.realisation_starts,
            "band_quantiles": band["quantiles"].tolist(), "band_limits": band["limits"].tolist(),
            "without_limit": band["n_without_limit"], "ts_q95": crit.tolist(), "seconds": round(res["seconds"], 4)}


def _frequentist(args, scales, idx, asimov, llh_ps, outfile, outfile_llh, binned=None, table=None):
    res = profile_llh.profile_scan(args, asimov, llh_ps, scales[idx], run_ids=idx, on_nonunitary=args.on_nonunitary,
                                   device=args.device, binned=binned, **({"table": table} if table is not None else {}))
    arr = np.stack([scales[idx], res["max_lnl"]], axis=1)
    for f in (outfile, outfile_llh):
        os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
        np.save(f + ".npy", arr)
    ml = res["max_lnl"]
    null = np.flatnonzero(scales[idx] == scales[0])
    ts = (-2 * (ml - ml[null[0]])).tolist() if len(null) and np.isfinite(ml[null[0]]) else None
    limit = profile_llh.profile_likelihood_limit(scales[idx], ml) if args.eval_segment is None else None
    toys = _realisations(args, scales, idx, asimov, llh_ps, binned) if getattr(args, "realisations", None) is not None else None
    print(json.dumps({
        **({"realisations": toys} if toys is not None else {}),
        **({"likelihood": "energy-resolved"} if binned is not None else {}),
        **({"likelihood": "table", "table_nside": table.nside} if table is not None else {}),
        "tool": "golemflavor_amd.sens", "stat_method": "FREQUENTIST", "dimension": args.dimension,
        "texture": args.texture.name, "segments": args.segments, "scales": scales[idx].tolist(), "max_lnl": ml.tolist(),
        "ts": ts, "limit": None if limit is None else float(limit), "starts": res["nstarts"].tolist(),
        "starts_agreeing": res["starts_agreeing"].tolist(), "niter": res["niter"].tolist(), "nfev": res["nfev"].tolist(),
        "nevals": int(res["nevals"].sum()), "nonunitary": res["nonunitary"].tolist(), "seconds": round(res["seconds"], 4),
        "evals_per_s": float(res["nevals"].sum() / max(res["seconds"], 1e-12)),
        "fr_stat": outfile + ".npy", "fr_maxllh": outfile_llh + ".npy"}, allow_nan=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
