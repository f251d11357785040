"""Tempered chains as a second route to the evidence: the ladder, the stepping-stone and thermodynamic estimators on the
series `DeviceEnsembleSampler.lnl_series()` reduces on the device, the closed-form prior mass that turns their ratio into ln Z in the
nested sampler's convention, and the scan over sens.py's scales that `nested.evidence_scan` can be checked against.

The identity.  Chain k of a ladder 1 = beta_0 > beta_1 > ... > beta_{K-1} >= 0 samples prior * L^beta_k / Z(beta_k).  For neighbours
    Z(beta_k) / Z(beta_{k+1}) = < L^(beta_k - beta_{k+1}) >  under chain k + 1,
so ln(Z_1 / Z_{beta_{K-1}}) is the sum over the rungs of the logs of those means (Xie et al. 2011, "stepping-stone sampling").  A sample
with L = 0 contributes 0 to the mean -- the estimator is exact where the likelihood vanishes on part of the prior, where the
thermodynamic integral of <ln L> is -inf.  With the last rung at beta = 0 the denominator is Z_0, the prior's own mass."""
import math
import time

import numpy as np

from .enums import ParamTag, PriorsCateg


def geometric_ladder(ntemps, beta_min):
    """ntemps + 1 betas: the geometric ladder 1 = beta_min^0, ..., beta_min^1 over ntemps rungs, then the prior's rung 0."""
    ntemps = int(ntemps)
    if ntemps < 1 or not 0.0 < float(beta_min) < 1.0:
        raise ValueError("geometric_ladder takes ntemps >= 1 and 0 < beta_min < 1")
    if ntemps == 1:
        return np.array([1.0, 0.0])
    b = float(beta_min) ** (np.arange(ntemps) / (ntemps - 1.0))
    b[0], b[-1] = 1.0, float(beta_min)
    return np.concatenate([b, [0.0]])


def _log_mean_steps(log_terms, nw):
    """ln of the mean over steps and walkers of terms given per step as ln(sum over walkers); -inf where every term is 0."""
    m = np.max(log_terms)
    if not np.isfinite(m):
        return -np.inf
    return m + math.log(np.sum(np.exp(log_terms - m))) - math.log(len(log_terms) * nw)


def stepping_stone(series, betas, discard=0, nbatch=16, nwalkers=None):
    """The estimators of one or more groups.  series: (ngroups * ntemps, nstored, 5) as `lnl_series()` returns it with its default
    exponents (count of finite lnl, their sum, their max m, sum_w exp(d_up (lnl - m)), sum_w exp(d_dn (lnl - m)), d_up the distance in beta
    to the rung above).  betas (ntemps,); discard: stored steps left out at the start; nwalkers: of the ensemble (default: the largest
    count seen, right unless every step of every chain holds a non-finite lnl).  Returns a dict of arrays with a leading group axis:

      ln_ratio            ln(Z(betas[0]) / Z(betas[-1])): the sum over k of ln mean(L^(beta_k - beta_{k+1})) under chain k + 1, the mean
                          over steps combined by log-sum-exp
      ln_ratio_err        its standard error from `nbatch` batch means over the steps of every rung, added in quadrature over the rungs;
                          approximate once exchanges correlate neighbouring chains
      ln_ratio_ti         the trapezoid over beta of the mean finite lnl; NaN if a chain it uses holds a non-finite lnl
      rungs               (ntemps - 1,) the terms of ln_ratio
      rungs_err           their standard errors
      nonfinite_fraction  (ntemps,) the share of each chain's samples without a finite lnl"""
    betas = np.asarray(betas, dtype=np.float64)
    K = len(betas)
    s = np.asarray(series, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 5 or s.shape[0] % K:
        raise ValueError("series must be (ngroups * %d, nstored, 5), got %s" % (K, s.shape))
    s = s[:, int(discard):]
    G, ns = s.shape[0] // K, s.shape[1]
    if ns < 1:
        raise ValueError("no stored steps left after discarding %d" % discard)
    nw = float(nwalkers if nwalkers is not None else s[:, :, 0].max())
    s = s.reshape(G, K, ns, 5)
    nbatch = max(1, min(int(nbatch), ns))
    out = dict(ln_ratio=np.zeros(G), ln_ratio_err=np.zeros(G), ln_ratio_ti=np.zeros(G), rungs=np.zeros((G, max(K - 1, 0))),
               rungs_err=np.zeros((G, max(K - 1, 0))), nonfinite_fraction=np.zeros((G, K)))
    with np.errstate(divide="ignore", invalid="ignore"):
        for g in range(G):
            cnt, tot, m, sup = s[g, :, :, 0], s[g, :, :, 1], s[g, :, :, 2], s[g, :, :, 3]
            out["nonfinite_fraction"][g] = (ns * nw - cnt.sum(axis=1)) / (ns * nw)
            var = 0.0
            for k in range(K - 1):
                d = betas[k] - betas[k + 1]
                # per step of chain k + 1: ln sum_w L^d = d m + ln S_up (S_up = 0 and m = -inf where no walker has a finite lnl)
                lt = np.where(cnt[k + 1] > 0, d * m[k + 1] + np.log(sup[k + 1]), -np.inf)
                out["rungs"][g, k] = _log_mean_steps(lt, nw)
                edges = np.linspace(0, ns, nbatch + 1).astype(int)
                bm = np.array([_log_mean_steps(lt[a:b], nw) for a, b in zip(edges[:-1], edges[1:]) if b > a])
                if len(bm) > 1 and np.all(np.isfinite(bm)):
                    # the batch means in linear units relative to the overall one: var(ln mean) ~ var(mean) / mean^2
                    rel = np.exp(bm - out["rungs"][g, k])
                    out["rungs_err"][g, k] = np.std(rel, ddof=1) / math.sqrt(len(rel))
                else:
                    out["rungs_err"][g, k] = np.inf if len(bm) > 1 else np.nan
                var += out["rungs_err"][g, k] ** 2
            out["ln_ratio"][g] = out["rungs"][g].sum()
            out["ln_ratio_err"][g] = math.sqrt(var) if K > 1 else 0.0
            mean_lnl = np.where(cnt.sum(axis=1) == ns * nw, tot.sum(axis=1) / (ns * nw), np.nan)
            out["ln_ratio_ti"][g] = float(np.sum(0.5 * (mean_lnl[:-1] + mean_lnl[1:]) * (betas[:-1] - betas[1:]))) if K > 1 else 0.0
    return out


def prior_draws(paramset, n, rng):
    """n draws of the prior over the box, (n, ndim): uniform columns uniformly, Gaussian ones -- truncated, or cut by the box -- by
    rejection.  rng: a numpy Generator."""
    out = np.empty((int(n), len(paramset)))
    for c, p in enumerate(paramset):
        lo, hi = float(p.ranges[0]), float(p.ranges[1])
        if p.prior is PriorsCateg.UNIFORM:
            out[:, c] = rng.uniform(lo, hi, int(n))
            continue
        x = np.empty(0)
        while x.size < n:
            d = rng.normal(float(p.nominal_value), float(p.std), 2 * int(n))
            x = np.concatenate([x, d[(d >= lo) & (d <= hi)]])
        out[:, c] = x[:int(n)]
    return out


def ladder_start(model, paramset, betas, nwalkers, rng, ndraws=1 << 17):
    """Start positions (ntemps, nwalkers, ndim) that are in equilibrium from the first step where the prior reaches the posterior: `ndraws`
    prior draws, and for every rung nwalkers DISTINCT ones picked with probability proportional to L^beta (the prior's rung: the
    first nwalkers).  Why: chains that all start from the prior are far from equilibrium at the cold end, and the first exchanges hand
    their low-likelihood walkers down the ladder, which the hot chains -- the slowest to mix -- take hundreds of steps to shed; the
    rungs' means of L^(delta beta) are biased low for as long.  Where a rung has fewer than nwalkers draws with L^beta > 0 the rest are
    the draws with the largest lnl.  Returns (p0, ess): ess (ntemps,) the effective number of draws behind every rung, the figure
    that says whether the start can be trusted (it should exceed nwalkers by a wide margin)."""
    th = prior_draws(paramset, ndraws, rng)
    lnl, st = model.lnprior_lnlike(th)[1:]
    lnl = np.where((st == 0) & np.isfinite(lnl), lnl, -np.inf)
    p0 = np.empty((len(betas), int(nwalkers), th.shape[1]))
    ess = np.empty(len(betas))
    order = np.argsort(-lnl, kind="stable")
    for k, b in enumerate(betas):
        if b == 0.0:
            p0[k], ess[k] = th[:nwalkers], float(ndraws)
            continue
        with np.errstate(invalid="ignore"):
            w = np.where(lnl > -np.inf, np.exp(b * (lnl - lnl.max())), 0.0)
        ess[k] = w.sum() ** 2 / np.sum(w * w)
        if np.count_nonzero(w) >= nwalkers:
            pick = rng.choice(ndraws, size=int(nwalkers), replace=False, p=w / w.sum())
        else:
            pick = order[:nwalkers]
        p0[k] = th[pick]
    return p0, ess


def _gauss_columns(paramset):
    return [p for p in paramset if p.prior is not PriorsCateg.UNIFORM]


def prior_log_mass(paramset):
    """ln of the integral of exp(lnprior) over the box, column by column in closed form.  A uniform column contributes 0, as `lnprior` has
    it (its width belongs to the box volume, and `ln_box_volume` leaves it out too: the two cancel in ln Z).  A Gaussian column
    contributes ln[(Phi(b) - Phi(a))] - log_mass with a, b the box in units of sigma around the nominal value and log_mass what
    `descriptor.compile_model` puts into lnprior: 0 for a truncated Gaussian (it is normalised over the box), ln(Phi(b) - Phi(a)) for an
    unbounded one (whose tails outside the box are lost)."""
    from .descriptor import log_gauss_mass
    total = 0.0
    for p in _gauss_columns(paramset):
        loc, sig = float(p.nominal_value), float(p.std)
        inside = log_gauss_mass((float(p.ranges[0]) - loc) / sig, (float(p.ranges[1]) - loc) / sig)
        total += inside - (inside if p.prior is PriorsCateg.LIMITEDGAUSS else 0.0)
    return total


def ln_box_volume(paramset):
    """ln of the volume of the box over the columns `prior_log_mass` integrates in their own units, the Gaussian ones."""
    return float(sum(math.log(float(p.ranges[1]) - float(p.ranges[0])) for p in _gauss_columns(paramset)))


def ln_z0(paramset):
    """ln Z at beta = 0 in the nested sampler's convention, Z = the integral over the unit cube of exp(lnprob)."""
    return prior_log_mass(paramset) - ln_box_volume(paramset)


def _opt(args, name, default):
    v = getattr(args, name, None)
    return default if v is None else v


def evidence_scan_tempered(args, asimov_paramset, llh_paramset, scales, ntemps=8, beta_min=1e-3, swap_every=8, nwalkers=256, burnin=500,
                           nsteps=1500, discard=0, nbatch=16, seed=None, on_nonunitary="raise", smearing=None, device=0, binned=None,
                           table=None):
    """ln Z of every scale by stepping-stone, the integral `nested.evidence_scan` does: per scale the model over every column but the
    scale, the scale fixed (`scale_fixed`) -- the scale's own prior is uniform and adds nothing --, the scales as the groups of ONE
    tempered sampler on `geometric_ladder(ntemps, beta_min)`.  Returns dict(scales, ln_z, ln_z_err, ln_ratio, ln_ratio_ti, swap_fraction
    (nscales, ntemps), nonunitary, nonfinite_fraction, betas, seconds, start_ess).  Every chain starts from `ladder_start`'s positions
    (start_ess (nscales, ntemps): the effective number of prior draws behind each).  With on_nonunitary="-inf" the ratio is over the region where the
    reference does not raise: `nonunitary` counts the proposals it would have died on, and nothing corrects for them.  binned
    (`llh.BinnedMeasurement`): the evidence of the energy-resolved likelihood -- the measurement is attached to every
    scale's model, as `nested.evidence_scan` does, and the sampler is the tempered binned one.  table (`llh.TabulatedLikelihood`):
    likewise the tabulated flavour-plane likelihood; not together with `binned`."""
    if binned is not None and table is not None:
        raise ValueError("binned and table are two likelihoods: give one")
    from . import fr as fr_utils
    from .descriptor import compile_model
    from .llh import LnProb
    from .mcmc import DeviceEnsembleSampler
    scales = np.asarray(scales, dtype=np.float64)
    ps = llh_paramset.from_tag(ParamTag.SCALE, invert=True)
    scale_prm = llh_paramset.from_tag(ParamTag.SCALE)[0]
    if scale_prm.prior is not PriorsCateg.UNIFORM:
        raise ValueError("the scale's prior is not uniform: fixing it changes the integrand by a scale-dependent constant")
    smearing = float(smearing if smearing is not None else _opt(args, "smearing", 0.02))
    bf = fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    betas = geometric_ladder(ntemps, beta_min)
    seed = int(seed if seed is not None else _opt(args, "seed", 0) or 0)
    fns = []
    try:
        for sc in scales:
            fns.append(LnProb(compile_model(ps, "BSM_GAUSS", bestfit_fr=bf, smearing=smearing, source_ratio=args.source_ratio,
                                            texture=args.texture, dimension=args.dimension, binning=args.binning, scale_fixed=float(sc)),
                              device=device, on_nonunitary=on_nonunitary))
            if binned is not None:
                fns[-1].model.set_binned_measurement(binned)
            if table is not None:
                fns[-1].model.set_table_likelihood(table)
        s = DeviceEnsembleSampler(int(nwalkers), len(ps), fns, seed=seed, betas=betas, swap_every=int(swap_every), ngroups=len(scales),
                                  energy_resolved=binned is not None, tabulated=table is not None)
        try:
            rng = np.random.default_rng(seed)
            starts = [ladder_start(f.model, ps, betas, int(nwalkers), rng) for f in fns]
            p0 = np.concatenate([p for p, _ in starts])
            t0 = time.perf_counter()
            s.run_mcmc(p0, int(burnin), storechain=False)
            s.reset()
            s.run_mcmc(None, int(nsteps))
            est = stepping_stone(s.lnl_series(), betas, discard=discard, nbatch=nbatch, nwalkers=int(nwalkers))
            seconds = time.perf_counter() - t0
            z0 = ln_z0(ps)
            return dict(scales=scales, ln_z=z0 + est["ln_ratio"], ln_z_err=est["ln_ratio_err"], ln_ratio=est["ln_ratio"],
                        ln_ratio_ti=est["ln_ratio_ti"], swap_fraction=s.swap_fraction, nonunitary=s.nonunitary_proposals,
                        nonfinite_fraction=est["nonfinite_fraction"], betas=betas, seconds=seconds,
                        start_ess=np.stack([e for _, e in starts]))
        finally:
            s.close()
    finally:
        for f in fns:
            f.close()
