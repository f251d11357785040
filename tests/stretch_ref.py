"""Test infrastructure (not a test module): the published stretch move written out in numpy on the device sampler's random
stream, and the reference's unitarity verdict with the band around its threshold arbitrated by the host build of the device's
x87 chain.  Used by tests/test_gpu_sampler.py, tests/test_gpu_fuzz.py and tests/test_gpu_scan_exact.py.

The device sampler (golemflavor_amd/csrc/gf_sampler.hip, stretch_body) draws one Philox4x32-10 block per (walker slot, half-step):
counter = (sid * (nwalkers / 2) + k, 2 * iteration + half), key = seed, where sid is the chain's stream id (its index in the
sampler unless `stream_ids` names it) and `iteration` counts every step since the sampler was created -- `reset()` clears the
stored chain, not the counter.  u1 has 53 bits, the partner j and u3 32 bits each; z = fma(a - 1, u1, 1)^2 / a; the proposal is
q = fma(-z, c_j - s_k, c_j), rounded once; the walker moves iff ln(z^(ndim-1) / u3) > lnprob(s_k) - lnprob(q), with z^(ndim-1)
a running product.  Step `it` of a run is stored iff it % thin == 0."""
from fractions import Fraction

import numpy as np

BAND = (10 ** -7.25, 10 ** -6.75)     # half a decade around the reference's threshold 1e-7 (fr.py:493-494)


def fma(x, y, z):
    """x * y + z rounded once (int / int true division is correctly rounded)."""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def draws(oracle, key, sid, nhalf, k, t, a=2.0):
    """(z, j, u3) of walker slot k of stream `sid` at half-step counter t."""
    g = sid * nhalf + k
    r = oracle.philox4x32_10((g & 0xffffffff, g >> 32, t & 0xffffffff, t >> 32), key)
    u1 = ((r[0] >> 5) * 67108864.0 + (r[1] >> 6)) / 9007199254740992.0
    j = (r[2] * nhalf) >> 32
    u3 = (r[3] + 0.5) / 4294967296.0
    zr = fma(a - 1.0, u1, 1.0)
    return zr * zr / a, j, u3


def propose(oracle, key, pos, half, t, sid=0, a=2.0, exact=True):
    """Proposals of the active half `half` of one ensemble `pos` (nwalkers, ndim) at half-step counter t:
    (q (nhalf, ndim), z (nhalf,), u3 (nhalf,)).  exact=False forms q as c_j - z (c_j - s_k) in two roundings."""
    nwalkers, ndim = pos.shape
    nhalf = nwalkers // 2
    cbase = (1 - half) * nhalf
    q, zz, u3 = np.empty((nhalf, ndim)), np.empty(nhalf), np.empty(nhalf)
    for k in range(nhalf):
        zz[k], j, u3[k] = draws(oracle, key, sid, nhalf, k, t, a)
        cj, sk = pos[cbase + j], pos[half * nhalf + k]
        if exact:
            q[k] = [fma(-zz[k], float(cj[d] - sk[d]), float(cj[d])) for d in range(ndim)]
        else:
            q[k] = cj - zz[k] * (cj - sk)
    return q, zz, u3


def accept_lhs(zz, u3, ndim):
    """ln(z^(ndim-1) / u3), z^(ndim-1) as the kernel forms it (a running product)."""
    zp = np.ones_like(zz)
    for _ in range(1, ndim):
        zp = zp * zz
    with np.errstate(all="ignore"):
        return np.log(zp / u3)


def reference_stretch(oracle, om, p0, nsteps, seed, a=2.0, lnprob=None, *, stream_ids=None, iteration0=0, thin=1, lnp0=None,
                      exact=True, full=False):
    """The stretch move of p0 (nchains, nwalkers, ndim) over nsteps steps.

    om: one posterior for all chains or a list of one per chain, evaluated by lnprob(om, theta) (default: the oracle's
    lnprob_batch).  stream_ids: the chains' stream ids (default 0..nchains-1); iteration0: the sampler's step counter at the
    start (a stored run after a burn-in of B steps and reset(): B); lnp0: the lnprob of p0 where the caller knows it (a run
    that continues another).

    Returns (chain (nchains, nsteps, nwalkers, ndim), final lnprob, acceptance counts), the chain of every step; with full=True a
    dict instead: 'chain' -- the stored steps only, (nchains, nstored, nwalkers, ndim), in the device's order --, 'lnp_chain',
    'pos', 'lnp', 'nacc'."""
    nchains, nwalkers, ndim = p0.shape
    nhalf = nwalkers // 2
    pos = np.array(p0, dtype=np.float64)
    oms = list(om) if isinstance(om, (list, tuple)) else [om] * nchains      # one posterior per chain, or one for all
    lnprob = lnprob or oracle.lnprob_batch
    sids = list(range(nchains)) if stream_ids is None else [int(x) for x in stream_ids]
    lnp = np.stack([lnprob(oms[c], pos[c]) for c in range(nchains)]) if lnp0 is None else np.array(lnp0, dtype=np.float64)
    nstored = (nsteps + thin - 1) // thin if full else nsteps
    chain = np.empty((nchains, nstored, nwalkers, ndim))
    lnp_chain = np.empty((nchains, nstored, nwalkers))
    nacc = np.zeros((nchains, nwalkers), dtype=int)
    key = (seed & 0xffffffff, seed >> 32)
    for it in range(nsteps):
        for half in (0, 1):
            t = 2 * (iteration0 + it) + half
            newpos, newlnp = pos.copy(), lnp.copy()
            for c in range(nchains):
                q, zz, u3 = propose(oracle, key, pos[c], half, t, sids[c], a, exact)
                lq = lnprob(oms[c], q)
                lk = lnp[c, half * nhalf:(half + 1) * nhalf]
                with np.errstate(invalid="ignore"):                  # -inf - -inf: NaN, no move
                    acc = accept_lhs(zz, u3, ndim) > lk - lq
                idx = np.arange(half * nhalf, (half + 1) * nhalf)[acc]
                newpos[c, idx] = q[acc]
                newlnp[c, idx] = lq[acc]
                nacc[c, idx] += 1
            pos, lnp = newpos, newlnp
        if not full:
            chain[:, it] = pos
        elif it % thin == 0:
            chain[:, it // thin] = pos
            lnp_chain[:, it // thin] = lnp
    if not full:
        return chain, lnp, nacc
    return {"chain": chain, "lnp_chain": lnp_chain, "pos": pos, "lnp": lnp, "nacc": nacc}


class Arbiter:
    """The reference's unitarity verdict on rows of one BSM model: the oracle's (its 80-bit closed form) outside BAND; inside it
    the reference's own verdict is a property of its libm's last bits, and the host build of the device's
    chain decides (tests/x87_harness.py: x87t_walker_residuals on the model's own tables), independent of the device.

    om: the oracle's model; model: the same posterior compiled by golemflavor_amd (its tables, and its value where the harness
    acquits a row the oracle raised on -- the oracle did not finish those).  Counts what it saw: `nbad` (non-unitary rows by the
    final verdict), `nband`, `nflip` (band rows on which the harness overrules the oracle)."""

    def __init__(self, oracle, om, model, harness=None):
        import x87_harness as H
        self.O, self.om, self.model, self.H = oracle, om, model, H
        self.hx = harness or H.build()
        self.tables = H.model_tables(model)
        self.nbad = self.nband = self.nflip = 0

    def verdict(self, theta, status):
        """(non-unitary (n,) bool, band (n,) bool, acquitted row indices) for rows theta whose oracle status is `status`."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        bad = status == self.O.NON_UNITARY
        band = np.zeros(len(theta), dtype=bool)
        acquit = np.zeros(0, dtype=int)
        inbox = status != self.O.OUT_OF_PRIOR
        self.residual = np.zeros(len(theta))                             # the oracle's residual of every row (0: out of prior)
        if inbox.any():
            res = self.O.unitarity_residual_batch(self.om, theta)
            self.residual = np.where(inbox, res, 0.0)
            band = inbox & (res > BAND[0]) & (res < BAND[1])
        if band.any():
            hbad = self.H.non_unitary(self.H.walker_residuals(self.hx, self.model.desc, self.tables, theta[band]))
            flip = np.flatnonzero(band)[hbad != bad[band]]
            self.nflip += flip.size
            acquit = flip[bad[flip]]                                    # the oracle raised, the harness does not
            bad[band] = hbad
        self.nband += int(band.sum())
        self.nbad += int(bad.sum())
        return bad, band, acquit

    def lnprob(self, om, theta):
        """lnprob with the on_nonunitary='-inf' rule: -inf where the verdict is non-unitary (a reference_stretch `lnprob`)."""
        lq, sq = self.O.lnprob_batch(self.om, theta, want_status=True)
        bad, _, acquit = self.verdict(theta, sq)
        if acquit.size:
            lq[acquit] = self.model.lnprob(np.ascontiguousarray(theta[acquit]))[0]
        return np.where(bad, -np.inf, lq)
