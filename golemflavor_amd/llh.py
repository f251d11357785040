"""The log-posterior callback, GPU-evaluated: drop-in for the callables the reference hands to
emcee (`partial(ln_prob, ...)`: examples/inference.ipynb:356-371, golemflavor/llh.py:121-130,
scripts/mc_unitary.py:134-143, scripts/mc_texture.py:161-170).

`LnProb(theta)` keeps the reference convention for a single walker -- `theta` of length ndim ->
Python float, `-inf` outside the box prior, AssertionError on a length mismatch or on a
non-unitary BSM mixing matrix -- and additionally accepts a whole ensemble `(n, ndim)` ->
`(n,)` array in ONE kernel launch (emcee-3's `vectorize=True` convention), which is what
`golemflavor_amd.mcmc.EnsembleSampler` uses.
"""
import numpy as np

from . import _lib
from . import fr as fr_utils
from .descriptor import compile_model
from .enums import ParamTag, Texture
from .model import Model

__all__ = ["LnProb", "CubeLnProb", "notebook_ln_prob", "tutorial_ln_prob", "bsm_ln_prob", "prior_ln_prob", "lnprior",
           "ln_prob", "triangle_llh", "multi_gaussian", "BinnedMeasurement", "equal_information_smearing", "TabulatedLikelihood"]


def equal_information_smearing(smearing, binning):
    """The per-bin widths that make the energy-resolved likelihood comparable with the flux-averaged one of width `smearing`:
    sigma_k = smearing / sqrt(w_k) with w_k = width_k / (E_max - E_min), the flux average's own weight of bin k (`binning`: the bin
    edges).  Then sum_k w_k^2 sigma_k^2 = smearing^2: the flux-weighted mean of the per-bin measurements has exactly the width the
    flux-averaged likelihood assumes."""
    if not float(smearing) > 0.0 or not np.isfinite(float(smearing)):
        raise ValueError("smearing must be positive and finite")
    b = np.asarray(binning, dtype=np.float64)
    if b.ndim != 1 or len(b) < 2 or not np.all(np.isfinite(b)):
        raise ValueError("binning must be a 1-D array of at least two finite bin edges")
    widths = np.abs(np.diff(b))
    if not np.all(widths > 0.0):
        raise ValueError("every energy bin needs a positive width")
    w = widths / np.abs(b[-1] - b[0])
    return float(smearing) / np.sqrt(w)


class BinnedMeasurement:
    """A measurement per energy bin for the energy-resolved Gaussian likelihood: `fr_bins` (K, 3) the measured
    composition m_k of every bin, `sigma` (K,) its width.  `smearing`: K values are the widths themselves; ONE value is the width
    of the flux-averaged likelihood this one is to be comparable with and needs `binning` (the K + 1 bin edges of the model):
    sigma_k = `equal_information_smearing(smearing, binning)`.  ValueError on a wrong shape, a non-finite composition, a width that
    is not positive or a number of smearings that is neither 1 nor K."""

    def __init__(self, fr_bins, smearing, binning=None):
        f = np.array(fr_bins, dtype=np.float64)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError("fr_bins has shape (K, 3): one composition per energy bin")
        if f.shape[0] > _lib.GF_MAX_BINS:
            raise ValueError("at most %d energy bins" % _lib.GF_MAX_BINS)
        if not np.all(np.isfinite(f)):
            raise ValueError("the measured compositions must be finite")
        K = f.shape[0]
        edges = None
        if binning is not None:
            edges = np.asarray(binning, dtype=np.float64)
            if edges.ndim != 1 or len(edges) != K + 1:
                raise ValueError("%d compositions for a binning of %d bins" % (K, max(len(np.atleast_1d(edges)) - 1, 0)))
        sm = np.atleast_1d(np.asarray(smearing, dtype=np.float64))
        if sm.ndim != 1 or (len(sm) != 1 and len(sm) != K):
            raise ValueError("smearing takes one value (the equal-information rule) or one per energy bin (%d), got %d" % (K, sm.size))
        if not np.all(np.isfinite(sm)) or not np.all(sm > 0.0):
            raise ValueError("every smearing must be positive and finite")
        if len(sm) == 1 and (K > 1 or edges is not None):
            if edges is None:
                raise ValueError("one smearing for %d bins needs the binning: sigma_k = smearing / sqrt(w_k)" % K)
            sigma = equal_information_smearing(float(sm[0]), edges)
        else:
            sigma = sm.copy()
        self.fr_bins = np.ascontiguousarray(f)
        self.sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        self.binning = edges

    @property
    def nbins(self):
        return self.fr_bins.shape[0]

    @classmethod
    def constant(cls, fr, smearing, binning):
        """The same composition `fr` in every bin of `binning` (what a source without new physics gives)."""
        b = np.asarray(binning, dtype=np.float64)
        return cls(np.tile(np.asarray(fr, dtype=np.float64).reshape(1, 3), (len(b) - 1, 1)), smearing, binning=b)

    def __repr__(self):
        return "BinnedMeasurement(nbins=%d)" % self.nbins


class TabulatedLikelihood:
    """A likelihood surface over the flavour triangle: ln L at the (N + 1)(N + 2) / 2 nodes (i, j), 0 <= j <= N - i, of
    the triangular lattice of side N -- node (i, j) is the composition (i, j, N - i - j) / N and lies at values[i (2N + 3 - i) / 2 + j].
    Between the nodes ln L is linear in the triangle of the lattice that holds the composition.  `values`: the flat array, its length
    fixes N.  Every value is finite or -inf and at least one is finite: else ValueError."""

    def __init__(self, values):
        v = np.array(values, dtype=np.float64)
        if v.ndim != 1 or v.size < 3:
            raise ValueError("values is the flat array of the (N + 1)(N + 2) / 2 node values of a table of side N >= 1")
        n = (int(np.sqrt(8 * v.size + 1)) - 3) // 2
        while (n + 1) * (n + 2) // 2 < v.size:
            n += 1
        if (n + 1) * (n + 2) // 2 != v.size:
            raise ValueError("%d values are not (N + 1)(N + 2) / 2 for any side N" % v.size)
        if n > _lib.GF_TABLE_MAX_NSIDE:
            raise ValueError("side %d beyond the largest table side %d" % (n, _lib.GF_TABLE_MAX_NSIDE))
        if np.any(np.isnan(v)) or np.any(v == np.inf):
            raise ValueError("a node value is finite or -inf: NaN or +inf in the table")
        if not np.any(np.isfinite(v)):
            raise ValueError("every node of the table is -inf")
        self.values = np.ascontiguousarray(v)
        self.nside = n

    @staticmethod
    def node_count(nside):
        return (int(nside) + 1) * (int(nside) + 2) // 2

    @staticmethod
    def node_index(nside, i, j):
        """where node (i, j) of a table of side `nside` lies (arrays allowed)"""
        i = np.asarray(i, dtype=np.int64)
        return i * (2 * int(nside) + 3 - i) // 2 + np.asarray(j, dtype=np.int64)

    @staticmethod
    def node_ij(nside):
        """(i, j) of every node in storage order: two int64 arrays"""
        n = int(nside)
        i = np.repeat(np.arange(n + 1), np.arange(n + 1, 0, -1))
        j = np.concatenate([np.arange(n + 1 - k) for k in range(n + 1)])
        return i.astype(np.int64), j.astype(np.int64)

    def node_fr(self):
        """the compositions of the nodes, [n][3] in storage order"""
        i, j = self.node_ij(self.nside)
        n = float(self.nside)
        return np.stack([i / n, j / n, (self.nside - i - j) / n], axis=1)

    @classmethod
    def from_function(cls, f, nside):
        """ln L = f(fr) at every node; f takes the [n][3] compositions of the nodes and returns [n] values"""
        nside = int(nside)
        if nside < 1 or nside > _lib.GF_TABLE_MAX_NSIDE:
            raise ValueError("nside outside 1 .. %d" % _lib.GF_TABLE_MAX_NSIDE)
        i, j = cls.node_ij(nside)
        n = float(nside)
        return cls(np.asarray(f(np.stack([i / n, j / n, (nside - i - j) / n], axis=1)), dtype=np.float64))

    @classmethod
    def from_gaussian(cls, bf, smearing, nside, offset=0.):
        """the Gaussian around `bf` of width `smearing`, node by node with `multi_gaussian`'s arithmetic"""
        return cls.from_function(lambda fr: multi_gaussian(fr, bf, smearing, offset=offset), nside)

    @classmethod
    def from_ternary(cls, d, scale):
        """From the dictionary `plot.heatmap` draws (golemflavor/plot.py:216-228): {(i, j, k): value} with i + j + k = scale, i
        counting fr_e and j fr_mu ((i, j) keys are taken too).  Every node of the lattice must be present."""
        scale = int(scale)
        if scale < 1 or scale > _lib.GF_TABLE_MAX_NSIDE:
            raise ValueError("scale outside 1 .. %d" % _lib.GF_TABLE_MAX_NSIDE)
        v = np.full(cls.node_count(scale), np.nan)
        for key, val in d.items():
            key = tuple(int(x) for x in key)
            if len(key) not in (2, 3):
                raise ValueError("a key is (i, j, k) or (i, j): %r" % (key,))
            i, j = key[0], key[1]
            if i < 0 or j < 0 or i + j > scale or (len(key) == 3 and key[2] != scale - i - j):
                raise ValueError("key %r is no node of a lattice of scale %d" % (key, scale))
            v[int(cls.node_index(scale, i, j))] = float(np.asarray(val, dtype=np.float64))
        missing = int(np.count_nonzero(np.isnan(v)))
        if missing:
            raise ValueError("%d of the %d nodes are missing from the dictionary (or NaN)" % (missing, v.size))
        return cls(v)

    def to_ternary(self):
        """the {(i, j, k): value} dictionary of the table"""
        i, j = self.node_ij(self.nside)
        return {(int(a), int(b), int(self.nside - a - b)): float(x) for a, b, x in zip(i, j, self.values)}

    def save(self, path):
        """the flat values as .npy"""
        with open(path, "wb") as fh:
            np.save(fh, self.values)

    @classmethod
    def load(cls, path):
        return cls(np.load(path, allow_pickle=False))

    def cell(self, fr):
        """(i, j, fu, fv, up, nan) of every composition: the cell the lookup takes (csrc/gf_table.hpp `locate`)"""
        fr = np.atleast_2d(np.asarray(fr, dtype=np.float64))
        N = self.nside
        n = float(N)
        with np.errstate(invalid="ignore", over="ignore"):
            u = fr[:, 0] * n
            v = fr[:, 1] * n
            nan = np.isnan(u) | np.isnan(v)
            u = np.where(nan, 0.0, u)
            v = np.where(nan, 0.0, v)
            u = np.where(u < 0.0, 0.0, np.where(u > n, n, u))
            vmax = n - u
            v = np.where(v < 0.0, 0.0, np.where(v > vmax, vmax, v))
            i = np.minimum(np.floor(u).astype(np.int64), N - 1)
            j = np.minimum(np.floor(v).astype(np.int64), N - 1 - i)
            fu = u - i
            fv = v - j
            up = (fu + fv <= 1.0) | (j == N - 1 - i)
        return i, j, fu, fv, up, nan

    def lnl(self, fr):
        """ln L of the compositions fr (n, 3) (or (3,): a float): the definition restated in numpy, operation by operation in the
        header's order, so that it is the device's value bit for bit"""
        single = np.ndim(fr) == 1
        i, j, fu, fv, up, nan = self.cell(fr)
        N = self.nside
        T = self.values
        a00 = self.node_index(N, i, j)
        a10 = a00 + (N + 1 - i)
        # upward: (i, j), (i + 1, j), (i, j + 1); downward: (i + 1, j + 1), (i, j + 1), (i + 1, j) with 1 - fu, 1 - fv
        ia = np.where(up, a00, a10 + 1)
        ib = np.where(up, a10, a00 + 1)
        ic = np.where(up, a00 + 1, a10)
        ta, tb, tc = T[ia], T[ib], T[ic]
        with np.errstate(invalid="ignore", over="ignore"):
            gu = np.where(up, fu, 1.0 - fu)
            gv = np.where(up, fv, 1.0 - fv)
            out = (ta + gu * (tb - ta)) + gv * (tc - ta)
        out = np.where(np.isneginf(ta) | np.isneginf(tb) | np.isneginf(tc), -np.inf, out)
        out = np.where(nan, np.nan, out)
        return float(out[0]) if single else out

    def __repr__(self):
        return "TabulatedLikelihood(nside=%d)" % self.nside


class LnProb:
    vectorized = True          # tells golemflavor_amd.mcmc.EnsembleSampler to batch the ensemble

    def __init__(self, desc, device=0, on_nonunitary="raise", check_unitarity=True):
        if on_nonunitary not in ("raise", "-inf"):
            raise ValueError("on_nonunitary must be 'raise' or '-inf'")
        self.model = Model(desc, device=device)
        self.ndim = self.model.ndim
        self.on_nonunitary = on_nonunitary
        self.check_unitarity = bool(check_unitarity) and self.model.mode == _lib.GF_MODE_BSM_GAUSS
        self.ncalls = 0
        self.nevals = 0

    def __call__(self, theta):
        single = np.ndim(theta) == 1
        if self.check_unitarity:
            lp, st = self.model.lnprob(theta, want_status=True)
            bad = st == _lib.GF_ST_NON_UNITARY
            if bad.any():
                if self.on_nonunitary == "raise":
                    # reference: AssertionError out of test_unitarity (fr.py:493-498)
                    th = np.atleast_2d(np.asarray(theta, dtype=float))[np.argmax(bad)]
                    raise AssertionError("Matrix is not unitary!\ntheta\n{0}".format(th))
                lp = np.where(bad, -np.inf, lp)
        else:
            lp = self.model.lnprob(theta, want_status=False)
        self.ncalls += 1
        self.nevals += lp.shape[0]
        return float(lp[0]) if single else lp

    def close(self):
        self.model.close()


def notebook_ln_prob(asimov_paramset, llh_paramset, device=0):
    """The posterior of examples/inference.ipynb (cells 21 and 23): lnprior + Gaussian flavor
    likelihood of u_to_fr(angles_to_fr(source angles), angles_to_u(mixing angles)) around the
    Asimov composition.  Smearing = asimov_paramset[first BESTFIT].std (ipynb:333)."""
    bestfit = asimov_paramset.from_tag(ParamTag.BESTFIT)
    bf = fr_utils.angles_to_fr(bestfit.values)                 # ipynb:330
    desc = compile_model(llh_paramset, "SM_GAUSS", bestfit_fr=bf, smearing=bestfit[0].std)
    return LnProb(desc, device=device)


def tutorial_ln_prob(asimov_paramset, llh_paramset, device=0):
    """The posterior of examples/tutorial.ipynb (cells 33 and 35): flat box priors + multi_gaussian(
    angles_to_fr(theta), angles_to_fr(asimov angles), smearing) -- the two flavor angles ARE theta and nothing
    oscillates, which is the Gaussian-likelihood kernel with the identity for a mixing matrix."""
    bestfit = asimov_paramset.from_tag(ParamTag.BESTFIT)
    bf = fr_utils.angles_to_fr(bestfit.values)
    desc = compile_model(llh_paramset, "SM_GAUSS", bestfit_fr=bf, smearing=bestfit[0].std,
                         sm_fixed=(0.0, 1.0, 0.0, 0.0), src_columns=(0, 1))
    return LnProb(desc, device=device)


def bsm_ln_prob(args, asimov_paramset, llh_paramset, smearing=0.02, device=0, binned=None, table=None, **kw):
    """golemflavor/llh.py:121-130 `ln_prob(theta, args, asimov_paramset, llh_paramset)` with the
    GolemFit likelihood replaced by the Gaussian substitute the README sanctions
    (README.md:70-74): multi_gaussian(measured, angles_to_fr(asimov BESTFIT angles), smearing).
    `args` needs: source_ratio, dimension, texture, binning (edges); `args.no_bsm` (fr.py:437-438) is honoured:
    the posterior is then lnprior + the Gaussian around u_to_fr(source_ratio, sm_u) (descriptor.compile_model).
    `binned` (a `BinnedMeasurement`): the posterior is the energy-resolved one, lnprior + the sum over the energy
    bins of multi_gaussian(composition at the bin, m_k, sigma_k); the flux-averaged bestfit and `smearing` are then not read.
    `table` (a `TabulatedLikelihood`): the posterior is lnprior + the table's value at the flux-averaged composition;
    not together with `binned`."""
    if binned is not None and table is not None:
        raise ValueError("binned and table are two likelihoods: give one")
    bf = fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    desc = compile_model(llh_paramset, "BSM_GAUSS", bestfit_fr=bf, smearing=smearing,
                         source_ratio=args.source_ratio, texture=args.texture,
                         dimension=args.dimension, binning=args.binning, no_bsm=bool(getattr(args, "no_bsm", False)))
    f = LnProb(desc, device=device, **kw)
    if binned is not None or table is not None:
        try:
            if binned is not None:
                f.model.set_binned_measurement(binned)
            else:
                f.model.set_table_likelihood(table)
        except BaseException:
            f.close()
            raise
    return f


def prior_ln_prob(llh_paramset, device=0, flat_llh=1.0):
    """scripts/mc_unitary.py:134-143 / mc_texture.py:161-170: lnprior + flat likelihood (1.0)."""
    return LnProb(compile_model(llh_paramset, "PRIOR_ONLY", flat_llh=flat_llh), device=device)


def lnprior(theta, paramset, device=0):
    """golemflavor/llh.py:65-91 for one theta or a batch, GPU-evaluated."""
    f = prior_ln_prob(paramset, device=device, flat_llh=0.0)
    try:
        return f(theta)
    finally:
        f.close()


# ---- the reference's own function names and signatures -------------------------------------------------
# `partial(ln_prob, args=args, asimov_paramset=..., llh_paramset=...)` (scripts/fr.py:182-187) keeps working:
# the bound state is compiled into a device model the first time it is seen and looked up afterwards.
_BOUND = {}
_BOUND_MAX = 64


def _fingerprint(args, asimov_paramset, llh_paramset, smearing):
    """Everything of the bound state the posterior depends on (param *values* are overwritten by theta in the
    reference, llh.py:72-73, so they are not part of it -- except for columns the model keeps fixed)."""
    ps = tuple((p.name, float(p.ranges[0]), float(p.ranges[1]), p.prior.value, float(p.nominal_value),
                None if p.std is None else float(p.std), p.tag.value if hasattr(p.tag, "value") else str(p.tag))
               for p in llh_paramset)
    bf = tuple(float(x) for x in asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    tex = args.texture.value if hasattr(args.texture, "value") else int(args.texture)
    return (ps, bf, tuple(float(x) for x in np.ravel(args.source_ratio)), int(args.dimension), tex,
            tuple(float(x) for x in np.ravel(args.binning)), float(smearing), bool(getattr(args, "no_bsm", False)))


def _bound(args, asimov_paramset, llh_paramset):
    smearing = float(getattr(args, "smearing", 0.02))
    key = _fingerprint(args, asimov_paramset, llh_paramset, smearing)
    f = _BOUND.get(key)
    if f is None:
        if len(_BOUND) >= _BOUND_MAX:                      # oldest first
            _BOUND.pop(next(iter(_BOUND))).close()
        f = _BOUND[key] = bsm_ln_prob(args, asimov_paramset, llh_paramset, smearing=smearing,
                                      device=int(getattr(args, "device", 0)))
    return f


def multi_gaussian(fr, fr_bf, smearing, offset=-320):
    """golemflavor/llh.py:32-54: log(multivariate_normal.pdf(fr, mean=fr_bf, cov=smearing^2 I)) + offset, with
    the reference's underflow to -inf (the pdf is formed in fp64 before the log).  Host closed form for single
    compositions; ensembles go through the model's kernel."""
    d = (np.asarray(fr, dtype=np.float64) - np.asarray(fr_bf, dtype=np.float64)) * np.sqrt(1.0 / (smearing * smearing))
    logpdf = -0.5 * (3 * np.log(2 * np.pi) + 3 * np.log(smearing * smearing) + np.sum(d * d, axis=-1))
    with np.errstate(divide="ignore", under="ignore"):
        return np.log(np.exp(logpdf)) + offset


def triangle_llh(theta, args, asimov_paramset, llh_paramset):
    """golemflavor/llh.py:94-119 with the Gaussian substitute for gf.get_llh (README.md:70-74): the composition
    comes from the device (flux_averaged_BSMu of theta), the Gaussian is applied to it."""
    if np.shape(theta)[-1] != len(llh_paramset):
        raise AssertionError('Length of MCMC scan is not the same as the input '
                             'params\ntheta={0}\nparamset]{1}'.format(theta, llh_paramset))
    f = _bound(args, asimov_paramset, llh_paramset)
    frs, st = f.model.propagate(theta)
    if np.any(st == _lib.GF_ST_NON_UNITARY):
        raise AssertionError("Matrix is not unitary!")
    bf = fr_utils.angles_to_fr(asimov_paramset.from_tag(ParamTag.BESTFIT, values=True))
    out = multi_gaussian(frs, bf, float(getattr(args, "smearing", 0.02)))
    return float(out[0]) if np.ndim(theta) == 1 else out


def ln_prob(theta, args, asimov_paramset, llh_paramset):
    """golemflavor/llh.py:121-130, same name and signature; theta (ndim,) -> float or (n, ndim) -> (n,)."""
    return _bound(args, asimov_paramset, llh_paramset)(theta)


class CubeLnProb:
    """MultiNest-style callback adapter (golemflavor/mn.py:26-45 `lnProb(cube, ndim, n_params, ...)`).

    `mn_paramset` is the scanned subset of `llh_paramset`; the unit cube is mapped onto its ranges,
    theta_i = (hi_i - lo_i) * cube_i + lo_i (mn.py:35-36), the other columns keep their current
    `.value`, and the batch goes to the GPU in one call: a nested sampler can hand over all its
    live-point proposals at once (`cube` of shape (n, ndim)) or one point (shape (ndim,)), as
    MultiNest does.  When `ln_prob` is a device posterior (`LnProb`) whose box for the scanned columns is the
    scanned ranges -- the reference's case: mn_paramset holds the same Param objects -- the map itself runs on
    the device (`gf_lnprob_cube_batch`) and only the cube crosses PCIe; otherwise it is one numpy expression.
    """

    def __init__(self, ln_prob, mn_paramset, llh_paramset):
        self.ln_prob = ln_prob
        names = list(llh_paramset.names)
        self.cols = np.array([names.index(n) for n in mn_paramset.names], dtype=np.intp)
        rng = np.array(mn_paramset.ranges, dtype=np.float64)
        self.lo, self.span = rng[:, 0], rng[:, 1] - rng[:, 0]
        self.base = np.array(llh_paramset.values, dtype=np.float64)
        self.ndim = len(self.cols)
        model = getattr(ln_prob, "model", None)
        box = np.array(llh_paramset.ranges, dtype=np.float64)[self.cols]
        self.on_device = (isinstance(ln_prob, LnProb) and model is not None and model.ndim == len(names)
                          and np.array_equal(box, rng))

    def __call__(self, cube, ndim=None, n_params=None):
        if ndim is not None and ndim != self.ndim:
            raise AssertionError("Length of MultiNest scan paramset is not the same as the input params")
        u = np.asarray([cube[i] for i in range(self.ndim)], dtype=np.float64) if np.ndim(cube) <= 1 and not \
            isinstance(cube, np.ndarray) else np.asarray(cube, dtype=np.float64)
        single = u.ndim == 1
        u = np.atleast_2d(u)[:, :self.ndim]
        if self.on_device:
            f = self.ln_prob
            lp, st = f.model.lnprob_cube(u, self.cols, self.base)
            bad = st == _lib.GF_ST_NON_UNITARY
            if f.check_unitarity and bad.any():
                if f.on_nonunitary == "raise":
                    raise AssertionError("Matrix is not unitary!")
                lp = np.where(bad, -np.inf, lp)
            f.ncalls += 1
            f.nevals += lp.shape[0]
            return float(lp[0]) if single else lp
        theta = np.tile(self.base, (u.shape[0], 1))
        theta[:, self.cols] = self.span * u + self.lo
        out = self.ln_prob(theta)
        return float(out[0]) if single else out
