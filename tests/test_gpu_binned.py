"""GPU: the energy-resolved Gaussian likelihood (csrc/gf_binned.hip, binned_llh in csrc/gf_bsm_device.hpp) -- the bulk
kernel against the device's own per-bin terms and against the reference-generated golden, its launch shapes and the underflow wall,
the refusals, and the nested sampler, the maximiser and the reweight path on a model that carries a measurement per energy bin."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from binned_ref import binned_bound, binned_lnl_host, multi_gaussian_host
from common import BIN_EDGES, TEX_BY_VALUE, uniform_theta
from golemflavor_amd import _lib, llh, nested
from golemflavor_amd import configs as Cf
from golemflavor_amd import fr as fr_utils
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd import profile_llh as P
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import Model
from golemflavor_amd.param import Param, ParamSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET = -320.0
SRC = (1., 2., 0.)


@pytest.fixture(scope="module")
def gs():
    with np.load(os.path.join(ROOT, "tests", "golden", "golden_spectrum.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def paramset_of(width, dim):
    """7: the texture posterior; 12: the bulk benchmark's posterior; 11: the NP mixing angles sampled (the generic row width)"""
    if width == 7:
        return Cf.texture_paramset(dim), None
    if width == 12:
        return Cf.fr_paramsets(dim, (0.4444, 0.0))[1], None
    t = list(Cf.texture_paramset(dim))
    mm = [Param(name="np_%s" % k, value=0.5, ranges=r, tag=ParamTag.MMANGLES)
          for k, r in (("s12", [0., 1.]), ("c13", [0., 1.]), ("s23", [0., 1.]), ("dcp", [0., 2 * np.pi]))]
    return ParamSet(t[:6] + mm + t[6:]), Texture.NONE


def bsm_model(width, dim, tex, binning=BIN_EDGES, source=SRC):
    ps, forced = paramset_of(width, dim)
    kw = dict(texture=forced or tex, dimension=dim, binning=np.asarray(binning, dtype=float), source_ratio=source, bestfit_fr=(1 / 3,) * 3,
              smearing=0.02)
    return Model(compile_model(ps, "BSM_GAUSS", **kw)), ps, kw


def a_measurement(K, binning, seed=3, smearing=0.02):
    """compositions well away from what the textures give, widths by the equal-information rule (0.04 to 0.25 on the default bins)"""
    rng = np.random.default_rng(seed)
    return llh.BinnedMeasurement(rng.dirichlet((6, 5, 4), size=K), smearing, binning=binning)


def host_lnprior(oracle, ps, theta):
    om = oracle.make_model(ps, "PRIOR_ONLY")
    return np.array([oracle.lnprior(om, t) for t in theta])


def lnprob_device(m, th, layout=_lib.GF_LAYOUT_AOS, want_status=False, guard=64):
    """lnprob_device into a buffer with `guard` sentinel doubles behind the output: (lnprob, status or None); the guard is checked"""
    n = th.shape[0]
    host = np.full(n + guard, -7.25)
    src = th if layout == _lib.GF_LAYOUT_AOS else np.ascontiguousarray(th.T)
    d_out, d_th = m.alloc(host.nbytes).upload(host), m.alloc(src.nbytes).upload(np.ascontiguousarray(src))
    sentinel = np.full(n + guard, 0x5a5a5a5a, dtype=np.int32)
    d_st = m.alloc(sentinel.nbytes).upload(sentinel) if want_status else None
    try:
        m.lnprob_device(d_th.ptr, n, d_out.ptr, None, d_st.ptr if want_status else None, layout=layout)
        m.sync()
        out = d_out.download((n + guard,))
        st = d_st.download((n + guard,), dtype=np.int32) if want_status else None
    finally:
        for b in (d_out, d_th, d_st):
            if b is not None:
                b.free()
    assert np.all(out[n:] == -7.25), "guard words behind lnprob overwritten"
    if want_status:
        assert np.all(st[n:] == 0x5a5a5a5a), "guard words behind status overwritten"
        return out[:n], st[:n]
    return out[:n], None


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def scale_rows(ps, n, rng, dim, lo=None, hi=None):
    """rows over the seeds' box with the scale spread over the range the scans cover, below where the reference starts raising"""
    th = uniform_theta(ps, n, rng, seeds=True)
    b = Cf.SCALE_BOUNDARIES[dim]
    th[:, -1] = rng.uniform(b[0] if lo is None else lo, (b[0] + 0.6 * (b[1] - b[0])) if hi is None else hi, n)
    return th


# ---- 1. against the device's own per-bin terms ------------------------------------------------------------------------------------
def check_against_own_terms(oracle, m, ps, th, meas, layouts=(_lib.GF_LAYOUT_AOS, _lib.GF_LAYOUT_SOA)):
    lp0, st0 = m.lnprob(th, want_status=True)                           # the same model without the measurement
    fr_bins = m.propagate_bins(th, want_status=False)
    m.set_binned_measurement(meas)
    assert m.is_binned
    lp, st = m.lnprob(th, want_status=True)
    assert np.array_equal(st, st0)
    lnl, terms = binned_lnl_host(fr_bins, meas, OFFSET, return_terms=True)
    lpr = host_lnprior(oracle, ps, th)
    want = lpr + lnl
    ok = st == _lib.GF_ST_OK
    assert ok.sum() >= 0.5 * len(th)
    bound = binned_bound(terms, lpr, OFFSET)
    err = np.abs(lp[ok] - want[ok])
    print("own terms: %d rows, worst |diff| / bound = %.3f (worst diff %.3e)" % (ok.sum(), np.max(err / bound[ok]), err.max()))
    assert np.all(np.isfinite(want[ok])) and np.all(err <= bound[ok])
    # a row the reference would have raised on: the value the flux-averaged path writes (NaN); outside the box: -inf
    assert np.all(np.isnan(lp[st == _lib.GF_ST_NON_UNITARY])) and np.all(np.isnan(lp0[st0 == _lib.GF_ST_NON_UNITARY]))
    assert np.all(lp[st == _lib.GF_ST_OUT_OF_PRIOR] == -np.inf)
    # without a status array, and both layouts on device buffers: the same bits for the rows with a value
    plain = m.lnprob(th, want_status=False)
    assert same_bits(plain[ok], lp[ok])
    for layout in layouts:
        d, dst = lnprob_device(m, th, layout, want_status=True)
        assert np.array_equal(dst, st) and same_bits(d[ok], lp[ok])
        assert same_bits(lnprob_device(m, th, layout)[0][ok], lp[ok])
    return lp, st


def test_against_own_terms_golden_rows(gs, oracle):
    """Model.lnprob of a binned model against lnprior + binned_lnl_host(Model.propagate_bins(theta), meas) on the golden's rows
    (7 columns; every texture and dimension the golden holds).

    The bound is (K + 4) 2^-52 S with S = sum_k |term_k| + |offset| + |lnprior|.  Both sides start from the same fr_k bit for
    bit.  The sum chain is K - 1 adds of terms (the first add, to 0.0, is exact), one of the offset and one of the prior: K + 1
    roundings, each at most 2^-53 of a partial sum that never exceeds S, together (K + 1) / 2 2^-52 S.  That is the part the
    device and the restatement share operation for operation.  Inside a term they differ in form: the device takes
    fma(mh_k, r2_k, k_k), r2_k by one product and two fmas and mh_k = -0.5 inv_smear^2 (4 roundings ahead of the one of the
    fma), the restatement, which is held to the oracle bit for bit, -0.5 (c0 + sum ((fr - m) scale)^2) (5 ahead of the last).
    k_k = -0.5 c0 is the same number on both sides, so a term differs by at most 9 2^-53 maha_k / 2 + 2 2^-53 |term_k|, and with
    maha_k / 2 <= |term_k| + |k_k| by at most 5.5 2^-52 |term_k| + 4.5 2^-52 |k_k|.  The widths used here keep |k_k| < 16 =
    |offset| / 20, so K <= 20 bins add at most 5.5 2^-52 S.  The worst case of every rounding at once is therefore
    ((K + 1) / 2 + 5.5) 2^-52 S: inside the bound for K >= 4, and up to 2.5 2^-52 S beyond it for K <= 3, where the bound
    stands as set and leaves no room for all 11 roundings of a term to fall the same way."""
    seen = set()
    for ci, (dim, texv) in enumerate(gs["configs"]):
        tex = TEX_BY_VALUE[int(texv)]
        seen.add((int(dim), tex))
        m, ps, _ = bsm_model(7, int(dim), tex, binning=gs["binning"], source=tuple(gs["source"]))
        with m:
            check_against_own_terms(oracle, m, ps, gs["theta"][ci], a_measurement(20, gs["binning"], seed=ci))
    print("golden configs:", sorted((d, t.name) for d, t in seen))


@pytest.mark.parametrize("width,dim,tex", [(7, 6, Texture.OEU), (7, 6, Texture.OET), (7, 3, Texture.OUT), (7, 3, Texture.OEU),
                                           (12, 6, Texture.OET), (12, 3, Texture.OUT), (11, 3, Texture.NONE), (11, 6, Texture.NONE)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_against_own_terms_widths_textures_dimensions(oracle, width, dim, tex):
    """The same check on 300 rows of every row width the kernel is compiled for (7, 12, generic), textures OEU / OET / OUT (and the
    sampled NP angles), dimensions 3 and 6, rows and columns; the scale reaches into the region where the reference raises, so the
    three statuses occur."""
    rng = np.random.default_rng(100 * width + dim)
    m, ps, _ = bsm_model(width, dim, tex)
    with m:
        b = Cf.SCALE_BOUNDARIES[dim]
        th = scale_rows(ps, 300, rng, dim, hi=b[1])
        th[::37, 0] = 2.0                                                # outside the box
        check_against_own_terms(oracle, m, ps, th, a_measurement(20, BIN_EDGES, seed=width))


# ---- 2. against the reference ---------------------------------------------------------------------------------------------------------
def test_against_the_reference_per_bin_compositions(gs, oracle):
    """The golden's reference-generated per-bin compositions in place of the device's: lnprior + binned_lnl_host(fr_ref) within
    sum_k (|fr_k - m_k|_1 / sigma_k^2) tol_k, tol_k the composition parity bar in force for the pair (README, "BSM parity bar"):
    1e-10 against the reference's value where the reference is itself accurate (its |U|^2 within 1e-12 of the exact one, the
    criterion of test_gpu_spectrum.py), 1e-11 against the 60-digit exact value elsewhere."""
    worst = 0.0
    nrows = 0
    for ci, (dim, texv) in enumerate(gs["configs"]):
        meas = a_measurement(20, gs["binning"], seed=10 + ci)
        m, ps, _ = bsm_model(7, int(dim), TEX_BY_VALUE[int(texv)], binning=gs["binning"], source=tuple(gs["source"]))
        th = gs["theta"][ci]
        with m:
            m.set_binned_measurement(meas)
            lp, st = m.lnprob(th, want_status=True)
        clean = (gs["ok"][ci] == 1) & (np.abs(gs["abs2_diff"][ci]).max(axis=(2, 3)) < 1e-12)          # (12, 20)
        ref = np.where(clean[..., None], gs["fr_ref"][ci], gs["fr_exact"][ci])
        tol = np.where(clean, 1e-10, 1e-11)
        want = host_lnprior(oracle, ps, th) + binned_lnl_host(ref, meas, OFFSET)
        bound = np.sum(np.abs(ref - meas.fr_bins[None]).sum(axis=-1) / meas.sigma[None] ** 2 * tol, axis=1)
        rows = (st == _lib.GF_ST_OK) & (gs["flux_status"][ci] == 0)
        nrows += int(rows.sum())
        assert np.all(np.isfinite(want[rows]))
        ratio = np.abs(lp[rows] - want[rows]) / bound[rows]
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (ci, ratio.max())
    print("against the reference: %d rows, worst |diff| / bound = %.3e" % (nrows, worst))
    assert nrows >= 24


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 20, 64])
def test_shapes_rows_and_bins(K):
    """n in {1, 63, 64, 65, 129} at K energy bins, rows and columns, with and without a status array: a row's value is the same bits
    alone and inside any batch, and the guard words behind the outputs are intact."""
    edges = np.geomspace(BIN_EDGES[0], BIN_EDGES[-1], K + 1)
    rng = np.random.default_rng(K)
    m, ps, _ = bsm_model(7, 6, Texture.OET, binning=edges)
    with m:
        assert m.nbins == K
        th = scale_rows(ps, 129, rng, 6)
        th[5, 1] = -1.0
        m.set_binned_measurement(a_measurement(K, edges, seed=K))
        full, fst = lnprob_device(m, th, want_status=True)
        assert np.isfinite(full[fst == 0]).all() and (fst == 0).sum() >= 100 and fst[5] == _lib.GF_ST_OUT_OF_PRIOR and full[5] == -np.inf
        for n in (1, 63, 64, 65, 129):
            for layout in (_lib.GF_LAYOUT_AOS, _lib.GF_LAYOUT_SOA):
                got, st = lnprob_device(m, th[:n], layout, want_status=True)
                assert same_bits(got, full[:n]) and np.array_equal(st, fst[:n]), (K, n, layout)
                assert same_bits(lnprob_device(m, th[:n], layout)[0], full[:n]), (K, n, layout)
        for i in (0, 63, 64, 128):
            assert same_bits(lnprob_device(m, th[i:i + 1])[0], full[i:i + 1])


@pytest.mark.parametrize("layout", [_lib.GF_LAYOUT_AOS, _lib.GF_LAYOUT_SOA], ids=["rows", "columns"])
def test_one_batch_past_one_pass_of_the_grid(layout):
    """gf_internal_pass_items + 65 rows in one launch: the kernel's stride loop goes round, a ragged last tile included; 129 base
    rows repeated, every copy the bits of the small batch."""
    rng = np.random.default_rng(9)
    m, ps, _ = bsm_model(7, 6, Texture.OET)
    with m:
        base = scale_rows(ps, 129, rng, 6)
        m.set_binned_measurement(a_measurement(20, BIN_EDGES, seed=9))
        small = lnprob_device(m, base)[0]
        n = _lib.pass_items(m._h) + 65
        idx = np.arange(n) % 129
        got = lnprob_device(m, np.ascontiguousarray(base[idx]), layout)[0]
        assert np.isfinite(small).all() and same_bits(got, small[idx])


# ---- 4. the underflow wall -------------------------------------------------------------------------------------------------------------
def test_underflow_wall(oracle):
    """One bin's width is chosen on the host so that its logpdf lies in the subnormal band (-745.13, -708.40) for some rows and
    below it for others: the first kind carries oracle.multi_gaussian's quantised value in that term, the second is -inf with
    status OK.  Where the inputs land is checked with the oracle before anything is asserted of the device."""
    rng = np.random.default_rng(41)
    edges = np.geomspace(BIN_EDGES[0], BIN_EDGES[-1], 4)
    m, ps, _ = bsm_model(7, 6, Texture.OET, binning=edges)
    with m:
        th = scale_rows(ps, 64, rng, 6)
        fr_bins = m.propagate_bins(th, want_status=False)
        mk = np.array([[1 / 3, 1 / 3, 1 / 3], [0.9, 0.05, 0.05], [1 / 3, 1 / 3, 1 / 3]])
        r2 = np.sum((fr_bins[:, 1, :] - mk[1]) ** 2, axis=1)
        # sigma with logpdf = -726 at the median distance: -0.5 (3 log 2 pi + 6 log sigma) - r2 / (2 sigma^2), by bisection
        lo, hi = 1e-4, 1.0
        for _ in range(200):
            mid = np.sqrt(lo * hi)
            v = -0.5 * (3 * np.log(2 * np.pi) + 6 * np.log(mid)) - np.median(r2) / (2 * mid * mid)
            lo, hi = (mid, hi) if v < -726.0 else (lo, mid)
        meas = llh.BinnedMeasurement(mk, [0.3, lo, 0.3])
        t1 = np.array([oracle.multi_gaussian(fr_bins[i, 1], mk[1], meas.sigma[1], 0.0) for i in range(len(th))])
        logpdf = -0.5 * (3 * np.log(2 * np.pi) + 6 * np.log(meas.sigma[1])) - r2 / (2 * meas.sigma[1] ** 2)
        band = np.isfinite(t1) & (logpdf > -745.0) & (logpdf < -708.5)
        below = (t1 == -np.inf) & (logpdf < -745.3)
        print("underflow wall: %d rows in the band, %d below, %d above" % (band.sum(), below.sum(), (logpdf > -708.3).sum()))
        assert band.sum() >= 3 and below.sum() >= 3
        # the band's values are quantised: log of a whole number of subnormal ulps, far from the logpdf itself
        assert np.all(np.abs(t1[band] - logpdf[band]) > 1e-9) or np.any(np.abs(t1[band] - logpdf[band]) > 1e-6)
        m.set_binned_measurement(meas)
        lp, st = m.lnprob(th, want_status=True)
        assert np.all(st == _lib.GF_ST_OK)
        lnl, terms = binned_lnl_host(fr_bins, meas, OFFSET, return_terms=True)
        assert np.array_equal(terms[:, 1], t1)
        lpr = host_lnprior(oracle, ps, th)
        assert np.all(lp[below] == -np.inf)
        fin = np.isfinite(t1)
        bound = binned_bound(terms[fin], lpr[fin], OFFSET)
        err = np.abs(lp[fin] - (lpr + lnl)[fin])
        assert np.all(err <= bound), (err.max(), bound.min())
        # ... which the unquantised logpdf would miss
        naive = lpr + ((terms[:, 0] + logpdf) + terms[:, 2]) + OFFSET
        assert np.any(np.abs(lp[band] - naive[band]) > 1e-6)
        # the same through the device buffers, rows and columns
        for layout in (_lib.GF_LAYOUT_AOS, _lib.GF_LAYOUT_SOA):
            assert same_bits(lnprob_device(m, th, layout)[0], lp)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def raw_set(m, f, sg):
    f, sg = np.ascontiguousarray(f, dtype=np.float64), np.ascontiguousarray(sg, dtype=np.float64)
    return _lib.lib().gf_model_set_binned_measurement(m._h, int(f.shape[0]), f.ctypes.data_as(_lib._dp), sg.ctypes.data_as(_lib._dp))


def test_refusals_leave_the_model_usable():
    L = _lib.lib()
    rng = np.random.default_rng(2)
    ang = fr_utils.fr_to_angles(fr_utils.u_to_fr((1, 0, 0), fr_utils.NUFIT_U))
    asimov, nps = Cf.notebook_paramsets(ang)
    good_f, good_s = np.full((20, 3), 1 / 3), np.full(20, 0.05)
    # a model without energy bins: SM and prior-only
    for mode in ("SM_GAUSS", "PRIOR_ONLY"):
        with Model(compile_model(nps, mode, bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02)) as sm:
            th = uniform_theta(nps, 50, rng)
            before = sm.lnprob(th, want_status=False)
            assert raw_set(sm, good_f, good_s) == _lib.GF_ERR_UNSUPPORTED
            assert L.gf_model_is_binned(sm._h) == 0 and not sm.is_binned
            with pytest.raises(_lib.GolemHipError) as e:
                sm.set_binned_measurement(llh.BinnedMeasurement(good_f, good_s))
            assert e.value.code == _lib.GF_ERR_UNSUPPORTED
            assert same_bits(sm.lnprob(th, want_status=False), before)
    m, ps, _ = bsm_model(7, 6, Texture.OET)
    other, _, _ = bsm_model(7, 6, Texture.OET)
    with m, other:
        th = scale_rows(ps, 100, rng, 6)
        before = m.lnprob(th, want_status=False)
        bad_f, bad_s = good_f.copy(), good_s.copy()
        bad_f[4, 2] = np.nan
        bad_s[7] = 0.0
        for f, s in ((good_f[:19], good_s[:19]), (np.full((21, 3), 1 / 3), np.full(21, 0.05)), (bad_f, good_s), (good_f, bad_s),
                     (good_f, -good_s), (good_f, np.where(np.arange(20) == 3, np.inf, good_s))):
            assert raw_set(m, f, s) == _lib.GF_ERR_INVALID_ARG
            assert L.gf_model_is_binned(m._h) == 0
        assert L.gf_model_set_binned_measurement(m._h, 20, None, None) == _lib.GF_ERR_INVALID_ARG
        assert L.gf_model_is_binned(None) == -1
        assert same_bits(m.lnprob(th, want_status=False), before)
        # a run set is binned or it is not
        m.set_binned_measurement(llh.BinnedMeasurement(good_f, good_s))
        binned = m.lnprob(th, want_status=False)
        assert not same_bits(binned, before)
        cols = np.arange(6, dtype=np.int32)
        base = np.tile(np.array(ps.values, dtype=np.float64), (2, 1))
        hs = (C.c_void_p * 2)(m._h, other._h)
        for create, tail in ((L.gf_nested_create, (64, 8, 5, 1, 0)), (L.gf_simplex_create, (4, 64, 1, 0))):
            h = C.c_void_p()
            rc = create(hs, 2, 6, cols.ctypes.data_as(_lib._ip), base.ctypes.data_as(_lib._dp), *tail, C.byref(h))
            assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
            assert b"binned" in L.gf_last_hip_error()
        # the ensemble sampler never samples the flux-averaged posterior of a binned model
        for fn, arg in ((L.gf_sampler_create, m._h), (L.gf_sampler_create_multi, (C.c_void_p * 2)(other._h, m._h))):
            h = C.c_void_p()
            rc = fn(arg, 1, 32, 5, 2.0, C.byref(h)) if fn is L.gf_sampler_create else fn(arg, 2, 32, 5, 2.0, C.byref(h))
            assert rc == _lib.GF_ERR_UNSUPPORTED and not h.value
            assert b"binned" in L.gf_last_hip_error()
        with pytest.raises(_lib.GolemHipError) as e:
            mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=1)
        assert e.value.code == _lib.GF_ERR_UNSUPPORTED
        # the models of a set share device, ndim and mode: the sampler names the model that differs, a run set the rule
        with Model(compile_model(nps, "SM_GAUSS", bestfit_fr=fr_utils.angles_to_fr(asimov.values), smearing=0.02)) as sm:
            differ = (C.c_void_p * 2)(other._h, sm._h)
            h = C.c_void_p()
            rc = L.gf_sampler_create_multi(differ, 2, 16, 5, 2.0, C.byref(h))
            assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
            assert b"gf_sampler_create_multi: model 1 differs from model 0 in device, ndim or mode" in L.gf_last_hip_error()
            for create, tail in ((L.gf_nested_create, (64, 8, 5, 1, 0)), (L.gf_simplex_create, (4, 64, 1, 0))):
                rc = create(differ, 2, 6, cols.ctypes.data_as(_lib._ip), base.ctypes.data_as(_lib._dp), *tail, C.byref(h))
                assert rc == _lib.GF_ERR_INVALID_ARG and not h.value
                assert b"every model must share device, ndim and mode with model 0" in L.gf_last_hip_error()
        # both models are what they were
        assert same_bits(m.lnprob(th, want_status=False), binned)
        assert same_bits(other.lnprob(th, want_status=False), before)
        # ... and a measurement can be replaced
        m.set_binned_measurement(llh.BinnedMeasurement(good_f, 2 * good_s))
        assert m.is_binned and not same_bits(m.lnprob(th, want_status=False), binned)


# ---- 6. the nested sampler -------------------------------------------------------------------------------------------------------------
def sens_args(texture=Texture.OET):
    return argparse.Namespace(source_ratio=fr_utils.normalize_fr((0., 1., 0.)), dimension=6, texture=texture,
                              binning=Cf.default_bin_edges(), smearing=0.02, injected_ratio=fr_utils.normalize_fr((1., 1., 1.)))


SCALES = np.array([-100.0, -45.0])


def sens_measurement(asimov):
    """what `sens --energy-resolved` fits, moved off the null truth so that the two scales differ"""
    bf = fr_utils.angles_to_fr(asimov.from_tag(ParamTag.BESTFIT, values=True))
    f = np.tile(np.asarray(bf, dtype=np.float64), (20, 1))
    f[12:] = (0.30, 0.36, 0.34)
    return llh.BinnedMeasurement(f, 0.05, binning=Cf.default_bin_edges())


def nested_run(binned, lpw=None):
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    old = os.environ.get("GF_NESTED_LPW")
    try:
        if lpw is not None:
            os.environ["GF_NESTED_LPW"] = lpw
        res = nested.evidence_scan(args, asimov, ps, SCALES, run_ids=np.arange(2), nlive=64, batch=8, walks=10, seed=7, tol=0.5,
                                   binned=sens_measurement(asimov) if binned else None, return_sampler=True, on_nonunitary="-inf")
    finally:
        if lpw is not None:
            os.environ.pop("GF_NESTED_LPW", None)
            if old is not None:
                os.environ["GF_NESTED_LPW"] = old
    return res


def close_run(res):
    res["sampler"].close()
    for m in res["models"]:
        m.close()


def test_nested_dead_points_equal_the_bulk_lnprob():
    """Two scales, nlive 64: every dead point's stored lnL is Model.lnprob of the same theta bit for bit -- the walk kernel's binned
    instance against the bulk kernel.

    What it holds in place: a run set maps the cube onto theta with the product and the sum each rounded, as the host and
    k_cube_to_theta do (cube_to_theta, gf_cube_runs.hpp).  With a fused multiply-add, which every instance but the binned one once
    had, a scanned coordinate is one ulp off the host's theta now and then, and 44 of 1096 and 34 of 1072 dead points of these two
    runs then differed from the bulk lnprob of the theta the host forms, by up to 38 and 148 ulps.  test_gpu_cube_runs.py holds the
    same for the other instances, on boxes that see the map far more often than these."""
    res = nested_run(True)
    try:
        for r, m in enumerate(res["models"]):
            assert m.is_binned
            d = res["sampler"].dead(r)
            lp, st = m.lnprob(d["theta"], want_status=True)
            assert len(lp) >= 64 + 8 * 20
            ok = st == _lib.GF_ST_OK
            assert ok.sum() >= len(lp) - 64                              # at most some of the first live points are not
            diff = d["lnl"][ok] != lp[ok]
            ulps = np.abs(d["lnl"][ok].view(np.int64) - lp[ok].view(np.int64))
            print("run %d: %d points, %d differ from the bulk lnprob, largest %d ulps" % (r, ok.sum(), diff.sum(), ulps.max()))
            assert np.all(d["lnl"][~ok] == -np.inf)
            assert same_bits(d["lnl"][ok], lp[ok]), (r, int(diff.sum()), int(ulps.max()))
    finally:
        close_run(res)


def test_nested_evidence_of_a_binned_model_and_the_lane_override():
    """lnz is finite and not the flux-averaged run's; forcing 4 or 16 lanes through the existing override changes nothing -- the
    binned instance runs at one lane -- and the dead points stay the bulk lnprob's bit for bit under it."""
    res = nested_run(True)
    try:
        assert np.all(np.isfinite(res["lnz"])) and np.all(res["niter"] >= 20) and np.all(res["niter"] <= 20000), (res["lnz"], res["niter"])
        for r, m in enumerate(res["models"]):
            d = res["sampler"].dead(r)
            lp, st = m.lnprob(d["theta"], want_status=True)
            ok = st == _lib.GF_ST_OK
            assert ok.sum() >= len(lp) - 64 and same_bits(d["lnl"][ok], lp[ok])
        dead0 = res["sampler"].dead(0)["lnl"]
    finally:
        close_run(res)
    flux = nested_run(False)
    try:
        assert np.all(np.isfinite(flux["lnz"]))
        # another likelihood, another evidence: different at every scale (how far apart is not this test's to say -- at the null
        # scale the two happen to lie within a few of their own errors of each other)
        assert np.all(flux["lnz"] != res["lnz"]), (flux["lnz"], res["lnz"])
        assert np.all(flux["max_lnl"] != res["max_lnl"])
    finally:
        close_run(flux)
    for lpw in ("4", "16"):
        again = nested_run(True, lpw=lpw)
        try:
            assert same_bits(again["lnz"], res["lnz"]) and np.array_equal(again["niter"], res["niter"])
            assert same_bits(again["sampler"].dead(0)["lnl"], dead0)
        finally:
            close_run(again)


# ---- 7. the maximiser ------------------------------------------------------------------------------------------------------------------
def test_profile_scan_on_a_binned_model():
    """profile_scan(..., binned=meas) on two scales: max_lnl is Model.lnprob(argmax) bit for bit, and no lower than the best of
    4096 uniform points of the scanned cube evaluated in bulk."""
    args = sens_args()
    asimov, ps = Cf.sens_paramsets(6, (1., 1., 1.))
    meas = sens_measurement(asimov)
    res = P.profile_scan(args, asimov, ps, SCALES, run_ids=np.arange(2), nstarts=4, nseed=512, seed=3, binned=meas, on_nonunitary="-inf",
                         return_maximizer=True)
    try:
        assert np.all(np.isfinite(res["max_lnl"]))
        rng = np.random.default_rng(17)
        names = list(ps.names)
        cols = [i for i in range(len(names)) if names[i] != "logLam"]
        for r, m in enumerate(res["models"]):
            assert m.is_binned
            again = m.lnprob(res["argmax_theta"][r:r + 1], want_status=False)
            assert same_bits(again, res["max_lnl"][r:r + 1]), (r, again, res["max_lnl"][r])
            lo, hi = np.asarray(m.desc.lo)[cols], np.asarray(m.desc.hi)[cols]
            th = np.tile(res["argmax_theta"][r], (4096, 1))
            th[:, cols] = (hi - lo) * rng.uniform(size=(4096, len(cols))) + lo
            lp, st = m.lnprob(th, want_status=True)
            best = np.max(lp[(st == _lib.GF_ST_OK) & np.isfinite(lp)])
            print("scale %g: max_lnl %.6f, best of 4096 uniform points %.6f" % (SCALES[r], res["max_lnl"][r], best))
            assert res["max_lnl"][r] >= best
        flux = P.profile_scan(args, asimov, ps, SCALES, run_ids=np.arange(2), nstarts=4, nseed=512, seed=3, on_nonunitary="-inf")
        assert np.all(flux["max_lnl"] != res["max_lnl"])
    finally:
        res["maximizer"].close()
        for m in res["models"]:
            m.close()


# ---- 8. the reweight path --------------------------------------------------------------------------------------------------------------
def test_reweight_a_flux_averaged_chain_to_the_binned_model():
    """The reweight contract with a binned model as the target: lnw = binned.lnprob(rows) - stored lnprob, bit for bit."""
    rng = np.random.default_rng(12)
    m, ps, _ = bsm_model(7, 6, Texture.OET)
    target, _, _ = bsm_model(7, 6, Texture.OET)
    with m, target:
        target.set_binned_measurement(a_measurement(20, BIN_EDGES, seed=5, smearing=0.05))
        p0 = scale_rows(ps, 32, rng, 6, lo=-50.0, hi=-42.0)
        s = mcmc_utils.DeviceEnsembleSampler(32, 7, m, seed=5)
        s.on_nonunitary = "-inf"
        try:
            s.run_mcmc(p0, 40)
            c, lp0, _ = s._fetch(chain=True, lnprob=True)
            rows, lp0 = c.reshape(-1, 7), lp0.reshape(-1)
            assert rows.shape == (1280, 7)
            r = s.reweight([target], on_nonunitary="-inf")
            lnw = r.lnw(0)[0]
            lt, st = target.lnprob(rows, want_status=True)
            keep = np.isfinite(lp0) & (st == _lib.GF_ST_OK) & np.isfinite(lt)
            assert keep.sum() >= 1000
            assert same_bits(lnw[keep], lt[keep] - lp0[keep])
            assert np.all(lnw[~keep] == -np.inf)
            assert r.summary()["ess"][0] > 1.0
        finally:
            s.close()


# ---- 9. no regression by construction --------------------------------------------------------------------------------------------------
def test_a_model_without_a_measurement_is_untouched():
    """A model without a measurement gives bitwise the lnprob (and status, and composition) it gave before the new entry points were
    called on another model of the same process -- which is also what it gives next to a binned twin."""
    rng = np.random.default_rng(77)
    plain, ps, _ = bsm_model(7, 6, Texture.OEU)
    with plain:
        th = scale_rows(ps, 400, rng, 6, hi=Cf.SCALE_BOUNDARIES[6][1])
        lp0, fr0, st0 = plain.lnprob(th, want_fr=True, want_status=True)
        cube = rng.uniform(size=(200, 6))
        cb0 = plain.lnprob_cube(cube, np.arange(6), np.array(ps.values, dtype=float))
        twin, _, _ = bsm_model(7, 6, Texture.OEU)
        with twin:
            twin.set_binned_measurement(a_measurement(20, BIN_EDGES, seed=1))
            tl, tf, ts = twin.lnprob(th, want_fr=True, want_status=True)
            assert not plain.is_binned and twin.is_binned
            lp1, fr1, st1 = plain.lnprob(th, want_fr=True, want_status=True)
            cb1 = plain.lnprob_cube(cube, np.arange(6), np.array(ps.values, dtype=float))
            tc = twin.lnprob_cube(cube, np.arange(6), np.array(ps.values, dtype=float))
        assert same_bits(lp1, lp0) and same_bits(fr1, fr0) and np.array_equal(st1, st0)
        assert same_bits(cb1[0], cb0[0]) and np.array_equal(cb1[1], cb0[1])
        # the twin: same statuses, same flux-averaged composition (propagation does not see the measurement), another lnprob
        assert np.array_equal(ts, st0) and same_bits(tf, fr0) and np.array_equal(tc[1], cb0[1])
        ok = st0 == _lib.GF_ST_OK
        assert ok.sum() >= 50 and np.all(tl[ok] != lp0[ok])
        assert {int(v) for v in np.unique(st0)} >= {_lib.GF_ST_OK, _lib.GF_ST_NON_UNITARY}
