"""GPU: the post-processing outputs against independent references.

  * k_flavor_hist (gf_flavor_histogram, gf_flavor_histogram_device, gf_sampler_postprocess_with) against np.histogramdd
    of the same float64 compositions (plot.py:365-370): at every edge of np.linspace(0, 1, nb + 1) and the doubles on both
    sides of it, on each axis in turn and on all three at once, at 0, -0, 1 and past [0, 1], NaN and inf; the documented
    `+=` of the device entry point and its argument checks; 2^25 + 3 atomic adds on one cell and on two;
  * the Philox4x32-10 stream of k_haar against the published known answer of counter (0, 0, 0, 0), key (0, 0);
  * the Haar draws against Haar-random unitaries built independently: QR of complex Gaussian matrices."""
import ctypes as C

import numpy as np
import pytest

from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd import mcmc as mcmc_utils
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

EDGE_NBINS = list(range(1, 161)) + [255, 256, 257, 384, 511, 512]      # 512^3 counts: 1 GiB, the largest size used here


@pytest.fixture(scope="module")
def model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    yield m
    m.close()


def reference_hist(fr, nb):
    want, _ = np.histogramdd(np.asarray(fr, dtype=np.float64).reshape(-1, 3), bins=(nb, nb, nb), range=((0, 1),) * 3)
    return want.astype(np.uint64)


def edge_values(nb):
    """Every edge of np.linspace(0, 1, nb + 1), the doubles on both sides of each, and the values at and past [0, 1]."""
    e = np.linspace(0.0, 1.0, nb + 1)
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                           [0.0, -0.0, 1.0, np.nextafter(1.0, 2.0), -5e-324, np.nan, np.inf, -np.inf]])


def edge_points(nb):
    """Each axis in turn takes every edge value; the other two components sit in the middle of a bin."""
    v = edge_values(nb)
    j = np.arange(v.size)
    mid = lambda k: (k % nb + 0.5) / nb
    pts = []
    for a in range(3):
        p = np.empty((v.size, 3))
        p[:, a] = v
        p[:, (a + 1) % 3] = mid(j)
        p[:, (a + 2) % 3] = mid(3 * j + 1)
        pts.append(p)
    return np.concatenate(pts)


def misplaced(got, want):
    """Samples binned unlike the reference: one put in the wrong cell, or dropped or kept wrongly, counts once."""
    d = got.astype(np.int64) - want.astype(np.int64)
    return int((np.abs(d).sum() + abs(d.sum())) // 2)


def test_histogram_edges_on_every_axis(model):
    bad = {}
    for nb in EDGE_NBINS:
        pts = edge_points(nb)
        got, want = model.flavor_histogram(pts, nb), reference_hist(pts, nb)
        if not np.array_equal(got, want):
            bad[nb] = misplaced(got, want)
        del got, want
    assert not bad, "nb -> samples binned unlike np.histogramdd: %s" % bad


def test_histogram_edges_on_all_axes_at_once(model):
    rng = np.random.default_rng(17)
    for nb in (2, 3, 5, 10, 21, 49, 100, 128, 256):
        v = edge_values(nb)
        pts = v[rng.integers(0, v.size, (100_000, 3))]
        assert np.array_equal(model.flavor_histogram(pts, nb), reference_hist(pts, nb)), nb
    # the first case the old rule (int)(v * nb) got wrong: 0.6 * 5 == 3.0, numpy's edge 3 is 0.6000000000000001
    h = model.flavor_histogram([[0.6, 0.6, 0.6]], 5)
    assert h[2, 2, 2] == 1 and h.sum() == 1


def test_histogram_device_entry_point(model):
    L = _lib.lib()
    rng = np.random.default_rng(4)
    nb = 21
    fr1 = np.concatenate([edge_points(nb), rng.uniform(-0.05, 1.05, (5000, 3))])
    fr2 = np.concatenate([rng.dirichlet((1., 1., 1.), 7000), edge_points(nb)[::3]])
    d1, d2 = model.alloc(fr1.nbytes).upload(fr1), model.alloc(fr2.nbytes).upload(fr2)
    dc = model.alloc(8 * nb ** 3).upload(np.zeros(nb ** 3, dtype=np.uint64))
    try:
        assert L.gf_flavor_histogram_device(model._h, d1.ptr, len(fr1), nb, dc.ptr) == _lib.GF_OK
        assert L.gf_flavor_histogram_device(model._h, d2.ptr, len(fr2), nb, dc.ptr) == _lib.GF_OK   # counts +=
        model.sync()
        both = reference_hist(fr1, nb) + reference_hist(fr2, nb)
        assert np.array_equal(dc.download((nb, nb, nb), dtype=np.uint64), both)
        assert L.gf_flavor_histogram_device(model._h, d1.ptr, 0, nb, dc.ptr) == _lib.GF_OK          # n = 0: no change
        model.sync()
        assert np.array_equal(dc.download((nb, nb, nb), dtype=np.uint64), both)
        for n_bad in (0, 1025):
            assert L.gf_flavor_histogram_device(model._h, d1.ptr, len(fr1), n_bad, dc.ptr) == _lib.GF_ERR_INVALID_ARG
            counts = np.zeros(8, dtype=np.uint64)
            assert L.gf_flavor_histogram(model._h, fr1.ctypes.data_as(_lib._dp), len(fr1), n_bad,
                                         counts.ctypes.data_as(C.POINTER(C.c_uint64))) == _lib.GF_ERR_INVALID_ARG
        model.sync()
        assert np.array_equal(dc.download((nb, nb, nb), dtype=np.uint64), both)
    finally:
        for b in (d1, d2, dc):
            b.free()


def test_histogram_atomics_under_contention(model):
    """2^25 + 3 samples in one cell, then the same number alternating between two neighbouring cells: exact counts."""
    n, nb = (1 << 25) + 3, 16
    a, b = (4, 8, 11), (4, 8, 12)
    fr = np.empty((n, 3))
    fr[:] = (np.array(a) + 0.5) / nb
    want = np.zeros((nb, nb, nb), dtype=np.uint64)
    want[a] = n
    assert np.array_equal(model.flavor_histogram(fr, nb), want)
    fr[1::2] = (np.array(b) + 0.5) / nb
    want[a], want[b] = (n + 1) // 2, n // 2
    assert np.array_equal(model.flavor_histogram(fr, nb), want)


def test_sampler_postprocess_histogram():
    """DeviceEnsembleSampler.postprocess(nbins=...) at flavor_contour's os_nbins + 1 bins and at 128, with the sampled
    posterior and with another source per chain: each chain's hist is np.histogramdd of that chain's returned fr."""
    ps = Cf.unitary_paramset()
    m = Model(compile_model(ps, "PRIOR_ONLY", source_ratio=np.array([1., 2., 0.]) / 3))
    pms = [Model(compile_model(ps, "PRIOR_ONLY", source_ratio=x)) for x in ([1., 0., 0.], [0., 1., 0.])]
    np.random.seed(8)
    p0 = np.stack([mcmc_utils.flat_seed(ps, 64) for _ in range(2)])
    s = mcmc_utils.DeviceEnsembleSampler(64, 4, m, nchains=2, seed=21)
    try:
        s.run_mcmc(p0, 200, thin=2)
        for nb in (21, 128):
            for models in (None, pms):
                post = s.postprocess(want_fr=True, nbins=nb, models=models)
                assert post["hist"].shape == (2, nb, nb, nb)
                for c in range(2):
                    fr = post["fr"][c].reshape(-1, 3)
                    assert np.array_equal(post["hist"][c], reference_hist(fr, nb)), (nb, models is None, c)
                    assert post["hist"][c].sum() == np.all((fr >= 0) & (fr <= 1), axis=1).sum()
    finally:
        s.close()
        for x in pms + [m]:
            x.close()


def u53(hi, lo):
    """gf_kernels.hip u53 / golem_oracle.c orc_u53: 53 bits of two Philox words in [0, 1)."""
    return ((hi >> 5) * 67108864.0 + (lo >> 6)) * (1.0 / 9007199254740992.0)


def test_haar_stream_is_published_philox(model):
    """Draw 0 of seed 0 is Philox4x32-10 of counter (0, 0, 0, 0), key (0, 0): 6627e8d5 e169c58d bc57ac4c 9b00dbd8
    (Random123 kat_vectors).  s12^2 takes the first two words, c13^4 the last two."""
    _, ang = model.haar_draw(seed=0, n=1, first_draw=0, want_angles=True)
    assert ang[0, 0] == u53(0x6627e8d5, 0xe169c58d)
    assert ang[0, 1] == u53(0xbc57ac4c, 0x9b00dbd8)


# ---- Haar measure: the device's draws against an independent construction ----------------------------------------------------
NHAAR = 1 << 20


def qr_haar_unitaries(n, seed):
    """Haar-random U(3) (Mezzadri, Notices AMS 54 (2007) 592): Q of the QR of a complex Gaussian matrix, times the phases
    of R's diagonal."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    q, r = np.linalg.qr(z)
    d = np.diagonal(r, axis1=1, axis2=2)
    return q * (d / np.abs(d))[:, None, :]


def compositions(u, src):
    """fr_b = sum_a sum_i |U_ai|^2 |U_bi|^2 s_a, s normalised: no mixing angles involved."""
    p = np.abs(u) ** 2
    return (p @ p.transpose(0, 2, 1)) @ (np.asarray(src, dtype=np.float64) / np.sum(src))


def pdg_unitaries(ang):
    """(s12^2, c13^4, s23^2, delta) -> U in the PDG parametrisation, for many draws at once."""
    s12_2, c13_4, s23_2, dcp = ang.T
    c13_2 = np.sqrt(c13_4)
    s12, c12 = np.sqrt(s12_2), np.sqrt(1 - s12_2)
    c13, s13 = np.sqrt(c13_2), np.sqrt(1 - c13_2)
    s23, c23 = np.sqrt(s23_2), np.sqrt(1 - s23_2)
    ep = np.exp(1j * dcp)
    u = np.empty((len(ang), 3, 3), dtype=np.complex128)
    u[:, 0] = np.stack([c12 * c13, s12 * c13, s13 * np.conj(ep)], axis=1)
    u[:, 1] = np.stack([-s12 * c23 - c12 * s23 * s13 * ep, c12 * c23 - s12 * s23 * s13 * ep, s23 * c13], axis=1)
    u[:, 2] = np.stack([s12 * s23 - c12 * c23 * s13 * ep, -c12 * s23 - s12 * c23 * s13 * ep, c23 * c13], axis=1)
    return u


@pytest.fixture(scope="module")
def qr_unitaries():
    return qr_haar_unitaries(NHAAR, 20260)


@pytest.mark.parametrize("src", [(1., 2., 0.), (1., 0., 0.)])
def test_haar_draws_match_qr_haar_unitaries(qr_unitaries, src):
    """2^20 device draws against 2^20 QR unitaries, KS per component, p > 1e-6.  Seeds are fixed, so the p-values are too.
    The same test rejects the prior with c13^2 flat instead of c13^4 (p < 1e-6 on every component)."""
    from scipy.stats import ks_2samp
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=np.array(src) / sum(src)))
    try:
        fr, ang = m.haar_draw(seed=26, n=NHAAR, want_angles=True)
    finally:
        m.close()
    ref = compositions(qr_unitaries, src)
    p = [ks_2samp(fr[:, k], ref[:, k]).pvalue for k in range(3)]
    print("Haar vs QR, source %s: KS p = %s" % (src, ", ".join("%.3g" % x for x in p)))
    assert min(p) > 1e-6, p
    # the draws' own angles, put through the PDG matrix here, give the device's compositions ...
    assert np.abs(compositions(pdg_unitaries(ang), src) - fr).max() < 1e-10
    # ... and with c13^2 flat (c13^4 = u^2) instead of c13^4 flat they are not Haar
    wrong = ang.copy()
    wrong[:, 1] = ang[:, 1] ** 2
    fw = compositions(pdg_unitaries(wrong), src)
    pw = [ks_2samp(fw[:, k], ref[:, k]).pvalue for k in range(3)]
    print("  c13^2 flat: KS p = %s" % ", ".join("%.3g" % x for x in pw))
    assert max(pw) < 1e-6, pw
