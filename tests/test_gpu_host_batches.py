"""The host-buffer entry points at the boundaries between their branches, with the optional outputs absent.

gf_lnprob_batch / gf_propagate_batch take a batch one of three ways: up to 2048 rows the kernel reads and writes the pinned mirror
directly (zero-copy), below 4 x 65536 rows the batch crosses in one transfer each way, from there on it streams through two pinned
slots in chunks of 65536 rows (four times as long from 32 x 65536 rows on).  gf_lnprob_cube_batch is the one-transfer path with the
cube map in front.  Every path evaluates, downloads and copies out only what the caller asked for: `fr` and `status` may be NULL for
lnprob, `status` for propagate.  Pinned here, bit for bit against the device-resident path on the same rows: every size either side of
a boundary, every combination of absent outputs (the C entry points are called through ctypes so that the NULLs reach the library),
twice on the same model so that the second call reuses the staging, into arrays pre-filled with a sentinel.
"""
import numpy as np
import pytest

from common import BIN_EDGES, notebook_sets, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import Texture
from golemflavor_amd.model import Model

pytestmark = pytest.mark.gpu

CHUNK = 65536
ROWS = (1, 2048, 2049, 4 * CHUNK - 1, 4 * CHUNK, 4 * CHUNK + 1)      # last zero-copy, first / last one-transfer, pipelined exact / ragged
ROWS_LONG_CHUNKS = 32 * CHUNK + 1                                    # SM only: the chunks are four times as long
CUBE_ROWS = (1, 2049)
SENTINEL, SENTINEL_ST = -12345.678, -77
FR_STATUS = ((True, True), (False, True), (True, False), (False, False))    # (fr given, status given)


class _Case:
    """One open model, its input rows (the first n of them are a batch) and the device-resident results of a batch."""

    def __init__(self, model, theta):
        self.m, self.theta = model, theta

    def want(self, th):
        """The device-resident path on the rows `th`, by whether a status array is given (without one a BSM model computes no unitarity
        verdict, and a row that would have failed it keeps its value): {with_status: (lnprob, fr, status, propagate's fr, its status)}."""
        n = len(th)
        m = self.m
        d_th = m.alloc(th.nbytes).upload(th)
        d_out, d_fr, d_st = m.alloc(8 * n), m.alloc(24 * n), m.alloc(4 * n)
        res = {}
        for with_status in (True, False):
            st_ptr = d_st.ptr if with_status else None
            status = (lambda: d_st.download((n,), dtype=np.int32)) if with_status else (lambda: None)
            m.lnprob_device(d_th.ptr, n, d_out.ptr, d_fr.ptr, st_ptr)
            m.sync()
            lnprob = (d_out.download((n,)), d_fr.download((n, 3)), status())
            m.propagate_device(d_th.ptr, n, d_fr.ptr, st_ptr)        # no prior: a row outside the box is evaluated, or NaN
            m.sync()
            res[with_status] = lnprob + (d_fr.download((n, 3)), status())
        for b in (d_th, d_out, d_fr, d_st):
            b.free()
        return res


@pytest.fixture(scope="module")
def sm(golden):
    _, ps = notebook_sets(golden)
    th = uniform_theta(ps, ROWS_LONG_CHUNKS, np.random.default_rng(41), seeds=True)
    th[::1000, 0] = 2.0                                              # some rows outside the prior box (row 0: the batch of one)
    with Model(compile_model(ps, "SM_GAUSS", bestfit_fr=golden["g6_bestfit_fr"], smearing=0.02)) as m:
        yield _Case(m, th)


@pytest.fixture(scope="module")
def bsm():
    ps = Cf.texture_paramset(6)
    lo, hi = Cf.SCALE_BOUNDARIES[6]
    rng = np.random.default_rng(43)
    th = uniform_theta(ps, max(ROWS), rng, seeds=True)
    th[:, 6] = rng.uniform(lo, hi, len(th))
    th[5::1000, 0] = 2.0                                             # some rows outside the prior box
    with Model(compile_model(ps, "BSM_GAUSS", texture=Texture.OEU, dimension=6, binning=BIN_EDGES, source_ratio=(0., 1., 0.),
                             bestfit_fr=(1 / 3,) * 3, smearing=0.02)) as m:
        yield _Case(m, th)


def _outputs(n, with_lnprob, with_fr, with_status):
    lp = np.full(n, SENTINEL) if with_lnprob else None
    fr = np.full((n, 3), SENTINEL) if with_fr else None
    st = np.full(n, SENTINEL_ST, dtype=np.int32) if with_status else None
    return lp, fr, st


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def _same(got, want):
    """Every output that was asked for is the device-resident path's, bit for bit (an output left unwritten still holds the sentinel)."""
    for g, w in zip(got, want):
        assert (g is None) or np.array_equal(g, w, equal_nan=True)


def _walk_host_batches(case, n):
    m, th = case.m, np.ascontiguousarray(case.theta[:n])
    want = case.want(th)
    L = m._L
    for with_fr, with_status in FR_STATUS:
        for _ in range(2):                                           # the second call reuses the staging
            lp, fr, st = _outputs(n, True, with_fr, with_status)
            rc = L.gf_lnprob_batch(m._h, _ptr(th, _lib._dp), n, _ptr(lp, _lib._dp), _ptr(fr, _lib._dp), _ptr(st, _lib._ip))
            _lib.check(rc, "gf_lnprob_batch")
            _same((lp, fr, st), want[with_status][:3])
    for with_status in (True, False):
        for _ in range(2):
            _, fr, st = _outputs(n, False, True, with_status)
            rc = L.gf_propagate_batch(m._h, _ptr(th, _lib._dp), n, _ptr(fr, _lib._dp), _ptr(st, _lib._ip))
            _lib.check(rc, "gf_propagate_batch")
            _same((fr, st), want[with_status][3:])
    return want[True]


def _walk_cube_batches(case, n, cols, base):
    """gf_lnprob_cube_batch against gf_lnprob_batch on the rows the cube expands to (mn.py:36's expression, the model's own box).
    The scanned columns' boxes start at 0, so that the map is one rounded product whether or not the sum is fused into it (a column
    of the scale's kind, lo = -56, would tell the two apart; that is the map kernel's business, not the batch plumbing's)."""
    m = case.m
    rng = np.random.default_rng(1000 + n)
    cube = rng.uniform(0.0, 1.0, size=(n, len(cols)))
    base = np.ascontiguousarray(base, dtype=np.float64)
    th = np.tile(base, (n, 1))
    for k, c in enumerate(cols):
        lo, hi = m.desc.lo[c], m.desc.hi[c]
        assert lo == 0.0
        th[:, c] = (hi - lo) * cube[:, k] + lo
    L = m._L
    want = {}
    for with_status in (True, False):
        want[with_status] = lp, fr, st = _outputs(n, True, True, with_status)
        _lib.check(L.gf_lnprob_batch(m._h, _ptr(th, _lib._dp), n, _ptr(lp, _lib._dp), _ptr(fr, _lib._dp), _ptr(st, _lib._ip)), "gf_lnprob_batch")
    ccols = np.ascontiguousarray(cols, dtype=np.int32)
    for with_fr, with_status in FR_STATUS:
        for _ in range(2):
            lp, fr, st = _outputs(n, True, with_fr, with_status)
            rc = L.gf_lnprob_cube_batch(m._h, _ptr(cube, _lib._dp), n, len(cols), _ptr(ccols, _lib._ip), _ptr(base, _lib._dp),
                                        _ptr(lp, _lib._dp), _ptr(fr, _lib._dp), _ptr(st, _lib._ip))
            _lib.check(rc, "gf_lnprob_cube_batch")
            _same((lp, fr, st), want[with_status])
    return want[True]


@pytest.mark.parametrize("n", ROWS + (ROWS_LONG_CHUNKS,))
def test_sm_host_batches_equal_the_device_resident_path(sm, n):
    want = _walk_host_batches(sm, n)
    assert np.isneginf(want[0][::1000]).all() and (want[2][::1000] == _lib.GF_ST_OUT_OF_PRIOR).all()
    assert n < 1000 or np.isfinite(want[0]).sum() > 0.99 * n


def test_bsm_input_carries_non_unitary_rows(bsm):
    """What the BSM cases below rely on: the status path carries something."""
    st = bsm.want(bsm.theta)[True][2]
    assert 0.1 < np.mean(st == _lib.GF_ST_NON_UNITARY) < 0.3
    assert (st[5::1000] == _lib.GF_ST_OUT_OF_PRIOR).all()


@pytest.mark.parametrize("n", ROWS)
def test_bsm_host_batches_equal_the_device_resident_path(bsm, n):
    want = _walk_host_batches(bsm, n)
    if n >= 2048:
        assert 0.1 < np.mean(want[2] == _lib.GF_ST_NON_UNITARY) < 0.3
        assert np.isnan(want[0][want[2] == _lib.GF_ST_NON_UNITARY]).all()


@pytest.mark.parametrize("n", CUBE_ROWS)
def test_sm_cube_batches_equal_the_host_batch_on_the_expanded_rows(sm, n):
    want = _walk_cube_batches(sm, n, (0, 3), sm.theta[1])
    assert np.isfinite(want[0]).all() and (want[2] == _lib.GF_ST_OK).all()


@pytest.mark.parametrize("n", CUBE_ROWS)
def test_bsm_cube_batches_equal_the_host_batch_on_the_expanded_rows(bsm, n):
    base = bsm.theta[1].copy()
    base[6] = Cf.SCALE_BOUNDARIES[6][1] - 3.0                        # the top of the scale range: the rows fail the unitarity verdict,
    want = _walk_cube_batches(bsm, n, (2, 3), base)                  # so lnprob is NaN with a status array and a value without
    assert (want[2] == _lib.GF_ST_NON_UNITARY).any() and np.isnan(want[0][want[2] == _lib.GF_ST_NON_UNITARY]).all()
