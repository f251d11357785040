"""GPU: the bulk kernels on the second and later trip of their tile loops, value by value against the oracle.

A bulk launch caps its grid at (compute units x blocks per compute unit) workgroups (gf_launch.h gf_grid_for), so one pass of the grid
covers `pass_items` walkers (gf_internal_pass_items: 524 288 on a 256-CU MI355X) and a wave takes a second tile only in a single launch
of more than that.  That trip is where k_bsm prefetches tile t + stride into its other LDS buffer, where k_lnprob_sm_fast / _soa
refill their register pipeline and defer the lnprob store, and where every other kernel's stride loop comes round -- and the host
entry point never gets there (it streams large batches in chunks of 65 536 rows).  Every batch here is one launch of
    n = 2 * pass_items + 64 * 5 + 29
walkers through the device entry points: two full passes, part of a third, a ragged last tile, n // 64 not divisible by 8 (uneven XCD
spans).  Each test asserts n >= 2 * pass_items + 64 before it launches, so a later change of the cap fails here instead of quietly
making these one-pass tests.

The oracle cannot evaluate a million BSM rows in seconds, so a batch repeats a base block of 4099 rows -- a prime: row i is base row
i mod 4099, no two tiles hold the same rows and every base row visits every lane -- and the oracle sees the base block only.  The block
holds seeded rows, an eighth of them outside the prior box, one NaN row and one +inf row; for BSM the scale is uniform over its whole
range, so a fifth of the rows fail the unitarity verdict and a few per cent need the arbitration.  One SM case uses independent random
rows throughout (a bug periodic in 4099 would hide behind the base block).

Asserted per case, with fr and status both requested and both NULL:
  * against the oracle on every row of the batch, with the suite's own bars (REL, ABS_FR, 1e-10 + 10 r80, the verdict outside half a
    decade around 1e-7);
  * bit for bit: a base row gives the same bits wherever it lands, and the bits of a sub-capacity launch (for SM: of the kernel that
    takes whole tiles within [0, 64 (n // 64)), of the generic kernel in the ragged tail);
  * nothing else is written: every output sits between 64-element guards, all pre-filled with a NaN whose payload no kernel
    produces (an int32 pattern for the status); afterwards the guards are intact and no such value is left in range.

Measured on an MI355X (256 CUs, pass_items = 524 288, n = 1 048 925): see DESIGN.md, "Tests past one pass of the grid".
"""
import numpy as np
import pytest

from common import BIN_EDGES, rel_err, uniform_theta
from golemflavor_amd import _lib
from golemflavor_amd import configs as Cf
from golemflavor_amd.descriptor import compile_model
from golemflavor_amd.enums import ParamTag, Texture
from golemflavor_amd.model import GF_LAYOUT_AOS, GF_LAYOUT_SOA, Model
from golemflavor_amd.param import Param, ParamSet
from test_gpu_parity import ABS_FR, REL                              # the suite's bars, from where they live
from test_gpu_parity_r2 import _decided                              # the verdict must agree outside half a decade around 1e-7
from test_gpu_postprocess_exact import reference_hist

pytestmark = pytest.mark.gpu

PERIOD = 4099                                                        # rows of a base block: prime
GUARD = 64                                                           # elements in front of and behind every output
SENTINEL_F64 = np.uint64(0x7FF8DEADBEEF5EED)                         # a quiet NaN with a payload: the kernels write 0x7ff8000000000000,
SENTINEL_I32 = np.int32(0x5EEDBEEF)                                  # the hardware's default NaN or an input's; statuses are 0 ... 3
BAND_SHARE_MAX = 0.03                                                # base rows the verdict band may leave out


def batch_rows(model):
    """(pass_items, n) for the model's device, with the properties every test here relies on."""
    p = _lib.pass_items(model._h)
    n = 2 * p + 64 * 5 + 29
    assert p > 0 and p % 64 == 0
    assert n >= 2 * p + 64, "not two passes of the grid: the cap of gf_grid_for has changed"
    assert n % 64 != 0 and (n // 64) % 8 != 0
    return p, n


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Guarded:
    """A device output of `count` elements between two guard zones, all pre-filled with the sentinel."""

    def __init__(self, model, count, dtype=np.float64):
        self.count, self.f64 = int(count), np.dtype(dtype) == np.float64
        self.raw_dtype = np.uint64 if self.f64 else np.int32
        self.sentinel = SENTINEL_F64 if self.f64 else SENTINEL_I32
        host = np.full(self.count + 2 * GUARD, self.sentinel, dtype=self.raw_dtype)
        self.buf = model.alloc(host.nbytes).upload(host)
        self.ptr = self.buf.at(GUARD * host.itemsize)

    def take(self, width=1):
        raw = self.buf.download((self.count + 2 * GUARD,), dtype=self.raw_dtype)
        self.buf.free()
        assert (raw[:GUARD] == self.sentinel).all(), "written in front of the output"
        assert (raw[GUARD + self.count:] == self.sentinel).all(), "written behind the output"
        body = raw[GUARD:GUARD + self.count]
        left = np.flatnonzero(body == self.sentinel)
        assert left.size == 0, "%d elements never written, the first at %d (walker %d)" % (left.size, left[0], left[0] // width)
        out = body.view(np.float64) if self.f64 else body
        return out.reshape(-1, width) if width > 1 else out


def upload_rows(model, rows, layout):
    arr = rows if layout == GF_LAYOUT_AOS else np.ascontiguousarray(rows.T)
    return model.alloc(arr.nbytes).upload(arr)


def launch(model, d_theta, n, layout, outputs, propagate=False):
    """One launch of the device entry point on n walkers into guarded outputs: (lnprob, fr, status), None where not requested
    (`outputs`: fr and status both, or neither; propagate has no lnprob and always a composition)."""
    g_lp = None if propagate else Guarded(model, n)
    g_fr = Guarded(model, 3 * n) if (outputs or propagate) else None
    g_st = Guarded(model, n, np.int32) if outputs else None
    p = lambda g: g.ptr if g is not None else None
    if propagate:
        model.propagate_device(d_theta.ptr, n, p(g_fr), p(g_st), layout=layout)
    else:
        model.lnprob_device(d_theta.ptr, n, p(g_lp), p(g_fr), p(g_st), layout=layout)
    model.sync()
    return (g_lp.take() if g_lp else None, g_fr.take(3) if g_fr else None, g_st.take() if g_st else None)


def launch_rows(model, rows, layout, outputs, propagate=False):
    d = upload_rows(model, rows, layout)
    try:
        return launch(model, d, len(rows), layout, outputs, propagate)
    finally:
        d.free()


def base_block(ps, seed, scale=None):
    """4099 seeded rows; an eighth of them outside the prior box (column 0 at 2.0), one NaN row, one +inf row.  `scale` = (column, lo,
    hi): that column uniform over [lo, hi]."""
    rng = np.random.default_rng(seed)
    th = uniform_theta(ps, PERIOD, rng, seeds=True)
    if scale is not None:
        col, lo, hi = scale
        th[:, col] = rng.uniform(lo, hi, PERIOD)
    assert np.array(ps.ranges, dtype=float)[0, 1] < 2.0
    where = rng.permutation(PERIOD)
    outside, rest = where[:PERIOD // 8], where[PERIOD // 8:]
    th[outside, 0] = 2.0
    th[rest[0], min(1, len(ps) - 1)] = np.nan
    th[rest[1], len(ps) - 1] = np.inf
    assert outside.size >= 0.1 * PERIOD
    return np.ascontiguousarray(th), {"outside": outside, "nan": rest[0], "inf": rest[1]}


# ---- SM / PRIOR_ONLY: k_lnprob_sm_fast, k_lnprob_sm_soa, k_lnprob_sm_gen -------------------------------------------------------------
NB_ANGLES = (0.5373597586219514, 0.5006819093249053)
LG = Cf.PriorsCateg.LIMITEDGAUSS


def sm_case(name):
    """(paramset, mode, compile_model's keywords, the oracle's extra keywords) of a row of the issue's SM table."""
    nbl = list(Cf.notebook_paramsets(NB_ANGLES)[1])
    kw, okw = dict(bestfit_fr=(0.55, 0.18, 0.27), smearing=0.02), {}
    mode = "SM_GAUSS"
    extra = lambda k: [Param(name="n%d" % i, value=1.0, ranges=[0., 2.], std=0.3, prior=LG if i % 2 else None, tag=ParamTag.NUISANCE)
                       for i in range(k)]
    if name == "notebook6":                                          # SAMPLED = 2: canonical columns
        ps = ParamSet(nbl)
    elif name == "permuted6":                                        # SAMPLED = 1: named re-reads from LDS
        ps = ParamSet([nbl[4], nbl[0], nbl[5], nbl[3], nbl[1], nbl[2]])
    elif name == "reordered6":                                       # ... with the mixing parameters in their own order, so that the
        ps = ParamSet([nbl[4], nbl[0], nbl[5], nbl[1], nbl[2], nbl[3]])  # rows are finite (permuted6 feeds dcp to c_13_4: mostly NaN)
    elif name == "fixed_source4":                                    # SAMPLED = 0
        ps = ParamSet(nbl[:4])
        kw["source_ratio"] = (0.2, 0.7, 0.1)
    elif name == "odd7":                                             # EVEN == false: half-filled last vector of every tile
        ps = ParamSet(nbl + [Param(name="extra", value=1.0, ranges=[0., 2.], std=0.25, prior=LG, tag=ParamTag.NUISANCE)])
    elif name == "wide12":                                           # the two-waves-per-SIMD instances
        ps = ParamSet(nbl + extra(6))
    elif name == "tutorial2":
        ps = Cf.tutorial_paramsets(NB_ANGLES)[1]
        kw.update(sm_fixed=(0.0, 1.0, 0.0, 0.0), src_columns=(0, 1))
    elif name == "generic5":                                         # no instance of this width: the generic kernel's own stride loop
        ps = ParamSet(list(Cf.unitary_paramset()) + [Param(name="extra", value=1.0, ranges=[0., 2.], std=0.3, prior=LG,
                                                           tag=ParamTag.NUISANCE)])
        kw = dict(bestfit_fr=(0.3, 0.35, 0.35), smearing=0.05, source_ratio=(1 / 3, 2 / 3, 0))
    elif name == "prior6":                                           # SAMPLED = 0 from columns
        ps, mode, kw = ParamSet(nbl), "PRIOR_ONLY", {}
    elif name == "prior12":
        ps, mode, kw = ParamSet(nbl + extra(6)), "PRIOR_ONLY", {}
    else:
        raise KeyError(name)
    return ps, mode, kw, dict(kw, **okw)


def check_sm(got, ref, idx, mode):
    """The outputs of a launch against the oracle's (lnprob, fr, status) of the base block, row idx[i] for walker i."""
    lp, fr, st = got
    rlp, rfr, rst = ref
    want = rlp[idx]
    assert np.array_equal(np.isneginf(lp), np.isneginf(want)) and np.array_equal(np.isnan(lp), np.isnan(want))
    assert not np.isposinf(lp).any()
    assert rel_err(lp, want) <= REL
    if st is not None:
        assert np.array_equal(st, rst[idx])
    if fr is not None:
        ok = (rst == _lib.GF_ST_OK)[idx]
        if mode == "SM_GAUSS":
            assert np.abs(fr[ok] - rfr[idx][ok]).max() <= ABS_FR
            assert np.isnan(fr[~ok]).all()
        else:
            assert np.isnan(fr).all()                                # no composition without a likelihood


SM_CASES = [("notebook6", GF_LAYOUT_AOS), ("notebook6", GF_LAYOUT_SOA), ("permuted6", GF_LAYOUT_AOS), ("reordered6", GF_LAYOUT_AOS),
            ("fixed_source4", GF_LAYOUT_AOS),
            ("odd7", GF_LAYOUT_AOS), ("wide12", GF_LAYOUT_AOS), ("wide12", GF_LAYOUT_SOA), ("tutorial2", GF_LAYOUT_AOS),
            ("generic5", GF_LAYOUT_AOS), ("generic5", GF_LAYOUT_SOA), ("prior6", GF_LAYOUT_SOA), ("prior12", GF_LAYOUT_SOA)]


@pytest.mark.parametrize("name,layout", SM_CASES, ids=["%s-%s" % (c, "soa" if l else "aos") for c, l in SM_CASES])
def test_sm_batches_past_one_pass(oracle, name, layout):
    ps, mode, kw, okw = sm_case(name)
    nd = len(ps)
    base, _ = base_block(ps, 100 + nd)
    om = oracle.make_model(ps, mode, **okw)
    ref = oracle.lnprob_batch(om, base, want_fr=True, want_status=True)
    assert (ref[2] != _lib.GF_ST_OUT_OF_PRIOR).sum() == PERIOD - PERIOD // 8 - 2 and np.isfinite(ref[0]).sum() > 500
    with Model(compile_model(ps, mode, **kw)) as m:
        _, n = batch_rows(m)
        idx = np.arange(n) % PERIOD
        nfast = 64 * (n // 64)                                       # whole tiles: the pipelined kernels; behind them the generic kernel
        d_big = upload_rows(m, np.resize(base, (n, nd)), layout)
        for outputs in (True, False):
            # sub-capacity launches: whole tiles only (65 tiles: base rows 0 ... 4098 and the first 61 again), the generic kernel
            # only (ragged launches of at most 2048 rows), and the base block as it is (64 whole tiles and 3 rows of tail)
            tiles = launch_rows(m, np.resize(base, (65 * 64, nd)), layout, outputs)
            parts = [launch_rows(m, base[a:a + 2046], layout, outputs) for a in range(0, PERIOD, 2046)]
            generic = tuple(None if p is None else np.concatenate([q[k] for q in parts]) for k, p in enumerate(parts[0]))
            block = launch_rows(m, base, layout, outputs)
            big = launch(m, d_big, n, layout, outputs)
            check_sm(big, ref, idx, mode)
            check_sm(tiles, ref, np.arange(65 * 64) % PERIOD, mode)
            check_sm(generic, ref, np.arange(PERIOD), mode)
            for k in range(3):
                if big[k] is None:
                    assert tiles[k] is None and generic[k] is None and block[k] is None
                    continue
                assert same_bits(big[k][:nfast], tiles[k][idx[:nfast]]), (name, outputs, k)
                assert same_bits(big[k][nfast:], generic[k][idx[nfast:]]), (name, outputs, k)
                assert same_bits(block[k][:4096], tiles[k][:4096]) and same_bits(block[k][4096:], generic[k][4096:PERIOD])
        d_big.free()


def test_sm_independent_rows_past_one_pass(oracle):
    """12 columns from rows, every row its own: the oracle on all of them."""
    ps, mode, kw, okw = sm_case("wide12")
    om = oracle.make_model(ps, mode, **okw)
    with Model(compile_model(ps, mode, **kw)) as m:
        _, n = batch_rows(m)
        rng = np.random.default_rng(12)
        th = uniform_theta(ps, n, rng, seeds=True)
        cols = rng.integers(0, len(ps), n)
        box = np.array(ps.ranges, dtype=float)
        out = np.flatnonzero(rng.random(n) < 0.1)                    # a tenth outside the box in one column
        th[out, cols[out]] = box[cols[out], 1] + 0.3
        wild = np.flatnonzero(rng.random(n) < 0.001)
        th[wild, cols[wild]] = rng.choice([np.nan, np.inf, -np.inf], wild.size)
        ref = oracle.lnprob_batch(om, th, want_fr=True, want_status=True)
        d_th = upload_rows(m, th, GF_LAYOUT_AOS)
        idx = np.arange(n)
        got = launch(m, d_th, n, GF_LAYOUT_AOS, True)
        check_sm(got, ref, idx, mode)
        bare = launch(m, d_th, n, GF_LAYOUT_AOS, False)
        check_sm(bare, ref, idx, mode)
        assert same_bits(bare[0], got[0])
        d_th.free()


@pytest.mark.parametrize("tiles", [29, 30, 31])
def test_sm_uneven_xcd_spans_within_one_pass(oracle, tiles):
    """A grid of 8 blocks (nx = 8) over 29 ... 31 tiles: XCD spans of 3 and 4 tiles, and in the spans of 3 a wave past the end."""
    ps, mode, kw, okw = sm_case("notebook6")
    n = 64 * tiles
    rng = np.random.default_rng(tiles)
    th = uniform_theta(ps, n, rng, seeds=True)
    th[rng.permutation(n)[:n // 8], 0] = 2.0
    ref = oracle.lnprob_batch(oracle.make_model(ps, mode, **okw), th, want_fr=True, want_status=True)
    with Model(compile_model(ps, mode, **kw)) as m:
        assert (n + 255) // 256 == 8 and n < _lib.pass_items(m._h)
        for outputs in (True, False):
            check_sm(launch_rows(m, th, GF_LAYOUT_AOS, outputs), ref, np.arange(n), mode)


# ---- BSM: k_bsm -------------------------------------------------------------------------------------------------------------------
_BSM = {}


def bsm_case(oracle, name):
    """A row of the issue's BSM table, built and put through the oracle once per session: the model's keywords, the base block and
    the oracle's outputs on it (never modified afterwards)."""
    if name in _BSM:
        return _BSM[name]
    src, bf = (0., 1., 0.), (1 / 3,) * 3
    mm_cols = None
    if name == "oeu7":                                               # <7, ., .>: the 7-column texture posterior
        ps, dim, tex = Cf.texture_paramset(6), 6, Texture.OEU
    elif name == "oeu12":                                            # <12, ., .>: the 12-column posterior of the bulk benchmark
        ps, dim, tex = Cf.fr_paramsets(6, (0.4444, 0.0))[1], 6, Texture.OEU
    elif name == "none11":                                           # NDIM = 0: the NP mixing angles are sampled
        t3 = list(Cf.texture_paramset(3))
        mm = [Param(name="np_%s" % k, value=0.5, ranges=r, tag=ParamTag.MMANGLES)
              for k, r in (("s12", [0., 1.]), ("c13", [0., 1.]), ("s23", [0., 1.]), ("dcp", [0., 2 * np.pi]))]
        ps, dim, tex, mm_cols = ParamSet(t3[:6] + mm + t3[6:]), 3, Texture.NONE, (6, 7, 8, 9)
        bf = (0.3, 0.4, 0.3)
    else:
        raise KeyError(name)
    kw = dict(texture=tex, dimension=dim, binning=BIN_EDGES, source_ratio=src, bestfit_fr=bf, smearing=0.02)
    lo, hi = Cf.SCALE_BOUNDARIES[dim]
    base, rows = base_block(ps, PERIOD, scale=(len(ps) - 1, lo, hi))
    om = oracle.make_model(ps, "BSM_GAUSS", **dict(kw, texture=tex.name))
    lp, fr, st = oracle.lnprob_batch(om, base, want_fr=True, want_status=True)
    # the residual and the composition without priors for the rows inside the box only (the oracle's 80-bit arithmetic on the NaN a
    # row outside the box turns into is ten times slower, and nothing is asserted of those rows): NaN and -1 elsewhere
    inbox = st != 1
    r80, pfr, pst = np.full(PERIOD, np.nan), np.full((PERIOD, 3), np.nan), np.full(PERIOD, -1, dtype=np.int32)
    r80[inbox] = oracle.unitarity_residual_batch(om, base[inbox])
    pfr[inbox], pst[inbox] = oracle.propagate_batch(om, base[inbox])
    case = dict(ps=ps, kw=kw, base=base, rows=rows, lp=lp, fr=fr, st=st, pfr=pfr, pst=pst, r80=r80, tex=tex, dim=dim, src=np.array(src),
                mm_cols=mm_cols)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _BSM[name] = case
    return case


def test_bsm_base_blocks_reach_the_tier_2_queue_and_the_arbitration(oracle):
    """What the OEU cases rely on, from the oracle alone: a fifth of the rows fails the verdict, a few per cent sit in the band."""
    for name in ("oeu7", "oeu12"):
        c = bsm_case(oracle, name)
        inbox = c["st"] != 1
        assert inbox.sum() == PERIOD - PERIOD // 8 - 2
        assert 0.1 < np.mean(c["st"] == 2) < 0.3
        band = inbox & ~_decided(c["r80"])
        assert 0 < band.sum() <= BAND_SHARE_MAX * PERIOD


def exact_rows(c, rows):
    from exact_mp import exact_flux_avg, mp_flux_avg
    if c["mm_cols"] is None:
        return exact_flux_avg(rows, c["tex"].name, c["dim"], c["src"], BIN_EDGES)
    a, b = c["mm_cols"][0], c["mm_cols"][-1] + 1
    return np.array([[float(v) for v in mp_flux_avg(list(map(float, r)), tuple(map(float, r[a:b])), c["dim"], c["src"], BIN_EDGES)]
                     for r in rows])


def check_bsm(c, got, idx, propagate=False):
    """The outputs of a launch against the oracle's on the base block, row idx[i] for walker i; the bars of test_gpu_parity.py's
    test_bsm_random_vs_oracle."""
    lp, fr, st = got
    inbox = (c["st"] != 1)[idx]                                      # the oracle's prior box (NaN fails it)
    ref_st = (c["pst"] if propagate else c["st"])[idx]
    ref_fr = (c["pfr"] if propagate else c["fr"])[idx]
    r80 = c["r80"][idx]
    evaluated = inbox & ((ref_st == 0) | (ref_st == 2))
    dec = _decided(r80) & evaluated
    assert np.mean(evaluated & ~dec) <= BAND_SHARE_MAX
    if lp is not None:
        assert np.array_equal(np.isneginf(lp), ~inbox) and not np.isposinf(lp).any()
    if st is not None:
        flagged = st == _lib.GF_ST_NON_UNITARY
        assert np.array_equal(flagged[dec], (ref_st == 2)[dec])
        if propagate:                                                # no prior: a row outside the box is evaluated, whatever comes of it
            assert not (st[inbox] == _lib.GF_ST_OUT_OF_PRIOR).any()
        else:
            assert np.array_equal(st == _lib.GF_ST_OUT_OF_PRIOR, ~inbox)
        if lp is not None:
            assert np.array_equal(np.isnan(lp), flagged | (st == _lib.GF_ST_NAN))
        assert not (st[evaluated] == _lib.GF_ST_NAN).any()
        good = (ref_st == 0) & (st == _lib.GF_ST_OK)
    else:
        good = (ref_st == 0) & dec                                   # no verdict was computed: the rows the oracle clearly passes
    clean = good & (r80 < 1e-13)
    assert clean.sum() > 0.4 * len(idx)                              # (half of the base rows, by the oracle)
    if lp is not None:
        fin = clean & np.isfinite(c["lp"][idx])
        assert rel_err(lp[fin], c["lp"][idx][fin]) <= REL
    if fr is not None:
        if not propagate:
            assert np.isnan(fr[~inbox]).all()
        err = np.abs(fr - ref_fr).max(axis=1)
        assert err[clean].max() <= ABS_FR
        over = np.flatnonzero(good & ~(err <= ABS_FR + 10.0 * r80))
        if over.size:
            # just under the reference's own threshold the 80-bit closed form can be off by more than ten times its unitarity defect:
            # 60-digit arithmetic arbitrates, and the kernel must be the accurate one
            assert over.size <= 0.005 * good.sum(), (over.size, good.sum())
            first = over[np.unique(idx[over], return_index=True)[1]]
            pick = first[np.argsort(err[first])[::-1][:8]]
            exact = exact_rows(c, c["base"][idx[pick]])
            assert np.abs(fr[pick] - exact).max() <= 1e-11
            assert np.all(np.abs(ref_fr[pick] - exact).max(axis=1) > np.abs(fr[pick] - exact).max(axis=1))
        assert np.abs(fr[good].sum(axis=1) - 1).max() < 1e-13


def bsm_batch(oracle, name, layout, outputs, propagate=False):
    """One launch of the whole batch and one of the base block alone; both checked against the oracle and against each other, bit
    for bit.  Returns the batch's outputs."""
    c = bsm_case(oracle, name)
    base, nd = c["base"], c["base"].shape[1]
    with Model(compile_model(c["ps"], "BSM_GAUSS", **c["kw"])) as m:
        _, n = batch_rows(m)
        idx = np.arange(n) % PERIOD
        block = launch_rows(m, base, layout, outputs, propagate)    # sub-capacity: several lanes per walker, no prefetch
        big = launch_rows(m, np.resize(base, (n, nd)), layout, outputs, propagate)
    check_bsm(c, block, np.arange(PERIOD), propagate)
    check_bsm(c, big, idx, propagate)
    for k in range(3):
        assert (big[k] is None) == (block[k] is None)
        if big[k] is not None:
            assert same_bits(big[k], block[k][idx]), (name, layout, outputs, propagate, "lnprob fr status".split()[k])
    return big


BSM_CASES = [("oeu7", True, False), ("oeu7", False, False), ("oeu7", True, True), ("oeu12", True, False), ("oeu12", False, False),
             ("none11", True, False)]


@pytest.mark.parametrize("name,outputs,propagate", BSM_CASES,
                         ids=["%s-%s-%s" % (c, "propagate" if p else "lnprob", "status" if o else "bare") for c, o, p in BSM_CASES])
def test_bsm_rows_past_one_pass(oracle, name, outputs, propagate):
    """From rows: the prefetching instances (7 and 12 columns; the generic width stages every tile itself), with the deferred tier 2
    and the arbitration behind them when a status is requested."""
    big = bsm_batch(oracle, name, GF_LAYOUT_AOS, outputs, propagate)
    if outputs and name != "none11":
        assert 0.1 < np.mean(big[2] == _lib.GF_ST_NON_UNITARY) < 0.3


@pytest.mark.parametrize("name", ["oeu7", "oeu12"])
def test_bsm_columns_past_one_pass_equal_rows(oracle, name):
    """From columns there is no prefetch; the result is the one from rows, bit for bit.  The columns go first, onto a stream whose
    verdict queues are new and so grow to exactly n walkers: a ragged n must still be one piece (columns cannot be cut)."""
    _lib.device_trim()
    soa = bsm_batch(oracle, name, GF_LAYOUT_SOA, True)
    aos = bsm_batch(oracle, name, GF_LAYOUT_AOS, True)
    for a, b in zip(soa, aos):
        assert same_bits(a, b)


# ---- the stride loops of k_haar, k_flavor_hist, k_cube_to_theta -----------------------------------------------------------------------
HAAR_SRC = np.array([1., 2., 0.]) / 3


@pytest.fixture(scope="module")
def prior_model():
    m = Model(compile_model(Cf.unitary_paramset(), "PRIOR_ONLY", source_ratio=HAAR_SRC))
    yield m
    m.close()


def haar_window(model, oracle, seed, first, n):
    g_ang, g_fr = Guarded(model, 4 * n), Guarded(model, 3 * n)
    model.haar_draw_device(seed, first, n, g_ang.ptr, g_fr.ptr)
    model.sync()
    ang, fr = g_ang.take(4), g_fr.take(3)
    ofr, oang = oracle.haar_draw(HAAR_SRC, seed, n, first=first)
    assert same_bits(ang, oang)                                      # the oracle's Philox stream
    assert np.abs(fr - ofr).max() <= ABS_FR


def test_haar_draws_past_one_pass(prior_model, oracle):
    p, _ = batch_rows(prior_model)
    haar_window(prior_model, oracle, 26, 0, 2 * p + 7)


def test_haar_window_across_the_counter_word(prior_model, oracle):
    haar_window(prior_model, oracle, 26, 2 ** 32 - 1000, 2000)


def test_flavor_histogram_past_one_pass(prior_model):
    p, _ = batch_rows(prior_model)
    n, nb = 2 * p + 7, 21
    rng = np.random.default_rng(21)
    fr = rng.dirichlet((1., 1., 1.), n)
    e = np.linspace(0.0, 1.0, nb + 1)
    special = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [-0.0, -5e-324, 1.5, np.nan, np.inf, -np.inf]])
    k = rng.permutation(n)[:n // 16]
    fr[k, rng.integers(0, 3, k.size)] = special[rng.integers(0, special.size, k.size)]
    assert np.array_equal(prior_model.flavor_histogram(fr, nb), reference_hist(fr, nb))


def test_cube_map_past_one_pass(oracle):
    """k_cube_to_theta over 2 * pass_items + 7 elements and more (the smallest whole number of rows that has them): lnprob and status
    of gf_lnprob_cube_batch are those of gf_lnprob_batch on the rows mn.py:36's expression gives on the host, bit for bit.  Two of the
    scanned columns start at -1 and at 0.5 pi, so the map's product and sum are told apart from a fused one."""
    nbl = list(Cf.notebook_paramsets(NB_ANGLES)[1])
    nbl[3] = Param(name="dcp", value=nbl[3].value, ranges=[0.5 * np.pi, 2 * np.pi], std=nbl[3].std, tag=nbl[3].tag)
    ps = ParamSet(nbl)
    kw = dict(bestfit_fr=(0.55, 0.18, 0.27), smearing=0.02)
    cols = np.array([0, 3, 5], dtype=np.int32)
    with Model(compile_model(ps, "SM_GAUSS", **kw)) as m, Model(compile_model(ps, "SM_GAUSS", **kw)) as m2:
        p, _ = batch_rows(m)
        nd = len(ps)
        n = -(-(2 * p + 7) // nd)
        assert 2 * p + 7 <= n * nd < 2 * p + 7 + nd
        rng = np.random.default_rng(6)
        cube = rng.uniform(0.0, 1.0, (n, len(cols)))
        cube[::1001, 0] = 1.5                                        # outside the box
        base = uniform_theta(ps, 1, rng, seeds=True)[0]
        th = np.tile(base, (n, 1))
        for k, c in enumerate(cols):
            lo, hi = m.desc.lo[c], m.desc.hi[c]
            th[:, c] = (hi - lo) * cube[:, k] + lo
        assert m.desc.lo[3] != 0.0 and m.desc.lo[5] == -1.0
        # the cube batch first, on a model whose staging has never held these rows
        lp = np.full(n, np.nan).view(np.uint64)
        lp[:] = SENTINEL_F64
        lp = lp.view(np.float64)
        st = np.full(n, SENTINEL_I32, dtype=np.int32)
        _lib.check(m._L.gf_lnprob_cube_batch(m._h, cube.ctypes.data_as(_lib._dp), n, len(cols), cols.ctypes.data_as(_lib._ip),
                                             base.ctypes.data_as(_lib._dp), lp.ctypes.data_as(_lib._dp), None, st.ctypes.data_as(_lib._ip)),
                   "gf_lnprob_cube_batch")
        want_lp, want_st = m2.lnprob(th)
    assert same_bits(lp, want_lp) and np.array_equal(st, want_st)
    assert (st[::1001] == _lib.GF_ST_OUT_OF_PRIOR).all() and np.isfinite(lp).sum() > 0.99 * n
    ref = oracle.lnprob_batch(oracle.make_model(ps, "SM_GAUSS", **kw), th[:PERIOD])
    assert rel_err(lp[:PERIOD], ref) <= REL
