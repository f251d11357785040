"""GPU: the tempered ensemble sampler (csrc/gf_temper.hip, csrc/gf_temper_host.hip) at the shapes its launch arithmetic
has and tests/test_gpu_temper.py -- the 12-column posterior at 24 walkers -- does not reach: k_stretch_tempered with more than one block
per chain and at the row widths 7 and 11 (the <7> and <0> instances, every lane count), k_pt_swap past one block and at the ladder's
edges (2 rungs, 7 rungs, 1 and 3 groups, the plateau lnl = -inf, the failing region), k_pt_series past one pass of its walker loop and
over a stored chain that was repacked.  The yardsticks are tests/test_gpu_temper.py's, imported: the numpy stretch move on the
sampler's Philox stream fed T = lp + beta lnl from `Model.lnprior_lnlike`, the numpy restatement of the round, the host build of
csrc/gf_temper.hpp.  Every comparison is bit for bit; the one tolerance is check_split's REL on lnprior against the oracle.
profiles/temper_shapes/README.txt has the instances each test executes."""
import numpy as np
import pytest

import stretch_ref
from common import BIN_EDGES
from golemflavor_amd import _lib
from golemflavor_amd import fr as fr_utils
from golemflavor_amd.enums import Texture
from stretch_ref import reference_stretch
from test_gpu_binned_sampler import assert_same_run, bsm_model, device_run, paramset_of, same_bits
from test_gpu_table_sampler import forced_lpw
from test_gpu_temper import (BETAS3, NW, check_split, failing_rows, numpy_T, numpy_tempered, posts, prior_draws,  # noqa: F401 (posts: a fixture)
                             series_against_host, state_holds_the_formula, tempered)

pytestmark = pytest.mark.gpu

BLOCK = 256                                # GF_BLOCK: the threads of a workgroup of every kernel here
# (lanes per walker, walkers) with nhalf * lpw just past 256: the second block holds 80, 12, 6 and 3 valid threads -- at 16 lanes one full
# wave and a quarter of the next
TWO_BLOCKS = [(16, 42), (4, 134), (2, 262), (1, 518)]
SRC_B = (1., 2., 0.)


def blocks_per_chain(nw, lpw):
    """gf_launch_stretch_tempered's grid.x"""
    return (nw // 2 * lpw + BLOCK - 1) // BLOCK


def second_block_moves(ref, nw, lpw):
    """accepted moves of the walkers whose slot k >= 256 / lpw, in either half: the second block's"""
    nhalf, first = nw // 2, BLOCK // lpw
    return int(ref["nacc"][:, first:nhalf].sum() + ref["nacc"][:, nhalf + first:].sum())


def check_launch(smp, lpw):
    shape = smp.launch_shape()
    assert shape["shape"] == "grid" and shape["lanes_per_walker"] == lpw, shape


def swap_counts_are(smp, ref):
    prop, acc = smp.swap_counts()
    assert np.array_equal(prop.reshape(-1), ref["counts"][:, 0]) and np.array_equal(acc.reshape(-1), ref["counts"][:, 1]), (prop, acc, ref["counts"])
    print("proposed\n%s\naccepted\n%s" % (prop, acc))
    return prop, acc


# ---- A. the half-step past one block per chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw, nw", TWO_BLOCKS)
def test_two_blocks_per_chain_on_the_plateau(oracle, posts, lpw, nw):
    """sens posterior at smearing 0.02, 3 chains at BETAS3 on streams (11, 3, 40), 6 steps at thin 2: stored and non-stored steps
    alternate in a launch of two blocks per chain, the second one partly filled"""
    assert blocks_per_chain(nw, lpw) >= 2 and 0 < nw // 2 * lpw - BLOCK <= 80
    f = posts["s002"]
    ids = (11, 3, 40)
    p0 = prior_draws(posts["ps"], 3 * nw, np.random.default_rng(100 + lpw)).reshape(3, nw, 12)
    with forced_lpw(lpw):
        smp = tempered(f, BETAS3, nw=nw, seed=23, stream_ids=ids)
        try:
            smp.run_mcmc(p0, 6, thin=2)
            check_launch(smp, lpw)
            ref = reference_stretch(oracle, [(f.model, b) for b in BETAS3], p0, 6, 23, lnprob=numpy_T, full=True, thin=2, stream_ids=ids)
            got = device_run(smp)
            assert got["chain"].shape == (3, 3, nw, 12)
            assert_same_run(got, ref, "plateau, %d walkers at %d lanes: %d blocks per chain" % (nw, lpw, blocks_per_chain(nw, lpw)))
            print("moves of the second block's walkers: %d" % second_block_moves(ref, nw, lpw))
            assert second_block_moves(ref, nw, lpw) > 0
        finally:
            smp.close()


def failing_two_blocks(oracle, posts, lpw, nw, seed_p0, seed):
    """the run below; returns (proposals of the second block's slots inside stretch_ref.BAND, those of them that were accepted)"""
    f, ps = posts["oeu"], posts["oeu_ps"]
    p0 = failing_rows(ps, 3 * nw, np.random.default_rng(seed_p0)).reshape(3, nw, 12)
    nhalf, first = nw // 2, BLOCK // lpw                                 # slots first .. nhalf - 1 are the second block's
    seen = []                                                            # every set of rows the reference evaluates, in its order

    def recording_T(om, q):
        seen.append(np.array(q))
        return numpy_T(om, q)

    with forced_lpw(lpw):
        smp = tempered(f, BETAS3, nw=nw, seed=seed)
        try:
            smp.run_mcmc(p0, 6)
            check_launch(smp, lpw)
            ref = reference_stretch(oracle, [(f.model, b) for b in BETAS3], p0, 6, seed, lnprob=recording_T, full=True)
            got = device_run(smp)
            assert_same_run(got, ref, "failing region, %d walkers at %d lanes" % (nw, lpw))
            print("parked %d, non-unitary %d" % (smp.parked_proposals, smp.nonunitary_proposals))
            assert smp.parked_proposals > 0 and smp.nonunitary_proposals > 0
            # no sample the reference would have died on is in any chain
            st = f.model.lnprior_lnlike(got["chain"].reshape(-1, 12))[2]
            moved = np.isfinite(got["lnp_chain"].reshape(-1))
            assert not np.any(st[moved] == _lib.GF_ST_NON_UNITARY)
        finally:
            smp.close()
    # the reference's proposals: 3 evaluations of the start, then one set of rows per (step, half, chain)
    assert len(seen) == 3 + 6 * 2 * 3
    om = oracle.make_model(ps, "BSM_GAUSS", texture="OEU", dimension=6, binning=BIN_EDGES, source_ratio=(1 / 3, 2 / 3, 0.),
                           bestfit_fr=fr_utils.angles_to_fr(fr_utils.fr_to_angles((1, 1, 1))), smearing=0.3)
    in_band = accepted_in_band = 0
    for it in range(6):
        for half in (0, 1):
            for c in range(3):
                q = seen[3 + (it * 2 + half) * 3 + c][first:]
                res = oracle.unitarity_residual_batch(om, q)
                band = (res > stretch_ref.BAND[0]) & (res < stretch_ref.BAND[1])
                took = np.all(ref["chain"][c, it, half * nhalf + first:(half + 1) * nhalf] == q, axis=1)
                in_band += int(band.sum())
                accepted_in_band += int(np.sum(band & took))
    print("slots %d .. %d: %d proposals in the band, %d of them accepted" % (first, nhalf - 1, in_band, accepted_in_band))
    return in_band, accepted_in_band


# lanes per walker -> (seed of the start, seed of the sampler).  (52, 29) are the 24-walker test's; at 134 walkers that start puts 3
# proposals of the slots 64 .. 66 into the band and none of them is accepted, the next start 7, of which 4 are
FAILING_SEEDS = {16: (52, 29), 4: (53, 29), 2: (52, 29), 1: (52, 29)}


@pytest.mark.parametrize("lpw, nw", TWO_BLOCKS)
def test_two_blocks_per_chain_through_the_failing_region(oracle, posts, lpw, nw):
    """texture OEU from a failing_rows start, 6 steps: proposals are parked in both blocks and k_stretch_settle completes rows
    chain * nhalf + k with k beyond the first block.

    Which proposal was parked is not visible from the host: `Model.lnprior_lnlike` returns the status after the exact verdict, and
    `parked_proposals` is one count for the whole sampler.  So the condition on the second block is the other one: the number of
    accepted moves in the slots k >= 256 / lpw whose proposal has its unitarity residual (the oracle's) inside stretch_ref.BAND, the
    half decade around the reference's threshold in which the in-kernel tiers leave the verdict to k_stretch_settle."""
    assert blocks_per_chain(nw, lpw) >= 2
    _, accepted_in_band = failing_two_blocks(oracle, posts, lpw, nw, *FAILING_SEEDS[lpw])
    assert accepted_in_band > 0, "no accepted move of the second block's slots had its proposal in the band"


# ---- B. row widths 7 and 11 ---------------------------------------------------------------------------------------------------------------
OEU_ANGLES = (0.5, 1.0, 0.0, 0.0)          # the new-physics mixing angles texture OEU fixes: a corner of the 11-column posterior's box


def width_model(width, tex=Texture.OEU, source=SRC_B):
    """(Model, paramset, the oracle's keywords): the flux-averaged BSM model of `width` columns (11: the texture is NONE, forced)"""
    m, ps = bsm_model(width, 6, tex, source=source)
    okw = dict(texture=(paramset_of(width, 6)[1] or tex).name, dimension=6, binning=BIN_EDGES, source_ratio=source, bestfit_fr=(1 / 3,) * 3,
               smearing=0.02)
    return m, ps, okw


def lower_scale_rows(ps, n, rng):
    """prior draws with the scale in the lower 60 % of its range (scale_rows of tests/test_gpu_binned_sampler.py, on the prior)"""
    th = prior_draws(ps, n, rng)
    lo, hi = ps[len(ps) - 1].ranges
    th[:, -1] = rng.uniform(lo, lo + 0.6 * (hi - lo), n)
    return th


@pytest.mark.parametrize("width", [7, 11])
def test_split_evaluation_at_widths_7_and_11(oracle, width):
    """About 1 000 rows through k_lnprior_lnl at ndim = 7 and 11: prior draws, rows just outside the box in every column in turn (below
    and above), rows with the scale across the top quarter of its range.  Texture OEU is non-unitary there; at 11 columns the
    new-physics angles are columns, and the rows of the last kind carry OEU's angles -- a corner of the box, inside it."""
    m, ps, okw = width_model(width)
    om = oracle.make_model(ps, "BSM_GAUSS", **okw)
    rng = np.random.default_rng(200 + width)
    with m:
        draws = prior_draws(ps, 512, rng)
        far = prior_draws(ps, 16 * width, rng)
        for i in range(len(far)):
            c = i % width
            lo, hi = ps[c].ranges
            far[i, c] = lo - (hi - lo) * 0.01 * (1 + i % 7) if (i // width) % 2 else hi + (hi - lo) * 0.01 * (1 + i % 5)
        top = prior_draws(ps, 1000 - 512 - 16 * width, rng)
        lo, hi = ps[width - 1].ranges
        top[:, -1] = rng.uniform(hi - 0.25 * (hi - lo), hi, len(top))
        if width == 11:
            top[:, 6:10] = OEU_ANGLES
        th = np.concatenate([draws, far, top])
        lp, lnl, st = check_split(oracle, m, om, th, "%d columns" % width)
    counts = {k: int(np.sum(st == v)) for k, v in (("ok", _lib.GF_ST_OK), ("out", _lib.GF_ST_OUT_OF_PRIOR), ("nonunitary", _lib.GF_ST_NON_UNITARY))}
    print("%d columns, %d rows: %s" % (width, len(th), counts))
    assert len(th) == 1000 and counts["ok"] > 0 and counts["nonunitary"] > 0
    assert np.all(st[512:512 + len(far)] == _lib.GF_ST_OUT_OF_PRIOR) and counts["out"] == len(far)
    assert np.sum(st[512 + len(far):] == _lib.GF_ST_NON_UNITARY) > 0 and np.sum(st[512 + len(far):] == _lib.GF_ST_OK) > 0


_REFS = {}


def shared(key, make):
    """the numpy run of a shape, computed by the first lane count that asks for it and read-only from then on"""
    if key not in _REFS:
        ref = make()
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.mark.parametrize("lpw", [1, 2, 4, 16])
@pytest.mark.parametrize("width", [7, 11])
def test_half_step_at_widths_7_and_11(oracle, width, lpw):
    """the <7> and <0> instances of k_stretch_tempered at every lane count: 3 chains at BETAS3, the smallest legal ensemble (14 and 22
    walkers), 12 steps"""
    nw = 2 * width
    m, ps, _ = width_model(width)
    with m:
        p0 = lower_scale_rows(ps, 3 * nw, np.random.default_rng(300 + width)).reshape(3, nw, width)
        with forced_lpw(lpw):
            smp = tempered(m, BETAS3, nw=nw, seed=61, ndim=width)
            smp.on_nonunitary = "-inf"
            try:
                smp.run_mcmc(p0, 12)
                check_launch(smp, lpw)
                ref = shared(("half-step", width), lambda: reference_stretch(oracle, [(m, b) for b in BETAS3], p0, 12, 61, lnprob=numpy_T, full=True))
                assert_same_run(device_run(smp), ref, "%d columns, %d walkers, %d lanes per walker" % (width, nw, lpw))
            finally:
                smp.close()


@pytest.mark.parametrize("lpw", [1, 16])
@pytest.mark.parametrize("width", [7, 11])
def test_half_step_parks_at_widths_7_and_11(oracle, width, lpw):
    """the same chains started with the scale over [-40, -30], where texture OEU fails (at 11 columns every walker carries OEU's
    angles, and a stretch move between two such walkers leaves them exactly): the <7> and <0> instances park rows of their own width
    and k_stretch_settle completes them"""
    nw = 2 * width
    m, ps, _ = width_model(width)
    with m:
        rng = np.random.default_rng(330 + width)
        p0 = prior_draws(ps, 3 * nw, rng)
        p0[:, -1] = rng.uniform(-40.0, -30.0, len(p0))
        if width == 11:
            p0[:, 6:10] = OEU_ANGLES
        p0 = p0.reshape(3, nw, width)
        with forced_lpw(lpw):
            smp = tempered(m, BETAS3, nw=nw, seed=73, ndim=width)
            smp.on_nonunitary = "-inf"
            try:
                smp.run_mcmc(p0, 12)
                check_launch(smp, lpw)
                ref = shared(("parking", width), lambda: reference_stretch(oracle, [(m, b) for b in BETAS3], p0, 12, 73, lnprob=numpy_T, full=True))
                got = device_run(smp)
                assert_same_run(got, ref, "%d columns from the failing region, %d lanes per walker" % (width, lpw))
                print("parked %d, non-unitary %d" % (smp.parked_proposals, smp.nonunitary_proposals))
                assert smp.parked_proposals > 0 and smp.nonunitary_proposals > 0
                st = m.lnprior_lnlike(got["chain"].reshape(-1, width))[2]
                assert not np.any(st[np.isfinite(got["lnp_chain"].reshape(-1))] == _lib.GF_ST_NON_UNITARY)
            finally:
                smp.close()


@pytest.mark.parametrize("width", [7, 11])
def test_two_blocks_per_chain_at_widths_7_and_11(oracle, width):
    """42 walkers at 16 lanes per walker: the tile stride lane * ndim of the <7> and <0> instances in a second, partly filled block"""
    lpw, nw = TWO_BLOCKS[0]
    assert blocks_per_chain(nw, lpw) >= 2
    m, ps, _ = width_model(width)
    with m:
        p0 = lower_scale_rows(ps, 3 * nw, np.random.default_rng(310 + width)).reshape(3, nw, width)
        with forced_lpw(lpw):
            smp = tempered(m, BETAS3, nw=nw, seed=67, ndim=width)
            smp.on_nonunitary = "-inf"
            try:
                smp.run_mcmc(p0, 6)
                check_launch(smp, lpw)
                ref = reference_stretch(oracle, [(m, b) for b in BETAS3], p0, 6, 67, lnprob=numpy_T, full=True)
                assert_same_run(device_run(smp), ref, "%d columns, %d walkers, %d lanes per walker" % (width, nw, lpw))
                print("moves of the second block's walkers: %d" % second_block_moves(ref, nw, lpw))
                assert second_block_moves(ref, nw, lpw) > 0
            finally:
                smp.close()


@pytest.mark.parametrize("width", [7, 11])
def test_series_and_swaps_at_widths_7_and_11(oracle, width):
    """two groups with different models (7 columns: textures OEU and OET; 11 columns: two sources), betas [1, 0.3, 0], a round every
    2 steps, 6 steps: chain, state and swap counts against the numpy round, k_pt_series against the host build"""
    nw, betas = 2 * width, [1.0, 0.3, 0.0]
    a, ps, _ = width_model(width)
    b, _, _ = width_model(width, tex=Texture.OET, source=(0., 1., 0.))
    with a, b:
        models = [a, b]
        p0 = lower_scale_rows(ps, 6 * nw, np.random.default_rng(320 + width)).reshape(6, nw, width)
        ids = (4, 9, 14, 1, 6, 11)
        smp = tempered(models, betas, nw=nw, seed=71, swap_every=2, ngroups=2, stream_ids=ids, ndim=width)
        smp.on_nonunitary = "-inf"
        try:
            smp.run_mcmc(p0, 6)
            ref = numpy_tempered(oracle, models, betas, p0, 6, 71, 2, ids)
            got = device_run(smp)
            assert_same_run(got, ref, "%d columns, a round every 2 steps" % width)
            prop, _ = swap_counts_are(smp, ref)
            assert prop[:, :2].min() > 0 and np.all(prop[:, 2] == 0)           # rounds 0 and 2 take the pair (0, 1), round 1 the pair (1, 2)
            state_holds_the_formula(smp, models, betas, got)
            ser, _ = series_against_host(smp, models, betas)
            assert ser.shape == (6, 6, 5) and np.all(ser[:, :, 0] > 0)
        finally:
            smp.close()


# ---- C. the swap kernel past one block and at the ladder's edges ----------------------------------------------------------------------------
def swapped_run(oracle, fns, models, betas, p0, nsteps, seed, swap_every, ngroups, ids, what, rounds=None):
    """the device's run and the numpy one: chain, state and swap counts bit for bit.  Returns (got, ref, proposed, accepted)."""
    smp = tempered(fns, betas, nw=p0.shape[1], seed=seed, swap_every=swap_every, ngroups=ngroups, stream_ids=ids)
    try:
        smp.run_mcmc(p0, nsteps)
        ref = numpy_tempered(oracle, models, betas, p0, nsteps, seed, swap_every, ids, rounds=rounds)
        got = device_run(smp)
        assert_same_run(got, ref, what)
        prop, acc = swap_counts_are(smp, ref)
        state_holds_the_formula(smp, models, betas, got)
        return got, ref, prop, acc
    finally:
        smp.close()


def test_swaps_in_three_blocks(oracle, posts):
    """134 walkers, two groups with different models, 4 rungs, a round after each of 4 steps: an even round has 2 * 2 * 134 = 536
    threads in three blocks, thread (group * npairs + pair) * 134 + walker.  Walker 10 of group 1's rung 1 starts outside the support:
    its pair with rung 0 is thread 278 of an even round, in the second block, and is never counted."""
    nw, betas = 134, [1.0, 0.3, 0.05, 0.0]
    assert (2 * 2 * nw + BLOCK - 1) // BLOCK == 3 and BLOCK <= (1 * 2 + 0) * nw + 10 < 2 * BLOCK
    fns = [posts["s01"], posts["out01"]]
    p0 = prior_draws(posts["ps"], 8 * nw, np.random.default_rng(401)).reshape(8, nw, 12)
    p0[5, 10, 0] = 1e6
    ids = tuple(range(10, 34, 3))
    got, ref, prop, acc = swapped_run(oracle, fns, [f.model for f in fns], betas, p0, 4, 37, 1, 2, ids, "134 walkers, 4 rungs, 2 groups")
    assert acc.sum() > 0 and np.all(prop[:, -1] == 0)
    # rounds 0 and 2 take the pairs (0, 1) and (2, 3), rounds 1 and 3 the pair (1, 2)
    assert np.all(prop[0, :3] <= 2 * nw) and prop[1, 0] <= 2 * (nw - 1) and prop[1, 1] <= 2 * (nw - 1) and prop[1, 2] <= 2 * nw
    assert np.all(prop[:, :3] > nw)
    assert got["lnp"][5, 10] == -np.inf and got["pos"][5, 10, 0] == 1e6


def test_swaps_on_a_ladder_of_two_rungs(oracle, posts):
    """ntemps = 2: an odd round holds no pair -- npairs = 0, and k_pt_swap must not divide by it.  Six single-step runs with a round
    after each: an odd round leaves counters and walkers as they were, an even one proposes at most nwalkers pairs per group; then
    the whole against the numpy run of 6 steps."""
    fns, betas = [posts["s01"], posts["out01"]], [1.0, 0.3]
    models = [f.model for f in fns]
    p0 = prior_draws(posts["ps"], 4 * NW, np.random.default_rng(402)).reshape(4, NW, 12)
    smp = tempered(fns, betas, seed=41, swap_every=1, ngroups=2)
    try:
        before = np.zeros((2, 2), dtype=np.uint32)
        for step in range(6):
            smp.run_mcmc(p0 if step == 0 else None, 1)
            prop, acc = smp.swap_counts()
            got = device_run(smp)
            assert np.all(prop[:, 1] == 0) and np.all(acc[:, 1] == 0)
            if step % 2:
                assert np.array_equal(prop, before) and same_bits(got["pos"], got["chain"][:, -1]) and same_bits(got["lnp"], got["lnp_chain"][:, -1])
            else:
                assert np.all(prop[:, 0] - before[:, 0] <= NW) and np.all(prop[:, 0] > before[:, 0])
            before = prop
        ref = numpy_tempered(oracle, models, betas, p0, 6, 41, 1)
        assert_same_run(got, ref, "2 rungs, a round after every step")
        prop, acc = swap_counts_are(smp, ref)
        assert acc.sum() > 0 and np.all(prop[:, 0] <= 3 * NW)
        state_holds_the_formula(smp, models, betas, got)
    finally:
        smp.close()


@pytest.mark.parametrize("ngroups", [1, 3])
def test_swaps_on_a_ladder_of_seven_rungs(oracle, posts, ngroups):
    """ntemps = 7: three pairs in every round, (0, 1) (2, 3) (4, 5) and (1, 2) (3, 4) (5, 6); one group, and three groups of one model;
    a round every 2 steps, 8 steps"""
    f, betas = posts["s01"], [1.0, 0.5, 0.25, 0.1, 0.03, 0.01, 0.0]
    nch = 7 * ngroups
    p0 = prior_draws(posts["ps"], nch * NW, np.random.default_rng(403 + ngroups)).reshape(nch, NW, 12)
    ids = tuple(range(5, 5 + 2 * nch, 2))
    _, _, prop, acc = swapped_run(oracle, f, [f.model] * ngroups, betas, p0, 8, 43, 2, ngroups, ids, "7 rungs, %d group(s)" % ngroups)
    assert prop.shape == (ngroups, 7) and np.all(prop[:, :6] > 0) and np.all(prop[:, :6] <= 2 * NW) and np.all(prop[:, 6] == 0)
    assert acc.sum() > 0


def test_swaps_on_the_plateau(oracle, posts):
    """smearing 0.02, betas [1, 0.25, 0], a round after each of 8 steps: the prior rung's walkers on the plateau lnl = -inf are live
    (T = lp), their pairs with rung 1 are proposed, and the log-ratio -inf (or NaN, both sides on the plateau cannot be: T would be
    -inf) rejects them"""
    f, betas = posts["s002"], BETAS3
    p0 = prior_draws(posts["ps"], 3 * NW, np.random.default_rng(405)).reshape(3, NW, 12)
    rounds = []
    got, ref, prop, acc = swapped_run(oracle, f, [f.model], betas, p0, 8, 47, 1, 1, None, "the plateau, a round after every step", rounds)
    assert len(rounds) == 8
    rejected = 0
    for r in rounds:
        for t in range(r["round"] % 2, 2, 2):
            live = (r["T"][t] > -np.inf) & (r["T"][t + 1] > -np.inf)
            same = np.all(r["pos"][t] == r["pos_after"][t], axis=1)
            rejected += int(np.sum(live & (r["lnl"][t + 1] == -np.inf) & same))
            assert not np.any(live & (r["lnl"][t + 1] == -np.inf) & ~same)
    print("proposed pairs with lnl = -inf on the hotter side, all rejected: %d" % rejected)
    assert rejected > 0 and acc.sum() > 0
    lnl = f.model.lnprior_lnlike(got["pos"][2])[1]
    assert np.sum((lnl == -np.inf) & np.isfinite(got["lnp"][2])) > 0


def test_swaps_through_the_failing_region(oracle, posts):
    """texture OEU from a failing_rows start, BETAS3, a round every 2 steps, 8 steps: the round's split evaluation meets rows that are
    not OK -- walkers still at a start the reference would have died on, lnl = NaN -- and goes through its own arbitration queue"""
    f, betas = posts["oeu"], BETAS3
    p0 = failing_rows(posts["oeu_ps"], 3 * NW, np.random.default_rng(406)).reshape(3, NW, 12)
    rounds = []
    swapped_run(oracle, f, [f.model], betas, p0, 8, 53, 2, 1, None, "the failing region, a round every 2 steps", rounds)
    assert len(rounds) == 4
    not_ok = [int(np.sum(r["status"] != _lib.GF_ST_OK)) for r in rounds]
    print("rows of a round's split evaluation that are not OK: %s" % not_ok)
    assert sum(not_ok) > 0 and all(np.all(np.isnan(r["lnl"][r["status"] == _lib.GF_ST_NON_UNITARY])) for r in rounds)


# ---- D. the series kernel past one pass ---------------------------------------------------------------------------------------------------
SERIES_BETAS = [1.0, 0.4, 0.1, 0.0]


def series_run(posts, nw, runs, seed=53):
    """tests/test_gpu_temper.py's series case: s002, rung 1 outside the support, a round every 2 steps; `runs`: the steps of each call"""
    f = posts["s002"]
    p0 = prior_draws(posts["ps"], 4 * nw, np.random.default_rng(71)).reshape(4, nw, 12)
    p0[1, :, 0] = 1e6
    smp = tempered(f, SERIES_BETAS, nw=nw, seed=seed, swap_every=2)
    try:
        for i, n in enumerate(runs):
            smp.run_mcmc(p0 if i == 0 else None, n)
        ser, lnl = series_against_host(smp, [f.model], SERIES_BETAS)
        assert same_bits(smp.lnlikelihood(), lnl.transpose(0, 2, 1))
        return ser, lnl
    finally:
        smp.close()


@pytest.mark.parametrize("nw", [258, 600])
def test_series_past_one_pass(posts, nw):
    """258 walkers: lanes 0 and 1 add two walkers, every other lane one; 600: three passes, the last one partial.  All five outputs
    and lnl against the host build (tests/test_temper_host.py pins its order at 257 and 600 walkers)."""
    assert nw > BLOCK
    ser, lnl = series_run(posts, nw, [3])
    assert ser.shape == (4, 3, 5) and lnl.shape == (4, 3, nw)
    assert np.all(ser[1, :, 0] == 0) and np.all(ser[1, :, 1] == 0) and np.all(ser[1, :, 2] == -np.inf) and np.all(ser[1, :, 3:] == 0)
    assert np.all(ser[0, :, 0] > 0) and np.any(ser[3, :, 0] < nw)
    assert np.any(np.isfinite(lnl[[0, 2, 3], :, BLOCK:]))                    # the later passes hold values that count


def test_series_of_a_repacked_chain(posts):
    """70 stored steps of 24 walkers in runs of 40 and 30: the first run's capacity is 64 steps, the second one grows it and repacks the
    40 stored steps between two rounds.  The series of all 70 against the host build, and its first 64 steps against a single run of
    64 steps on the same seed, which never repacks."""
    ser, lnl = series_run(posts, NW, [40, 30])
    assert ser.shape == (4, 70, 5)
    ser64, lnl64 = series_run(posts, NW, [64])
    assert same_bits(ser[:, :64], ser64) and same_bits(lnl[:, :64], lnl64)
    assert len(np.unique(ser[0, :, 1])) > 10                                # the cold chain moves
