"""CPU: the rules behind the post-processing kernels, pinned to published or library answers.

  * Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), the stream behind the Haar draws, the stretch move and the nested
    sampler: the oracle's C restatement and the numpy one of test_gpu_nested_exact.py against the known-answer vectors
    Random123 publishes (kat_vectors, philox4x32_10);
  * the bin index of k_flavor_hist (gf_kernels.hip), restated in numpy, against np.histogramdd's bins (plot.py:365-370) at
    every edge of np.linspace(0, 1, nb + 1), its neighbouring doubles and the values outside [0, 1], for nb = 1 .. 1024."""
import numpy as np
import pytest

from test_gpu_nested_exact import philox

# (counter c0..c3, key k0 k1) -> output words
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answers(oracle, ctr, key, want):
    assert oracle.philox4x32_10(ctr, key) == want
    got = philox(*[np.uint64(x) for x in ctr + key])
    assert tuple(int(x) for x in got) == want


def kernel_bins(v, nb):
    """k_flavor_hist's bin of each value on one axis, -1 where the sample is dropped: (int)(v * nb) clamped to the last bin,
    then moved down if v < edge(b), up if v >= edge(b + 1), with edge(k) = k * (1.0 / nb) as np.linspace makes it."""
    v = np.asarray(v, dtype=np.float64)
    ok = (v >= 0.0) & (v <= 1.0)
    b = np.minimum((np.where(ok, v, 0.0) * nb).astype(np.int64), nb - 1)
    step = 1.0 / nb
    b = np.where(v < b * step, b - 1, b)
    b = np.where((b + 1 < nb) & (v >= (b + 1) * step), b + 1, b)
    return np.where(ok, b, -1)


def truncating_bins(v, nb):
    """The rule k_flavor_hist had before: (int)(v * nb) alone."""
    v = np.asarray(v, dtype=np.float64)
    ok = (v >= 0.0) & (v <= 1.0)
    b = np.minimum((np.where(ok, v, 0.0) * nb).astype(np.int64), nb - 1)
    return np.where(ok, b, -1)


def edge_values(nb):
    """Every edge of np.linspace(0, 1, nb + 1), k / nb, the doubles on both sides of each, and the values at and past [0, 1]."""
    e = np.linspace(0.0, 1.0, nb + 1)
    q = np.arange(nb + 1) / nb
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), q, np.nextafter(q, -np.inf),
                           np.nextafter(q, np.inf),
                           [0.0, -0.0, 1.0, np.nextafter(1.0, 2.0), -5e-324, np.nan, np.inf, -np.inf]])


def histogramdd_bins(v, nb):
    """np.histogramdd's bin of each value, -1 where it drops the sample.  Its bins are monotone in v, so the counts of the
    sorted in-range values give each value's bin: the first counts[0] are in bin 0, the next counts[1] in bin 1, ..."""
    v = np.asarray(v, dtype=np.float64)
    counts, _ = np.histogramdd(v[:, None], bins=(nb,), range=((0, 1),))
    inside = (v >= 0.0) & (v <= 1.0)
    assert counts.sum() == inside.sum()
    order = np.argsort(v, kind="stable")
    out = np.full(v.shape, -1, dtype=np.int64)
    out[order[inside[order]]] = np.repeat(np.arange(nb), counts.astype(np.int64))
    return out


def test_histogram_bin_rule_matches_histogramdd():
    rng = np.random.default_rng(5)
    for nb in range(1, 1025):
        v = np.concatenate([edge_values(nb), rng.uniform(-0.01, 1.01, 64)])
        got, want = kernel_bins(v, nb), histogramdd_bins(v, nb)
        assert np.array_equal(got, want), (nb, v[got != want], got[got != want], want[got != want])


def test_truncating_bin_rule_disagrees_with_histogramdd():
    """Why the kernel moves its first guess: at nb = 5 the component 0.6 is 3.0 bins up, but np.linspace's edge 3 is
    0.6000000000000001, so numpy bins it in 2."""
    assert np.linspace(0, 1, 6)[3] == 0.6000000000000001
    assert truncating_bins([0.6], 5)[0] == 3 and kernel_bins([0.6], 5)[0] == 2
    counts, _ = np.histogramdd(np.array([[0.6]]), bins=(5,), range=((0, 1),))
    assert counts[2] == 1
    wrong = sum(not np.array_equal(truncating_bins(v, nb), kernel_bins(v, nb))
                for nb in range(1, 1025) for v in [edge_values(nb)])
    assert wrong > 900
