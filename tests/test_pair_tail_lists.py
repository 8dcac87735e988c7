"""What the inputs of tests/test_gpu_pair_tail.py reach, shown on the CPU: on the oracle's tail stack of PAIRS_192 a
kernel that sums in another precision or order, ignores the weights or carries its chain wrongly gives other bits than
the statement of tests/pair_tail_lists.py, and the standard edges hold every shape of bin the kernel treats apart."""
import numpy as np
import pytest

import pair_cdf_lists as CL
import pair_tail_lists as TL


@pytest.fixture(scope="module")
def tails(small_problem):
    return TL.tails_192(small_problem)


def test_the_fp64_chain_is_not_an_fp32_chain(small_problem, tails):
    """A kernel that keeps the sum over pairs in fp32 is caught at some site of every cut -- but perhaps not of c = K,
    whose tails are 1 give or take an ulp and whose sums may be exact either way."""
    cuts = CL.cuts(small_problem["model"])
    want = TL.tail_sum(tails)
    acc32 = np.zeros(want.shape, np.float32)
    for i in range(tails.shape[1]):
        acc32 = acc32 + tails[:, i, :]
    assert acc32.dtype == np.float32
    differs = (acc32.astype(np.float64) != want).any(axis=1)
    for j, c in enumerate(cuts):
        if c != small_problem["model"].K:
            assert differs[j], f"cut {c}: an fp32 chain gives the fp64 chain's bits at every site"
    # ... and the fp64 chain rounded to float32 at the end is not the fp32 chain either
    assert (acc32 != want.astype(np.float32)).any()


def test_the_bin_mean_order_is_not_an_fp32_accumulation(tails):
    want = TL.bin_tail_mean(tails, TL.EDGES)
    other = np.empty_like(want)
    for b in range(len(TL.EDGES) - 1):
        lo, hi = int(TL.EDGES[b]), int(TL.EDGES[b + 1])
        a = np.zeros(tails.shape[:2], np.float32)
        for t in range(lo, hi):
            a = a + tails[:, :, t]
        other[:, :, b] = a / np.float32(hi - lo)
    assert other.dtype == np.float32
    assert (other != want).any()
    # a bin of one site is that site's tail
    assert np.array_equal(want[:, :, 1], tails[:, :, 70])


def test_the_weights_show(small_problem, tails):
    """The weights are not constant, and the weighted length is not the mean times the bin's weight sum: a kernel that
    drops w[t] or takes one weight a bin is caught."""
    w = TL.widths(small_problem["gen"])
    assert w.dtype == np.float32 and w.shape == (640,) and np.isfinite(w).all()
    assert np.unique(w[5:639]).size > 100
    mean = TL.bin_tail_mean(tails, TL.EDGES)
    length = TL.bin_tail_length(tails, TL.EDGES, w)
    differs_somewhere = False
    for b in range(len(TL.EDGES) - 1):
        lo, hi = int(TL.EDGES[b]), int(TL.EDGES[b + 1])
        wsum = np.float64(0.0)
        for t in range(lo, hi):
            wsum = wsum + np.float64(w[t])
        flat = (mean[:, :, b].astype(np.float64) * wsum).astype(np.float32)
        if hi - lo > 1:
            differs_somewhere |= bool((flat != length[:, :, b]).any())
    assert differs_somewhere
    # the one-site bin: exactly float32(tail * w), the exact product rounded once
    assert np.array_equal(length[:, :, 1], (tails[:, :, 70].astype(np.float64) * np.float64(w[70])).astype(np.float32))
    # unit weights give the fp64 slot sum itself: mean * m up to the two roundings, and exactly the sum for one site
    ones = np.ones(640, np.float32)
    assert np.array_equal(TL.bin_tail_length(tails, TL.EDGES, ones)[:, :, 1], tails[:, :, 70])


def test_the_statement_does_not_depend_on_slicing(tails):
    """The chain cut into slices of groups, into calls over parts of the list, and at a ragged place: the same bits; and a
    non-zero incoming accumulator is part of the chain (it is not added at the end)."""
    want = TL.tail_sum(tails)
    for bounds in ([64, 128], [128], [64], [150], [1, 2, 3, 191]):
        assert np.array_equal(TL.tail_sum_in_parts(tails, bounds), want), bounds
    rng = np.random.default_rng(3)
    seed = rng.random(want.shape) * 1e3 + 0.1
    carried = TL.tail_sum(tails, seed)
    assert np.array_equal(TL.tail_sum_in_parts(tails, [64, 128], seed), carried)
    assert (carried != want + seed).any()  # (adding the seed afterwards is another order)


def test_the_standard_edges_hold_every_case():
    e = [int(x) for x in TL.EDGES]
    widths = [hi - lo for lo, hi in zip(e[:-1], e[1:])]
    assert all(w > 0 for w in widths) and e[0] >= 0 and e[-1] <= 640
    assert any(1 < w < 64 for w in widths)       # narrower than the 64 slots
    assert 1 in widths                           # a one-site bin
    assert any(x % 64 != 0 for x in e)           # an edge that is no multiple of 64
    assert any(w > 3 * 64 and w % 64 != 0 for w in widths)  # several strides of 64, the last one short
    assert e[0] > 0 and e[-1] < 640              # sites that belong to no bin, at both ends


def test_site_widths_is_the_statements_widths(small_problem):
    import __graft_entry__ as g

    g.build()
    from fastsmc_amd import api

    gen = small_problem["gen"]
    got = api.site_widths(gen)
    assert got.dtype == np.float32 and np.array_equal(got, TL.widths(gen))
    # three sites a centimorgan apart: the ends stand for half a gap, the middle for two halves
    assert api.site_widths([0.0, 0.01, 0.02]).tolist() == [0.5, 1.0, 0.5]
    assert api.site_widths([0.3]).tolist() == [0.0]
    with pytest.raises(ValueError):
        api.site_widths([])
    with pytest.raises(ValueError):
        api.site_widths([0.0, float("nan")])
