"""The edge sets of tests/pair_bins_lists.py reach, on the oracle's rows of PAIRS_192, the regimes the GPU tests of
fsmc_decode_pair_bins rely on -- shown on the CPU (O.decode_batch, O.per_pair_output), not on the code under test.

Counts when this was written (asserted below as lower bounds of 100 where a count is given):
  bins whose MAP minimum is tied between sites                    E1 191 of 192, E3 558 of 768, E2 7010 of 7680
  bins whose first MAP minimum lies beyond the bin's first 64 sites      E1 150, E3 140
  bins where a tied later site sits in a LOWER slot ((t - e[b]) % 64) than the first: a combine in lane order alone
    picks the wrong site                                                 E1 133, E3 162
  bins whose mean minimum lies beyond the first 64 sites                 E1 178, E3 253
The mean rows hold no tie between sites of a bin at all, which is why the tie rule is exercised on the MAP rows.  The
defined fp64 order differs from numpy's float32 mean in 84 of 320 (pair, range) samples (the first 64 pairs over the bin
of E1 and the four of E3) and equals the float64 mean rounded once in all 320."""
import numpy as np

import pair_bins_lists as BL


def _slices(edges):
    return [(int(edges[b]), int(edges[b + 1])) for b in range(len(edges) - 1)]


def _tie_counts(rows, edges):
    """(bins, tied, first beyond 64 sites, a tied later site in a lower slot) over all pairs and bins."""
    bins = tied = beyond = lower_slot = 0
    for lo, hi in _slices(edges):
        part = rows[:, lo:hi]
        first = part.argmin(axis=1)
        is_min = part == part.min(axis=1, keepdims=True)
        slot = np.arange(hi - lo) % 64
        for i in range(rows.shape[0]):
            where = np.nonzero(is_min[i])[0]
            assert where[0] == first[i]
            bins += 1
            tied += where.size > 1
            beyond += first[i] >= 64
            lower_slot += bool((slot[where[1:]] < slot[first[i]]).any())
    return bins, int(tied), int(beyond), int(lower_slot)


def test_edge_sets_are_what_the_docstring_says():
    assert BL.E1.tolist() == [0, 640] and BL.E3.tolist() == [5, 70, 71, 200, 639]
    assert BL.E2.tolist() == list(range(0, 641, 16)) and BL.E4.tolist() == list(range(641))
    for e in BL.EDGE_SETS.values():
        assert e.dtype == np.int32 and (np.diff(e) > 0).all() and e[0] >= 0 and e[-1] <= 640
    assert np.diff(BL.E3).tolist() == [65, 1, 129, 439]


def test_rows_hold_no_nan(small_problem):
    mean, mp = BL.rows_192(small_problem)
    assert mean.shape == mp.shape == (192, 640)
    assert not np.isnan(mean).any() and np.isfinite(mean).all()


def test_map_ties_reach_every_regime(small_problem):
    _, mp = BL.rows_192(small_problem)
    for name, floor_beyond in (("E1", 100), ("E3", 100), ("E2", None)):
        bins, tied, beyond, lower_slot = _tie_counts(mp, BL.EDGE_SETS[name])
        print(f"MAP {name}: {tied} of {bins} bins tied, first minimum beyond 64 sites in {beyond}, a tied later site in "
              f"a lower slot in {lower_slot}")
        assert tied >= 100, name
        if floor_beyond:
            assert beyond >= floor_beyond, name
            assert lower_slot >= 100, name


def test_mean_minima_lie_beyond_the_first_stride_and_are_never_tied(small_problem):
    mean, _ = BL.rows_192(small_problem)
    for name in ("E1", "E3"):
        bins, tied, beyond, _ = _tie_counts(mean, BL.EDGE_SETS[name])
        print(f"mean {name}: minimum beyond the first 64 sites in {beyond} of {bins} bins, {tied} tied")
        assert beyond >= 100, name
        assert tied == 0, name


def test_the_defined_order_is_not_numpys_float32_mean(small_problem):
    mean, _ = BL.rows_192(small_problem)
    rows = mean[:64]
    differs = equal64 = samples = 0
    for edges in (BL.E1, BL.E3):
        got = BL.bin_mean(rows, edges)
        for b, (lo, hi) in enumerate(_slices(edges)):
            samples += rows.shape[0]
            differs += int((got[:, b] != rows[:, lo:hi].mean(axis=1, dtype=np.float32)).sum())
            equal64 += int((got[:, b] == rows[:, lo:hi].mean(axis=1, dtype=np.float64).astype(np.float32)).sum())
    print(f"defined order against numpy: {differs} of {samples} differ from the float32 mean, {equal64} equal the float64 "
          "mean rounded once")
    assert samples == 320
    assert differs > 0


def test_bin_mean_is_the_slot_order_written_out(small_problem):
    """bin_mean() vectorises over pairs; here the definition is followed literally, scalar by scalar, for a few cells."""
    mean, _ = BL.rows_192(small_problem)
    for edges in (BL.E1, BL.E3):
        got = BL.bin_mean(mean[:3], edges)
        for i in range(3):
            for b, (lo, hi) in enumerate(_slices(edges)):
                a = [np.float64(0.0)] * 64
                for j in range(64):
                    for t in range(lo + j, hi, 64):
                        a[j] = a[j] + np.float64(mean[i, t])
                for stride in (32, 16, 8, 4, 2, 1):
                    for j in range(stride):
                        a[j] = a[j] + a[j + stride]
                assert got[i, b] == np.float32(a[0] / np.float64(hi - lo)), (i, b)


def test_single_site_bins_are_the_rows(small_problem):
    mean, mp = BL.rows_192(small_problem)
    want = BL.expected_192(small_problem, "E4")
    sites = np.broadcast_to(np.arange(640, dtype=np.int32), mean.shape)
    assert np.array_equal(want[0], mean) and np.array_equal(want[1], mean) and np.array_equal(want[3], mp)
    assert np.array_equal(want[2], sites) and np.array_equal(want[4], sites)
