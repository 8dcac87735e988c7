"""The pair list of tests/pair_minima_lists.py reaches the regimes the GPU tests of fsmc_decode_pair_minima rely on --
shown on the CPU oracle (O.decode_batch, O.per_pair_output), not on the code under test.  The properties themselves are
asserted, not their counts on today's `synth`: every group holds the first argmin of the mean somewhere, at least two
groups that of the MAP, every site's minimum is tied between list positions, and ties cross group boundaries for both
outputs.  (Counts when this was written: first argmin of the mean in groups 0 / 1 / 2 at 10 / 206 / 424 sites, of the
MAP at 0 / 138 / 502; all 640 sites tied for both; 216 mean ties and 138 MAP ties across groups; smallest mean 36.2.)"""
import numpy as np

import pair_minima_lists as L


def _first_last(rows):
    first = rows.argmin(axis=0)
    last = rows.shape[0] - 1 - rows[::-1].argmin(axis=0)
    return first, last


def test_the_list_is_three_full_groups_with_copies():
    assert len(L.PAIRS_192) == 192 and len(set(L.PAIRS_192)) == 150
    assert L.PAIRS_192[48] == L.BASE_PAIRS[140] and L.PAIRS_192[140] == L.BASE_PAIRS[48]
    assert L.PAIRS_192[150:153] == [L.BASE_PAIRS[23], L.BASE_PAIRS[64], L.BASE_PAIRS[48]]


def test_copies_decode_to_bit_equal_rows(small_problem):
    mean, mp = L.rows_192(small_problem)
    assert mean.shape == mp.shape == (192, small_problem["model"].S)
    assert mean.dtype == np.float32 and mp.dtype == np.int32
    for pos in range(150, 192):
        src = L.PAIRS_192.index(L.PAIRS_192[pos])
        assert src < 150
        assert np.array_equal(mean[pos].view(np.uint32), mean[src].view(np.uint32)), pos
        assert np.array_equal(mp[pos], mp[src]), pos


def test_no_nan_no_inf(small_problem):
    mean, _ = L.rows_192(small_problem)
    assert np.isfinite(mean).all()
    assert mean.min() > 0


def test_every_regime_is_reached(small_problem):
    mean, mp = L.rows_192(small_problem)
    S = mean.shape[1]
    for name, rows, groups_needed in (("mean", mean, 3), ("MAP", mp, 2)):
        first, last = _first_last(rows)
        winners = np.bincount(first // 64, minlength=3)
        tied = int((first != last).sum())
        cross = int((first // 64 != last // 64).sum())
        print(f"{name}: first argmin per group {winners.tolist()}, tied sites {tied} of {S}, across groups {cross}")
        assert (winners > 0).sum() >= groups_needed, name
        assert tied == S, name  # (every minimum is tied: the last winner is never the first)
        assert cross > 0, name
        # the reference's loop and numpy's argmin agree on these rows
        m, a = L.first_minima(rows)
        best, arg = rows[0].copy(), np.zeros(S, np.int32)
        for i in range(1, rows.shape[0]):
            take = rows[i] < best
            best[take] = rows[i][take]
            arg[take] = i
        assert np.array_equal(best, m) and np.array_equal(arg, a), name


def test_a_range_boundary_inside_a_group_separates_tied_positions(small_problem):
    """Ranges of 40 pairs (the GPU test's setting) cut the list at 40, 80, 120, 160: inside every group.  Ties must span
    such a boundary too."""
    mean, mp = L.rows_192(small_problem)
    for rows in (mean, mp):
        first, last = _first_last(rows)
        assert (first // 40 != last // 40).any()


def test_continue_minima_is_the_chain(small_problem):
    mean, mp = L.rows_192(small_problem)
    for rows in (mean, mp):
        m0, a0 = L.first_minima(rows[:100])
        m1, a1 = L.continue_minima(m0, a0, rows[100:], 100)
        m, a = L.first_minima(rows)
        assert np.array_equal(m1, m) and np.array_equal(a1, a)
