"""Pair lists and expected values for the tests of fsmc_decode_pair_minima (per site: the smallest posterior mean / MAP
over the pairs and the FIRST pair that has it, DecodePairsReturnStruct.hpp:105-118).

The main list: 192 pairs of conftest's small problem (64 haplotypes x 640 sites, K = 69), three full groups.  It is the
150 pairs P = enumerate_all_pairs(32)[100:250] with entries 48 and 140 swapped, followed by copies of entries 23, 64, 48
and 0 ... 38 of P.  A copy decodes to a bit-equal row, so every site's minimum is attained at two list positions at
least, many of them in different groups: an implementation that keeps the last winner, or loses the carried state at a
slice or range boundary, differs at hundreds of sites.  tests/test_pair_minima_lists.py proves on the CPU oracle that
the list reaches these regimes.

Expected values come from the oracle alone: O.decode_batch per batch of 64 pairs, O.per_pair_output, and numpy's
argmin (the first of equal minima) -- never from the code under test."""
import numpy as np

from oracle import oracle as O

BASE_PAIRS = O.enumerate_all_pairs(32)[100:250]
ORDER = list(range(150))
ORDER[48], ORDER[140] = ORDER[140], ORDER[48]
ORDER += [23, 64, 48] + list(range(39))  # positions in BASE_PAIRS of the list's 192 entries
PAIRS_192 = [BASE_PAIRS[i] for i in ORDER]
assert len(PAIRS_192) == 192


def oracle_rows(pm, folded, pairs):
    """(mean [n][S] float32, MAP [n][S] int32) of `pairs`, decoded batch by batch of 64 as the work list's groups are."""
    means, maps = [], []
    for b0 in range(0, len(pairs), 64):
        chunk = pairs[b0:b0 + 64]
        ob = np.stack([folded[a] ^ folded[b] for a, b in chunk])
        hb = np.stack([folded[a] & folded[b] for a, b in chunk])
        post, _ = O.decode_batch(pm, ob, hb, 0, pm.S)
        mean, mp, _ = O.per_pair_output(pm, post, len(chunk))
        means.append(mean)
        maps.append(mp)
    return np.concatenate(means), np.concatenate(maps)


def first_minima(rows, base=0):
    """(min [S], argmin [S] int32) of rows [n][S]: the column-wise minimum and the first row that attains it, counted
    from `base`.  (For rows without NaN this is the reference's loop: pair 0 seeds, a later pair wins only if `<`.)"""
    assert not np.isnan(rows).any()
    arg = rows.argmin(axis=0)
    return rows[arg, np.arange(rows.shape[1])], (arg + base).astype(np.int32)


def continue_minima(state_min, state_arg, rows, base):
    """The chain continued over `rows` from a carried (min, argmin): a new value wins only if strictly smaller."""
    m, a = first_minima(rows, base)
    take = m < state_min
    return np.where(take, m, state_min).astype(rows.dtype), np.where(take, a, state_arg).astype(np.int32)


_cache = {}


def rows_192(small_problem):
    """The oracle's rows of PAIRS_192, computed once a process and handed out read-only."""
    if "192" not in _cache:
        mean, mp = oracle_rows(small_problem["model"], small_problem["folded"], PAIRS_192)
        mean.setflags(write=False)
        mp.setflags(write=False)
        _cache["192"] = (mean, mp)
    return _cache["192"]
