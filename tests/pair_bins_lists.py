"""Bin edges and the numpy statement of fsmc_decode_pair_bins (per pair: mean, min and argmin of the posterior-mean row
and min and argmin of the MAP row over bins of sites) for its tests.  Nothing here calls the code under test.

The rows are those of tests/pair_minima_lists.py: PAIRS_192 of conftest's small problem (64 haplotypes x 640 sites,
K = 69, three full groups) and the oracle's rows_192.  Four edge sets:
  E1 = [0, 640]               one bin of ten strides of 64
  E2 = 0, 16, ..., 640        40 narrow bins
  E3 = [5, 70, 71, 200, 639]  unaligned starts, a bin of 65 sites, a bin of one site, sites 0-4 and 639 in no bin
  E4 = 0, 1, ..., 640         every site its own bin: the outputs are the rows themselves and argmin == site
tests/test_pair_bins_lists.py proves on the CPU what these reach on the oracle's rows.

The expected values, for edges e and rows mean / map [n][S], bin b = sites [e[b], e[b+1]), m = e[b+1] - e[b]:
  bin_mean: slot j (0 <= j < 64) starts at +0.0 (fp64) and adds float64(mean[i][t]) for t = e[b] + j, + 64, ... below
    e[b+1] in ascending order; then for stride = 32, 16, 8, 4, 2, 1: a[j] = a[j] + a[j + stride] for j < stride;
    float32(a[0] / float64(m)).  numpy's float64 `+` and `/` and its float64 -> float32 conversion are IEEE
    round-to-nearest operations, one per step written here: no pairwise or fused summation enters.
  bin_min_* / bin_argmin_*: numpy's min of the slice and e[b] + numpy's argmin (the first of equal minima)."""
import numpy as np

from pair_minima_lists import PAIRS_192, oracle_rows, rows_192  # noqa: F401  (re-exported for the tests)

E1 = np.array([0, 640], np.int32)
E2 = np.arange(0, 641, 16, dtype=np.int32)
E3 = np.array([5, 70, 71, 200, 639], np.int32)
E4 = np.arange(0, 641, dtype=np.int32)
EDGE_SETS = {"E1": E1, "E2": E2, "E3": E3, "E4": E4}


def bin_mean(mean, edges):
    """[n][B] float32: the defined fp64 order, all pairs at once."""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32
    n = mean.shape[0]
    out = np.empty((n, len(edges) - 1), np.float32)
    for b in range(len(edges) - 1):
        lo, hi = int(edges[b]), int(edges[b + 1])
        a = np.zeros((n, 64), np.float64)
        for r0 in range(lo, hi, 64):  # (ascending: one stride of 64 sites at a time, slot j takes site r0 + j)
            w = min(64, hi - r0)
            a[:, :w] = a[:, :w] + mean[:, r0:r0 + w].astype(np.float64)
        stride = 32
        while stride >= 1:
            a[:, :stride] = a[:, :stride] + a[:, stride:2 * stride]
            stride //= 2
        out[:, b] = (a[:, 0] / np.float64(hi - lo)).astype(np.float32)
    return out


def bin_min(rows, edges):
    """([n][B] of rows' dtype, [n][B] int32): the smallest value of each bin and the LOWEST absolute site that has it."""
    rows = np.asarray(rows)
    if rows.dtype.kind == "f":
        assert not np.isnan(rows).any()
    n = rows.shape[0]
    mn = np.empty((n, len(edges) - 1), rows.dtype)
    arg = np.empty((n, len(edges) - 1), np.int32)
    for b in range(len(edges) - 1):
        lo, hi = int(edges[b]), int(edges[b + 1])
        a = rows[:, lo:hi].argmin(axis=1)
        mn[:, b] = rows[np.arange(n), lo + a]
        arg[:, b] = lo + a
    return mn, arg


def expected(mean, mp, edges):
    """(bin_mean, bin_min_mean, bin_argmin_mean, bin_min_map, bin_argmin_map) of the rows."""
    return (bin_mean(mean, edges),) + bin_min(mean, edges) + bin_min(mp, edges)


NAMES = ("bin_mean", "bin_min_mean", "bin_argmin_mean", "bin_min_map", "bin_argmin_map")
DTYPES = (np.float32, np.float32, np.int32, np.int32, np.int32)

_cache = {}


def expected_192(small_problem, name):
    """expected() of rows_192 for the edge set `name`, computed once a process and handed out read-only."""
    if name not in _cache:
        mean, mp = rows_192(small_problem)
        want = expected(mean, mp, EDGE_SETS[name])
        for w in want:
            w.setflags(write=False)
        _cache[name] = want
    return _cache[name]
