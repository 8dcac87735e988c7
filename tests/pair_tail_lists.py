"""The numpy statement of fsmc_decode_pair_tail_summaries (the tail probabilities of fsmc_decode_pair_cdf reduced over the
pairs per site and over bins of sites per pair) for its tests.  Nothing here calls the code under test.

tail [n_tail][n][S] float32 is the tail stack of tests/pair_cdf_lists.py (`reduce` / `expected_192`: the fp32 running sum
of the oracle's posterior over the first `cut` states).  Three reductions, every addition written out as a loop step
(np.sum / np.cumsum / np.mean are not used: their order is numpy's business; numpy's float64 `+`, `*`, `/` on arrays and
its float32 <-> float64 conversions are IEEE round-to-nearest operations, one an element):
  tail_sum[j][t]: acc = acc + float64(tail[j][i][t]) for i = 0, 1, ... in list order, starting from the accumulator that
    is passed in (zeros to start): one fp64 add a pair.
  bin_tail_mean[j][i][b]: bin b = sites [e[b], e[b+1]), m of them.  Slot s (0 <= s < 64) starts at +0.0 (fp64) and adds
    float64(tail[j][i][t]) for t = e[b] + s, + 64, ... below e[b+1] in ascending order; then for stride = 32, 16, 8, 4, 2, 1:
    a[s] = a[s] + a[s + stride] for s < stride; float32(a[0] / float64(m)).  (The order of tests/pair_bins_lists.bin_mean.)
  bin_tail_length[j][i][b]: the same slots and tree over float64(tail[j][i][t]) * float64(w[t]) -- the product of two
    float32 values is exact in float64 --; float32(a[0]), no divide.

The standard inputs: PAIRS_192 of conftest's small problem (64 haplotypes x 640 sites, K = 69, three full groups), the cuts
of pair_cdf_lists.cuts, the edges EDGES and the weights `widths(gen)` of the problem's genetic map.
  EDGES = [5, 70, 71, 100, 400, 639]: a bin of 65 sites from an unaligned start, a bin of one site, a bin of 29 sites (narrower
  than the 64 slots), a bin of 300 sites (several strides of 64, the last one short), a bin of 239; sites 0-4 and 639 in no bin.
tests/test_pair_tail_lists.py proves on the CPU what these reach on the oracle's posteriors."""
import numpy as np

import pair_cdf_lists as CL
from pair_cdf_lists import PAIRS_192  # noqa: F401  (re-exported for the tests)

EDGES = np.array([5, 70, 71, 100, 400, 639], np.int32)


def widths(gen):
    """float32 [S]: the centimorgans site t stands for, 50 * (gen[min(t+1, S-1)] - gen[max(t-1, 0)]) with gen in Morgans,
    in float64, rounded once (what api.site_widths documents), one site at a time."""
    gen = np.asarray(gen, np.float64).reshape(-1)
    S = gen.size
    out = np.empty(S, np.float32)
    for t in range(S):
        out[t] = np.float32(np.float64(50.0) * (gen[min(t + 1, S - 1)] - gen[max(t - 1, 0)]))
    return out


def tail_sum(tail, acc=None):
    """[n_tail][S] float64: the pair-order fp64 chain over tail [n_tail][n][S], continuing `acc` (zeros if None)."""
    tail = np.asarray(tail)
    assert tail.dtype == np.float32 and tail.ndim == 3
    acc = np.zeros((tail.shape[0], tail.shape[2]), np.float64) if acc is None else np.array(acc, np.float64)
    assert acc.shape == (tail.shape[0], tail.shape[2])
    for i in range(tail.shape[1]):  # list order: one fp64 add a pair
        acc = acc + tail[:, i, :].astype(np.float64)
    return acc


def tail_sum_in_parts(tail, bounds, acc=None):
    """The same chain cut at the pair indices `bounds` (slices of a call, calls over parts of a list): every part
    continues the accumulator of the one before."""
    lo = 0
    for hi in list(bounds) + [np.asarray(tail).shape[1]]:
        acc = tail_sum(np.asarray(tail)[:, lo:hi], acc)
        lo = hi
    return acc


def _slots_and_tree(x, lo, hi):
    """a[0] of the defined order over x[..., lo:hi] (float64 values): [...] float64."""
    a = np.zeros(x.shape[:-1] + (64,), np.float64)
    for r0 in range(lo, hi, 64):  # (ascending: one stride of 64 sites at a time, slot s takes site r0 + s)
        w = min(64, hi - r0)
        a[..., :w] = a[..., :w] + x[..., r0:r0 + w]
    stride = 32
    while stride >= 1:
        a[..., :stride] = a[..., :stride] + a[..., stride:2 * stride]
        stride //= 2
    return a[..., 0]


def bin_tail_mean(tail, edges):
    """[n_tail][n][B] float32."""
    tail = np.asarray(tail)
    assert tail.dtype == np.float32 and tail.ndim == 3
    x = tail.astype(np.float64)
    out = np.empty(tail.shape[:2] + (len(edges) - 1,), np.float32)
    for b in range(len(edges) - 1):
        lo, hi = int(edges[b]), int(edges[b + 1])
        out[:, :, b] = (_slots_and_tree(x, lo, hi) / np.float64(hi - lo)).astype(np.float32)
    return out


def bin_tail_length(tail, edges, weights):
    """[n_tail][n][B] float32."""
    tail = np.asarray(tail)
    weights = np.asarray(weights)
    assert tail.dtype == np.float32 and tail.ndim == 3
    assert weights.dtype == np.float32 and weights.shape == (tail.shape[2],)
    x = tail.astype(np.float64) * weights.astype(np.float64)[None, None, :]  # (exact products)
    out = np.empty(tail.shape[:2] + (len(edges) - 1,), np.float32)
    for b in range(len(edges) - 1):
        out[:, :, b] = _slots_and_tree(x, int(edges[b]), int(edges[b + 1])).astype(np.float32)
    return out


def expected(tail, edges=None, weights=None, acc=None):
    """(tail_sum, bin_tail_mean or None, bin_tail_length or None) of a tail stack."""
    return (tail_sum(tail, acc), None if edges is None else bin_tail_mean(tail, edges),
            None if edges is None or weights is None else bin_tail_length(tail, edges, weights))


_cache = {}


def tails_192(small_problem, cut_list=None):
    """The tail stack of PAIRS_192 for the given cuts (pair_cdf_lists.cuts by default): [n_tail][192][640] float32,
    read-only."""
    return CL.expected_192(small_problem, cut_list, [])[0]


def expected_192(small_problem, cut_list=None):
    """expected() of tails_192 with EDGES and the widths of the problem's map, computed once a process for each set of
    cuts and handed out read-only."""
    key = None if cut_list is None else tuple(int(c) for c in cut_list)
    if key not in _cache:
        want = expected(tails_192(small_problem, cut_list), EDGES, widths(small_problem["gen"]))
        for w in want:
            w.setflags(write=False)
        _cache[key] = want
    return _cache[key]
