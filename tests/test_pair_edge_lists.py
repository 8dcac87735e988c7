"""What the cases of tests/pair_edge_lists.py reach, proven on the CPU oracle: the GPU tests of
tests/test_gpu_pair_edges.py compare bits with expected values, and these tests show that the expected values sit in the
regime each case is there for -- subnormal tails and means, a quantile met with equality, a plateau of the running sum,
ties between the sites of a bin and the pairs of a site, signed zeros -- and that a wrong rule would change them: `>` for
`>=`, the last state or site of a tie for the first, subnormals flushed to zero, -0.0 taken for +0.0.  Every figure is
printed beside its bound (pytest -s shows them); a bound is a condition on the inputs, about half of what was measured
when the case was written, so a later change to a generator cannot quietly turn the GPU file into a benign one.

No test here calls the library."""
import numpy as np
import pytest

import pair_bins_lists as BL
import pair_edge_lists as PL
import pair_minima_lists as ML
import pair_tail_lists as TL


def _at_least(what, measured, bound):
    """Print the figure beside its bound and hold it; a bound of 0 records a figure the case is not there for."""
    print(f"{what}: {measured} (at least {bound})")
    assert measured >= bound, (what, measured, bound)


def _tail(case, cut):
    return PL.expected_cdf(case)[0][PL.cuts(case).index(cut)]


def _qstate(case, name):
    return PL.expected_cdf(case)[1][list(PL.quantile_set(case)).index(name)]


def _first_state(cdf, q, strict=False):
    """An explicit loop, independent of CL.reduce: the first k with cdf[k] >= q (`>` if strict), K-1 if none."""
    K = cdf.shape[0]
    out = np.full(cdf.shape[1:], K - 1, np.int32)
    for k in range(K - 1, -1, -1):  # (descending: the lowest k that passes is written last)
        hit = cdf[k] > q if strict else cdf[k] >= q
        out[hit] = k
    return out


def _last_equal_state(cdf, q):
    """The last k with cdf[k] == q, -1 where there is none."""
    out = np.full(cdf.shape[1:], -1, np.int32)
    for k in range(cdf.shape[0]):
        out[cdf[k] == q] = k
    return out


def _flushed(a):
    return np.where(PL.is_subnormal(a), a.dtype.type(0), a)


# ---------------------------------------------------------------- subnormal posteriors

# (subnormal tails at cut 1, at cut 8, cells where the subnormal quantile finds a state other than 0, distinct states it
# finds): the bounds, about half of what was measured
SUBNORMAL_30 = {
    ("subnormal-1e-30", 69, False): (15000, 3000, 10000, 5),  # measured: 37 145, 6 370, 29 673, 9
    # 33 states: the eight scaled states are a quarter of the model, and the running sum is normal from the second on
    ("subnormal-1e-30", 33, False): (1600, 0, 700, 2),        # measured: 3 338, 0, 1 408, 4
    ("subnormal-1e-30", 200, False): (11000, 450, 8000, 5),   # measured: 23 309, 949, 17 037, 9
    ("subnormal-1e-30", 69, True): (14000, 2300, 13000, 5),   # measured: 28 650, 4 750, 27 727, 9
}


@pytest.mark.parametrize("case", list(SUBNORMAL_30), ids=PL.case_id)
def test_subnormal_tails_and_a_subnormal_quantile(case):
    cut1, cut8, moved, distinct = SUBNORMAL_30[case]
    _at_least("subnormal tails at cut 1", int(PL.is_subnormal(_tail(case, 1)).sum()), cut1)
    _at_least("subnormal tails at cut 8", int(PL.is_subnormal(_tail(case, 8)).sum()), cut8)
    q = PL.quantile_set(case)["sub"]
    assert PL.is_subnormal(q)
    states = _qstate(case, "sub")
    assert np.array_equal(states, _first_state(PL.running_sums(case), q))
    # a compare, add or select that flushes subnormals finds q at state 0 (0 >= 0), or nowhere
    _at_least("cells where the subnormal quantile finds a state other than 0", int((states != 0).sum()), moved)
    _at_least("distinct states the subnormal quantile finds", int(np.unique(states).size), distinct)


def test_subnormal_tails_count_in_the_sums():
    """K = 69: the fp64 sum over the pairs, the bin means and the bin lengths all change when the subnormal tails (or
    weights) are taken for 0, and bin means and lengths are themselves subnormal: a conversion to fp64 that flushes its
    input, or a conversion back that flushes its result, shows."""
    case = ("subnormal-1e-30", 69, False)
    tail = PL.expected_cdf(case)[0]
    S = tail.shape[2]
    want_sum = TL.tail_sum(tail)
    _at_least("tail_sum cells that differ when subnormal tails are flushed",
              int((TL.tail_sum(_flushed(tail)) != want_sum).sum()), 100)
    _at_least("sites whose fp64 tail sum at cut 1 is below the fp32 normal range",
              int(((want_sum[0] > 0) & (want_sum[0] < PL.TINY)).sum()), 48)
    for name, edges in PL.edge_sets(S).items():
        _, mean, length = PL.expected_tail(case, name)
        sub_mean = PL.is_subnormal(mean)
        print(f"{name}: {int(sub_mean.sum())} of {mean.size} subnormal bin_tail_mean cells, "
              f"{int(PL.is_subnormal(length).sum())} of {length.size} subnormal bin_tail_length cells, "
              f"{int((length >= PL.TINY).sum())} normal ones")
        if name == "sixteen":
            _at_least("subnormal, non-zero bin_tail_mean cells", int(sub_mean.sum()), 100)
        _at_least("subnormal, non-zero bin_tail_length cells", int(PL.is_subnormal(length).sum()), 96)
        _at_least("normal bin_tail_length cells", int((length >= PL.TINY).sum()), 96)
        w = PL.site_weights(S)
        _at_least("bin_tail_length cells that differ when subnormal weights are flushed",
                  int((TL.bin_tail_length(tail, edges, _flushed(w)) != length).sum()), 96)
        _at_least("bin_tail_mean cells that differ when subnormal tails are flushed",
                  int((TL.bin_tail_mean(_flushed(tail), edges) != mean).sum()), 100 if name == "sixteen" else 1)
        # the rounding of (float)(a / n) falls into the subnormal range: the fp64 quotient is no float32
        lo, hi = int(edges[1]), int(edges[2])
        exact = TL._slots_and_tree(tail.astype(np.float64), lo, hi) / np.float64(hi - lo)
        inexact = sub_mean[:, :, 1] & (mean[:, :, 1].astype(np.float64) != exact)
        _at_least(f"{name}: subnormal means of bin 1 that the conversion to float32 rounds", int(inexact.sum()), 1)


@pytest.mark.parametrize("K", [69, 33])
def test_exact_zeros_in_front_and_the_smallest_quantile(K):
    """subnormal-1e-38: q = 2^-149 finds the first state whose running sum is not 0 -- `cdf >= q` with a flushed q
    (0 >= 0) would return state 0 everywhere.  At 69 states the first state is exactly 0 at every cell, so the answer is
    state 0 nowhere; at 33 states it is exactly 0 at more than half of the cells."""
    case = ("subnormal-1e-38", K, False)
    cdf = PL.running_sums(case)
    first = np.full(cdf.shape[1:], -1, np.int32)
    for k in range(K - 1, -1, -1):
        first[cdf[k] != 0] = k
    assert (first >= 0).all()
    assert np.array_equal(_qstate(case, "ulp"), first)
    if K == 69:
        assert (PL.bits(_tail(case, 1)) == 0).all() and (first > 0).all()
    # (measured at 33 states: 21 696 of 38 400)
    _at_least("cells whose first state is exactly 0", int((first > 0).sum()), first.size if K == 69 else 10000)
    print(f"K = {K}: the first state with a non-zero running sum takes {np.unique(first).size} values, "
          f"{int(first.min())} ... {int(first.max())}")
    plateau = (cdf[1:] == cdf[:-1]).any(axis=0)
    _at_least("cells with a plateau of the running sum", int(plateau.sum()), 19000)  # (measured: all 38 400)


# ---------------------------------------------------------------- equality and plateaus

# cells where the running sum equals the quantile "eq": the bounds, about half of what was measured
EQUALITY = {
    ("degenerate", 69, False): 5000,                    # measured: 14 505
    ("degenerate", 33, False): 7000,                    # measured: 14 481
    ("degenerate_with_dead_states", 69, False): 5000,   # measured: 16 386
    ("degenerate_with_dead_states", 33, False): 7000,   # measured: 14 802
    ("degenerate_with_dead_states", 200, False): 5500,  # measured: 11 590
}


@pytest.mark.parametrize("case", list(EQUALITY), ids=PL.case_id)
def test_the_quantile_is_met_with_equality(case):
    """At thousands of cells cdf[k] == q at the state the statement returns: `>` for `>=` moves every one of them.  The
    float32 above q moves every such cell by exactly one state and the float32 below q moves none of them (the state
    before the hit is a whole posterior lower): together they fix the compare to `>=` at q itself.  With dead states the
    running sum stays on q for a state at every such cell: the last state that equals q is not the first."""
    cdf = PL.running_sums(case)
    q = PL.quantile_set(case)["eq"]
    k = _qstate(case, "eq")
    assert np.array_equal(k, _first_state(cdf, q))
    at = np.take_along_axis(cdf, k[None].astype(np.int64), axis=0)[0] == q
    _at_least("cells where the running sum equals q at the returned state", int(at.sum()), EQUALITY[case])
    strict = _first_state(cdf, q, strict=True)
    assert (strict[at] != k[at]).all()
    assert (_qstate(case, "eq+")[at] == strict[at]).all()  # (the next float: what `>` at q returns)
    assert (_qstate(case, "eq-")[at] == k[at]).all()
    last = _last_equal_state(cdf, q)
    if case[0] == "degenerate_with_dead_states":
        assert (last[at] > k[at]).all()
        assert (strict[at] >= k[at] + 2).all()
        # ghost states of a padded member and the dead last states: q = 1.0 and the cut K stop at the model's states
        print(f"q = 1.0 finds states {np.unique(_qstate(case, 'one')).tolist()} of {case[1]}")
    else:
        assert (last[at] == k[at]).all() and (strict[at] == k[at] + 1).all()


def test_zero_states_plateaus_and_equal_tails():
    for K in (69, 33):
        case = ("zero-states", K, False)
        cdf = PL.running_sums(case)
        assert (cdf[1:] == cdf[:-1]).any(axis=0).all(), "every cell has a plateau"
        d = PL.dead_state(K)
        below, above, before = _tail(case, d), _tail(case, d + 1), _tail(case, d - 1)
        assert np.array_equal(PL.bits(below), PL.bits(above))
        differ = int((PL.bits(before) != PL.bits(below)).sum())
        _at_least(f"K = {K}: cells where the cut before the dead state differs from the cut below it", differ,
                  before.size // 2)


# ---------------------------------------------------------------- expected times in the subnormal range

def test_times_scaled_into_the_subnormal_range():
    case = ("benign", 69, False)
    own, _ = PL.rows(case, "own")
    mean, _ = PL.rows(case, "2^-140")
    _at_least("subnormal means", int(PL.is_subnormal(mean).sum()), 8000)
    scaled = (own.astype(np.float64) * 2.0 ** -140).astype(np.float32)
    _at_least("means that differ from the benign mean scaled", int((mean != scaled).sum()), 8000)
    bin_mean = PL.expected_bins(case, "2^-140", "wide")[0]
    _at_least("subnormal bin means", int(PL.is_subnormal(bin_mean).sum()), 40)
    for c in PL.POSTERIOR_CASES:
        rows, total = PL.expected_posteriors(c, "2^-140")
        print(f"{PL.case_id(c)}: {int(PL.is_subnormal(rows).sum())} subnormal products, "
              f"{int(PL.is_subnormal(total).sum())} of {total.size} subnormal sums over the pairs")
        _at_least("subnormal post * time products", int(PL.is_subnormal(rows).sum()), 20000)
        _at_least("subnormal sums over the pairs", int(PL.is_subnormal(total).sum()), 4000 if c[1] == 69 else 0)


@pytest.mark.parametrize("case", PL.BINS_CASES, ids=PL.case_id)
def test_ties_en_masse(case):
    """The float tie rules: `v < best` keeps the FIRST pair of a site (minima), `v == best && t < arg` the LOWEST site
    of a bin (bins).  With the few-ulp times every case ties at most sites and bins; the degenerate model does with its
    own times as well."""
    S = PL.model(*case)[0].S
    edges = PL.edge_sets(S)["sixteen"]
    for variant in ("few-ulp", "own") if case[0] == "degenerate" else ("few-ulp",):
        mean, mp = PL.rows(case, variant)
        values = np.unique(mean)
        scale = f" (times * 2^{PL.few_ulp_exponent(case)})" if variant == "few-ulp" else ""
        print(f"{variant}{scale}: {values.size} distinct means, the largest {float(values[-1]) / 2.0 ** -149:.3g} ulps")
        if variant == "few-ulp":
            assert values[-1] <= 16 * PL.ULP
            assert values.size >= (1 if case[0] == "degenerate" else 3)  # (degenerate: one value at every pair and site)
        tied_sites = int(((mean == mean.min(axis=0)).sum(axis=0) > 1).sum())
        first = ML.first_minima(mean)[1]
        last = mean.shape[0] - 1 - mean[::-1].argmin(axis=0)
        assert int((first != last).sum()) == tied_sites
        _at_least(f"{variant}: sites whose minimum mean is tied between pairs", tied_sites, S // 2)
        mn, arg = BL.bin_min(mean, edges)
        tied = last_differs = 0
        for b in range(len(edges) - 1):
            lo, hi = int(edges[b]), int(edges[b + 1])
            hit = mean[:, lo:hi] == mn[:, b:b + 1]
            tied += int((hit.sum(axis=1) > 1).sum())
            last_differs += int((lo + (hi - lo - 1) - hit[:, ::-1].argmax(axis=1) != arg[:, b]).sum())
        bound = 400 if (case, variant) == (("degenerate", 69, False), "own") else mn.size // 4
        _at_least(f"{variant}: sixteen-site bins (of {mn.size}) with a tied minimum mean", tied, bound)
        _at_least(f"{variant}: bins whose last tied site is not the expected argmin", last_differs, bound)
        if case[0] == "degenerate":  # the int rule: the MAP is 0 everywhere, so every argmin is the bin's first site
            assert (mp == 0).all()
            assert np.array_equal(BL.bin_min(mp, edges)[1], np.broadcast_to(edges[:-1], mn.shape))


def test_zero_times_and_signed_zeros():
    """+0.0 and -0.0 times: every mean is +0.0 (the mean starts at +0.0 and adds products of either sign of zero), every
    table value of the -0.0 times is -0.0, and the sum over the pairs keeps the sign of its accumulator: +0.0 + -0.0 is
    +0.0, -0.0 + -0.0 is -0.0.  np.array_equal sees none of it."""
    for case in PL.MINIMA_CASES:
        for variant in ("+0", "-0"):
            mean, _ = PL.rows(case, variant)
            assert (PL.bits(mean) == 0).all(), (case, variant)
            assert (ML.first_minima(mean)[1] == 0).all()  # every site reports the first pair
    for case in PL.POSTERIOR_CASES[:2]:
        K, S = case[1], PL.model(*case)[0].S
        rows, from_plus = PL.expected_posteriors(case, "-0")
        assert (PL.bits(rows) == 0x80000000).all()
        assert (PL.bits(from_plus) == 0).all()
        _, from_minus = PL.expected_posteriors(case, "-0", acc=np.full((K, S), -0.0, np.float32))
        assert (PL.bits(from_minus) == 0x80000000).all()
        assert np.array_equal(from_plus, from_minus)  # (what the bit patterns are for)
        with pytest.raises(AssertionError):
            PL.assert_same_bits(from_plus, from_minus)
        rows, total = PL.expected_posteriors(case, "+0", acc=np.full((K, S), -0.0, np.float32))
        assert (PL.bits(rows) == 0).all() and (PL.bits(total) == 0).all()


def test_bit_pattern_helper():
    a = np.array([0.0, 1.0, 1e-45], np.float32)
    PL.assert_same_bits(a, a.copy())
    PL.assert_same_bits(a.astype(np.float64), a.astype(np.float64))
    PL.assert_same_bits(np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32))
    for other in (np.array([-0.0, 1.0, 1e-45], np.float32), np.array([0.0, 1.0, 0.0], np.float32), a.astype(np.float64),
                  a[:2]):
        with pytest.raises(AssertionError):
            PL.assert_same_bits(other, a)
    with pytest.raises(AssertionError):
        PL.assert_same_bits(np.array([0.0, -0.0]), np.array([0.0, 0.0]))
    with pytest.raises(AssertionError):
        PL.assert_same_bits(np.arange(3, dtype=np.int32), np.array([0, 1, 3], np.int32))
