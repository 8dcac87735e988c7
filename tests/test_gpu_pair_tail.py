"""fsmc_decode_pair_tail_summaries on the GPU: the tail probabilities of fsmc_decode_pair_cdf summed over the pairs per
site (fp64, pair order) and reduced per pair over bins of sites (the defined fp64 order; the mean and the weighted sum),
without the tail rows crossing the bus.  Everything is np.array_equal against the numpy statement of
tests/pair_tail_lists.py on the oracle's posteriors (tests/test_pair_tail_lists.py shows what the standard inputs reach).

The ABI's outputs have no rows beyond the list (a cut's cells are [n_pairs][n_bins], the next cut follows at once), so the
sentinels are the caller's memory behind each array and, for the bin outputs, every cell before the call: a row written for
a dead lane of a ragged group would land in the next cut's cells or behind the array."""

import numpy as np
import pytest

import pair_cdf_lists as CL
import pair_tail_lists as TL
from conftest import expected_member
from fastsmc_amd import api, capi
from oracle import oracle as O
from pair_common import (EDGES_700, N_HAP, N_PAIRS, SITES, pairs_array as _pairs_array, upload as _upload,
                         open_context as _open, gpu_context, problem as _problem, cohort_files as _cohort_files,
                         params as _params, cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(small_problem):
    yield from gpu_context(small_problem)


GUARD = 64  # cells of caller memory behind every output, NaN before and after the call
NAMES = ("tail_sum", "bin_tail_mean", "bin_tail_length")


class Outputs:
    """The three output arrays as views of larger buffers: GUARD cells of NaN behind each; the bin outputs NaN all over,
    tail_sum the incoming accumulator (zeros, or `seed`)."""

    def __init__(self, n_tail, n, S, n_bins, want=(True, True, True), seed=None):
        shapes = ((n_tail, S), (n_tail, n, n_bins), (n_tail, n, n_bins))
        self.whole, self.out = [], []
        for shape, dt, w in zip(shapes, (np.float64, np.float32, np.float32), want):
            if not w:
                self.whole.append(None)
                self.out.append(None)
                continue
            cells = int(np.prod(shape))
            buf = np.full(cells + GUARD, np.nan, dt)
            view = buf[:cells].reshape(shape)
            if dt == np.float64:
                view[...] = 0.0 if seed is None else seed
            self.whole.append(buf)
            self.out.append(view)
        self.out = tuple(self.out)

    def guards_untouched(self):
        return all(b is None or bool(np.isnan(b[b.size - GUARD:]).all()) for b in self.whole)

    def bins_untouched(self):
        return all(o is None or bool(np.isnan(o).all()) for o in self.out[1:])


def _assert_equal(got, want, msg=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{name} {msg}: {int((g != w).sum())} of {g.size} cells differ"


def _run(ctx, model, n, S, cuts, edges=TL.EDGES, weights=None, want=(True, True, True), seed=None):
    o = Outputs(len(cuts), n, S, 0 if edges is None else len(edges) - 1, want, seed)
    got = ctx.decode_pair_tail_summaries(model, cuts, edges, weights, out=o.out)
    assert all(g is b for g, b in zip(got, o.out))
    assert o.guards_untouched()
    return got


def test_all_outputs_on_the_192_pairs_both_k69_kernels(small_problem, window_waves):
    # (a context opened here: the two-wave / one-wave choice of `window_waves` is read at every launch)
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    _upload(ctx, pm, TL.PAIRS_192)
    got = _run(ctx, model, 192, pm.S, CL.cuts(pm), weights=TL.widths(small_problem["gen"]))
    assert ctx.last_kernel() == 69
    assert ctx.last_waves_per_window() == (2 if window_waves == "two-waves-auto" else 1)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_tail_slices() >= 1
    ctx.close()
    assert got[0].shape == (4, 640) and got[1].shape == got[2].shape == (4, 192, 5)
    _assert_equal(got, TL.expected_192(small_problem))


# the cap: eight cuts in descending order with duplicates, c = K and c = 1 among them -- two passes of pair_cdf_kernel
CUTS_8 = [69, 40, 25, 25, 13, 2, 1, 1]


@pytest.mark.parametrize("cuts", [[25], [1], [69], CUTS_8], ids=["one-cut", "first-state", "all-states", "eight"])
def test_one_and_eight_cuts(gpu, small_problem, cuts):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, TL.PAIRS_192)
    got = _run(ctx, model, 192, pm.S, cuts, weights=TL.widths(small_problem["gen"]))
    _assert_equal(got, TL.expected_192(small_problem, cuts))


def test_slices_do_not_show(gpu, small_problem):
    ctx, model = gpu
    pm = small_problem["model"]
    want = TL.expected_192(small_problem)
    _upload(ctx, pm, TL.PAIRS_192)
    for slice_groups, n_slices in ((1, 3), (2, 2), (0, None)):
        ctx.set_pair_tail_slice(slice_groups)
        got = _run(ctx, model, 192, pm.S, CL.cuts(pm), weights=TL.widths(small_problem["gen"]))
        if n_slices is None:
            assert ctx.last_pair_tail_slices() >= 1
        else:
            assert ctx.last_pair_tail_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


@pytest.mark.parametrize("slice_groups", [0, 1, 2])
def test_ragged_list(gpu, small_problem, slice_groups):
    """150 pairs: the last group holds 22, its lanes 22 ... 63 are dead and add nothing to the sums; no cell but the
    list's is written (the guards of _run; every bin cell of the list is, none stays NaN)."""
    ctx, model = gpu
    pm = small_problem["model"]
    w = TL.widths(small_problem["gen"])
    _upload(ctx, pm, TL.PAIRS_192[:150])
    ctx.set_pair_tail_slice(slice_groups)
    got = _run(ctx, model, 150, pm.S, CL.cuts(pm), weights=w)
    _assert_equal(got, TL.expected(TL.tails_192(small_problem)[:, :150], TL.EDGES, w), f"slice {slice_groups}")


def test_chaining(gpu, small_problem):
    """Pairs 0-127 and then 128-191 in a second call that continues tail_sum give the bits of one call; a non-zero
    incoming accumulator is the start of the chain."""
    ctx, model = gpu
    pm = small_problem["model"]
    cuts = CL.cuts(pm)
    tails = TL.tails_192(small_problem)
    _upload(ctx, pm, TL.PAIRS_192[:128])
    first = _run(ctx, model, 128, pm.S, cuts, edges=None, want=(True, False, False))[0]
    assert np.array_equal(first, TL.tail_sum(tails[:, :128]))
    _upload(ctx, pm, TL.PAIRS_192[128:])
    second = _run(ctx, model, 64, pm.S, cuts, edges=None, want=(True, False, False), seed=first)[0]
    assert np.array_equal(second, TL.expected_192(small_problem)[0])
    seed = np.random.default_rng(3).random((4, pm.S)) * 1e3 + 0.1
    _upload(ctx, pm, TL.PAIRS_192)
    for slice_groups in (0, 1):
        ctx.set_pair_tail_slice(slice_groups)
        got = _run(ctx, model, 192, pm.S, cuts, edges=None, want=(True, False, False), seed=seed)[0]
        assert np.array_equal(got, TL.tail_sum(tails, seed)), slice_groups


def test_the_sum_alone_and_the_bins_alone(gpu, small_problem):
    ctx, model = gpu
    pm = small_problem["model"]
    w = TL.widths(small_problem["gen"])
    want = TL.expected_192(small_problem)
    _upload(ctx, pm, TL.PAIRS_192)
    for wanted, edges, weights in (((True, False, False), None, None), ((False, True, True), TL.EDGES, w),
                                   ((False, True, False), TL.EDGES, None), ((False, False, True), TL.EDGES, w),
                                   ((True, True, False), TL.EDGES, w)):
        got = _run(ctx, model, 192, pm.S, CL.cuts(pm), edges=edges, weights=weights, want=wanted)
        assert [g is not None for g in got] == list(wanted)
        _assert_equal(got, want, str(wanted))
    # the binding's defaults: the sum alone without edges, the mean with edges, the length with weights as well
    got = ctx.decode_pair_tail_summaries(model, CL.cuts(pm))
    assert got[1] is None and got[2] is None
    _assert_equal(got, want)
    got = ctx.decode_pair_tail_summaries(model, CL.cuts(pm), TL.EDGES, w)
    assert all(g is not None for g in got)
    _assert_equal(got, want)


def _other_kernel_case(pm, bits, folded, n_pairs):
    """Cuts [1, K / 2, K] -- the cut K reads the last state, and a walk into ghost states would move it -- on a list of
    two groups, the second ragged, slices of one group, against this model's own oracle posteriors; the edges end one site
    before S, inside the short last block of 64 sites, and the weights are a seeded vector."""
    pairs = O.enumerate_all_pairs(32)[:n_pairs]
    cuts = [1, pm.K // 2, pm.K]
    edges = np.array([3, 40, 41, pm.S - 1], np.int32)
    w = (np.random.default_rng(pm.K).random(pm.S) * 0.05 + 0.001).astype(np.float32)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.set_pair_tail_slice(1)
    got = _run(ctx, model, n_pairs, pm.S, cuts, edges=edges, weights=w)
    member, slices = ctx.last_kernel(), ctx.last_pair_tail_slices()
    ctx.close()
    assert member == expected_member(pm.K)
    assert slices == 2
    tails = CL.expected(pm, folded, pairs, cuts, [])[0]
    _assert_equal(got, TL.expected(tails, edges, w), f"K = {pm.K}, S = {pm.S}")


@pytest.mark.parametrize("K,S,n_pairs", [(40, 200, 96), (200, 200, 96), (1030, 120, 70)])
def test_other_kernels_and_a_short_last_site_block(K, S, n_pairs):
    """A padded member with ghost states (40 -> 48), the wave-group kernel (200 states), the any-K kernel (1030); S = 200
    and 120 are no multiples of the 64 sites of a block."""
    pm, bits, folded = _problem(K, S=S)
    _other_kernel_case(pm, bits, folded, n_pairs)


def test_sequence_mode(seq_problem):
    _other_kernel_case(seq_problem["model"], seq_problem["bits"], seq_problem["folded"], 100)


def test_errors(gpu, small_problem):
    ctx, model = gpu
    pm = small_problem["model"]
    w = TL.widths(small_problem["gen"])
    _upload(ctx, pm, TL.PAIRS_192)

    def good(msg):
        _assert_equal(_run(ctx, model, 192, pm.S, [25], weights=w), TL.expected_192(small_problem, [25]), msg)

    def refused(text, cuts=(25,), edges=TL.EDGES, weights=w, want=(True, True, True)):
        o = Outputs(len(cuts), 192, pm.S, 0 if edges is None else max(len(edges) - 1, 0), want, seed=7.5)
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_tail_summaries(model, cuts, edges, weights, out=o.out)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert o.guards_untouched() and o.bins_untouched()
        assert o.out[0] is None or bool((o.out[0] == 7.5).all())
        good("after: " + text)

    refused("at least one output", edges=None, weights=None, want=(False, False, False))
    refused("at least one output", want=(False, False, False))
    refused("one tail state at least", cuts=())
    refused("at most 8 tail states", cuts=[1] * 9)
    for c in (0, -3, 70):
        refused("outside [1, K]", cuts=[25, c])
    refused("bin outputs need bin edges", edges=None, want=(True, True, False))
    refused("bin outputs need bin edges", edges=None, want=(False, False, True))
    refused("need one bin at least", edges=[])
    refused("need one bin at least", edges=[5])
    refused("strictly ascending", edges=[0, 5, 5, 9])
    refused("strictly ascending", edges=[9, 5])
    refused("more bins than sites", edges=list(range(642)))
    refused("bin edges must lie in [0, sites]", edges=[-1, 5])
    refused("bin edges must lie in [0, sites]", edges=[0, 641])
    refused("bin_tail_length needs site weights", weights=None)
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[639] = bad
        refused("site weight 639 is not finite", weights=wb)
    # weights that are not finite are no matter where the length is not asked for
    wb = w.copy()
    wb[0] = np.nan
    _assert_equal(_run(ctx, model, 192, pm.S, [25], weights=wb, want=(True, True, False)),
                  TL.expected_192(small_problem, [25]))
    # a windowed group
    groups = capi.whole_sequence_groups(len(TL.PAIRS_192), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(TL.PAIRS_192), groups)
    o = Outputs(1, 192, pm.S, len(TL.EDGES) - 1)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_tail_summaries(model, [25], TL.EDGES, w, out=o.out)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value)
    assert o.guards_untouched() and o.bins_untouched() and bool((o.out[0] == 0).all())
    _upload(ctx, pm, TL.PAIRS_192)
    good("after the windowed group")


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

NEW_FIELDS = ("tail_summary_times", "tail_summary_states", "site_weights", "sum_of_tail_probabilities",
              "per_pair_bin_tail_means", "per_pair_bin_tail_lengths")
OLD_FIELDS = ("sum_of_posteriors", "per_pair_posterior_means", "min_posterior_means", "argmin_posterior_means",
              "per_pair_MAPs", "min_MAPs", "argmin_MAPs", "bin_edges", "bin_mean_posterior_means",
              "bin_min_posterior_means", "bin_argmin_posterior_means", "bin_min_MAPs", "bin_argmin_MAPs", "tail_times",
              "tail_states", "quantiles", "per_pair_tail_probabilities", "per_pair_quantile_states")


def _summaries(res):
    return (np.array(res.sum_of_tail_probabilities), np.array(res.per_pair_bin_tail_means),
            np.array(res.per_pair_bin_tail_lengths))


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, tail_summary_times=[50, 200], site_bins=..., site_weights=api.site_widths(map)) on a
    synthetic cohort's files.  sum_of_tail_probabilities is the fp64 pair-order chain over the per_pair_tail_probabilities
    rows a SEPARATE call with tail_times= returns, the bin outputs are the statement applied to those rows (and those rows
    are the oracle's).  With FSMC_DIAG_FLUSH_PAIRS=128 the queue is decoded every 128 pairs: two flushes (128 and 72
    pairs) continue one sum and fill the bin outputs at the pairs written so far.  A call without the new keywords returns
    the new fields empty and every other field as a call with them does; refused arguments raise and leave the results."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, tables, haps, derived, folded = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    times = [50, 200]
    gen = np.array(api.Data(p).geneticPositions, np.float32)
    w = api.site_widths(gen)
    assert np.array_equal(w, TL.widths(gen)) and np.unique(w).size > 100
    cuts = api.tail_states(tables.discretization, times)

    # the rows, from a call of their own, are the oracle's
    asmc.decodePairs(a, b, tail_times=times)
    res = asmc.get_copy_of_results()
    rows = np.array(res.per_pair_tail_probabilities)
    assert rows.shape == (2, N_PAIRS, SITES) and rows.dtype == np.float32
    pm = O.prepare_model(tables, gen, haps.bp, derived, N_HAP, time=p.time, no_conditional_age_estimates=False)
    assert np.array_equal(rows, CL.expected(pm, folded, pairs, cuts, [])[0])
    assert all(np.array(getattr(res, name)).size == 0 for name in NEW_FIELDS)
    want = TL.expected(rows, EDGES_700, w)

    # all three
    asmc.decodePairs(a, b, tail_summary_times=times, site_bins=EDGES_700, site_weights=w)
    res = asmc.get_copy_of_results()
    assert np.array(res.tail_summary_times).tolist() == times
    assert np.array(res.tail_summary_states).tolist() == cuts.tolist()
    assert np.array_equal(np.array(res.site_weights), w)
    got = _summaries(res)
    assert got[0].dtype == np.float64 and got[0].shape == (2, SITES)
    assert got[1].shape == got[2].shape == (2, N_PAIRS, len(EDGES_700) - 1)
    _assert_equal(got, want, "all three")
    # the rows are not stored, nor anything else that was not asked for
    assert np.array(res.per_pair_tail_probabilities).size == 0 and np.array(res.tail_states).size == 0
    assert len(res.per_pair_posteriors) == 0 and np.array(res.sum_of_posteriors).size == 0
    assert np.array(res.per_pair_posterior_means).size == 0 and np.array(res.per_pair_MAPs).size == 0

    # the sum alone; the sum and the means
    asmc.decodePairs(a, b, tail_summary_times=times)
    got = _summaries(asmc.get_copy_of_results())
    assert np.array_equal(got[0], want[0]) and got[1].size == 0 and got[2].size == 0
    asmc.decodePairs(a, b, tail_summary_times=times, site_bins=EDGES_700)
    got = _summaries(asmc.get_copy_of_results())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].size == 0
    # the sum starts again with every call: a shorter list
    asmc.decodePairs(a[:70], b[:70], tail_summary_times=times)
    assert np.array_equal(np.array(asmc.get_copy_of_results().sum_of_tail_probabilities), TL.tail_sum(rows[:, :70]))

    # the fields that were there before do not see the new keywords
    old = dict(sum_of_posteriors=True, per_pair_posterior_means=True, per_pair_MAPs=True, site_bins=EDGES_700,
               tail_times=times, quantiles=[0.5])
    asmc.decodePairs(a, b, **old)
    before = asmc.get_copy_of_results()
    assert all(np.array(getattr(before, name)).size == 0 for name in NEW_FIELDS)
    assert np.array_equal(np.array(before.per_pair_tail_probabilities), rows)
    asmc.decodePairs(a, b, **old, tail_summary_times=times, site_weights=w)
    after = asmc.get_copy_of_results()
    for name in OLD_FIELDS:
        x, y = np.array(getattr(before, name)), np.array(getattr(after, name))
        assert x.size > 0 and x.dtype == y.dtype and np.array_equal(x, y), name
    assert before.per_pair_indices == after.per_pair_indices
    _assert_equal(_summaries(after), want, "together with the older outputs")

    # refused arguments raise before anything is touched
    wb = w.copy()
    wb[3] = np.nan
    for kwargs, text in ((dict(tail_summary_times=[0.0]), "no interval"),
                         (dict(tail_summary_times=[50] * 9), "at most 8 tail states"),
                         (dict(site_weights=w, site_bins=EDGES_700), "site weights need tail summary times"),
                         (dict(tail_summary_times=times, site_weights=w), "site weights need site bins"),
                         (dict(tail_summary_times=times, site_bins=EDGES_700, site_weights=w[:-1]), "699 values for 700"),
                         (dict(tail_summary_times=times, site_bins=EDGES_700, site_weights=wb), "not finite")):
        with pytest.raises(RuntimeError, match=text):
            asmc.decodePairs(a, b, **kwargs)
        _assert_equal(_summaries(asmc.get_ref_of_results()), want, "after a refused call")
