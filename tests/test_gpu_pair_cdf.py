"""fsmc_decode_pair_cdf on the GPU: per pair and site, tail probabilities at state cuts and quantile states of the
posterior, computed on the device without the [K][S] tables crossing the bus.  Everything is np.array_equal against the
numpy statement of tests/pair_cdf_lists.py on the oracle's posteriors (tests/test_pair_cdf_lists.py shows what the
standard cuts and quantiles reach: the order of the sum, the `>=` rule and the K-1 fallback all show in the expected
values).  No test here can put a NaN into the posteriors: the NaN rule of the kernel's comment is not tested."""
import ctypes as C

import numpy as np
import pytest

import pair_cdf_lists as CL
from conftest import expected_member
from fastsmc_amd import api, capi
from oracle import oracle as O
from pair_common import (N_HAP, N_PAIRS, SITES, pairs_array as _pairs_array, upload as _upload,
                         open_context as _open, gpu_context, problem as _problem, cohort_files as _cohort_files,
                         params as _params, cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(small_problem):
    yield from gpu_context(small_problem)


INT_MIN = np.iinfo(np.int32).min


def _sentinels(n_tail, n_q, rows, S):
    """(tail, qstate) output arrays prefilled with values no result has: NaN and INT_MIN."""
    return np.full((n_tail, rows, S), np.nan, np.float32), np.full((n_q, rows, S), INT_MIN, np.int32)


def _untouched(a):
    return bool(np.isnan(a).all()) if a.dtype == np.float32 else bool((a == INT_MIN).all())


def _assert_equal(got, want, msg=""):
    for name, g, w in zip(("tail", "qstate"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{name} {msg}: {int((g != w).sum())} of {g.size} cells differ"


def test_all_outputs_on_the_192_pairs_both_k69_kernels(small_problem, window_waves):
    # (a context opened here: the two-wave / one-wave choice of `window_waves` is read at every launch)
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    _upload(ctx, pm, CL.PAIRS_192)
    got = ctx.decode_pair_cdf(model, CL.cuts(pm), CL.QS)
    assert ctx.last_kernel() == 69
    assert ctx.last_waves_per_window() == (2 if window_waves == "two-waves-auto" else 1)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_cdf_slices() >= 1
    ctx.close()
    assert got[0].shape == got[1].shape == (4, 192, 640)
    _assert_equal(got, CL.expected_192(small_problem))


# the caps: eight of each, in descending order, with duplicates -- four passes of the kernel over the dump
CUTS_8 = [69, 40, 25, 25, 13, 2, 1, 1]
QS_8 = [1.0, 0.975, 0.975, 0.5, 0.3, 0.1, 0.025, 0.001]


@pytest.mark.parametrize("cuts,qs", [([25], []), ([], [0.5]), (CUTS_8, QS_8), ([69, 1, 25, 7, 33], [0.5])],
                         ids=["one-cut", "one-quantile", "eight-and-eight", "five-and-one"])
def test_subsets(gpu, small_problem, cuts, qs):
    """One pass with a single output of either kind, a last pass that is not full (6 outputs), and the caps."""
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, CL.PAIRS_192)
    got = ctx.decode_pair_cdf(model, cuts, qs)
    assert got[0].shape == (len(cuts), 192, 640) and got[1].shape == (len(qs), 192, 640)
    _assert_equal(got, CL.expected_192(small_problem, cuts, qs))


def test_slices_do_not_show(gpu, small_problem):
    ctx, model = gpu
    pm = small_problem["model"]
    want = CL.expected_192(small_problem)
    _upload(ctx, pm, CL.PAIRS_192)
    for slice_groups, n_slices in ((1, 3), (2, 2), (0, None)):
        ctx.set_pair_cdf_slice(slice_groups)
        got = ctx.decode_pair_cdf(model, CL.cuts(pm), CL.QS)
        if n_slices is None:
            assert ctx.last_pair_cdf_slices() >= 1
        else:
            assert ctx.last_pair_cdf_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


@pytest.mark.parametrize("slice_groups", [0, 1, 2])
def test_ragged_list_and_rows_beyond_it(gpu, small_problem, slice_groups):
    """150 pairs: the last group holds 22, its lanes 22 ... 63 are dead.  The output arrays have 170 rows a matrix; rows
    150 ... 169, where the dead lanes' rows would land, stay untouched."""
    ctx, model = gpu
    pm = small_problem["model"]
    want = CL.expected_192(small_problem)
    _upload(ctx, pm, CL.PAIRS_192[:150])
    ctx.set_pair_cdf_slice(slice_groups)
    bufs = _sentinels(4, 4, 170, pm.S)
    got = ctx.decode_pair_cdf(model, CL.cuts(pm), CL.QS, out=bufs)
    assert got[0] is bufs[0] and got[1] is bufs[1]
    for name, g, w in zip(("tail", "qstate"), got, want):
        assert np.array_equal(g[:, :150], w[:, :150]), name
        assert _untouched(g[:, 150:]), name


@pytest.mark.parametrize("slice_groups", [0, 1])
def test_short_row_copies_do_not_show(small_problem, monkeypatch, slice_groups):
    """The ragged list of 150 pairs through pinned buffers of 4000 bytes: 1000 cells a copy, no multiple of the 640
    sites, so copies straddle rows.  A slice of 64 pairs leaves in 41 copies per output, the last of 960 cells, the
    slice of 22 pairs in 15, the last of 80 cells -- and on the device an output's rows lie 64 x 640 cells apart, more
    than that slice holds; the automatic slice, all 150 pairs, in 96 full copies per output."""
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", "4000")
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    want = CL.expected_192(small_problem)
    _upload(ctx, pm, CL.PAIRS_192[:150])
    ctx.set_pair_cdf_slice(slice_groups)
    bufs = _sentinels(4, 4, 170, pm.S)
    got = ctx.decode_pair_cdf(model, CL.cuts(pm), CL.QS, out=bufs)
    slices = ctx.last_pair_cdf_slices()
    ctx.close()
    assert slices == (3 if slice_groups else 1)
    for name, g, w in zip(("tail", "qstate"), got, want):
        assert np.array_equal(g[:, :150], w[:, :150]), name
        assert _untouched(g[:, 150:]), name


def _other_kernel_case(pm, bits, folded, n_pairs):
    """Cuts [1, K / 2, K] and quantiles [0.025, 0.5, 1.0] -- the cut K and q = 1.0 read the last state, and a walk into
    ghost states would move them -- on a list of two groups, the second ragged, slices of one group, inside arrays with
    sentinel rows beyond the list, against this model's own oracle posteriors."""
    pairs = O.enumerate_all_pairs(32)[:n_pairs]
    cuts, qs = [1, pm.K // 2, pm.K], [0.025, 0.5, 1.0]
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.set_pair_cdf_slice(1)
    bufs = _sentinels(3, 3, n_pairs + 5, pm.S)
    ctx.decode_pair_cdf(model, cuts, qs, out=bufs)
    member, slices = ctx.last_kernel(), ctx.last_pair_cdf_slices()
    ctx.close()
    assert member == expected_member(pm.K)
    assert slices == 2
    want = CL.expected(pm, folded, pairs, cuts, qs)
    _assert_equal(tuple(b[:, :n_pairs] for b in bufs), want, f"K = {pm.K}, S = {pm.S}")
    assert all(_untouched(b[:, n_pairs:]) for b in bufs)


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
    _upload(ctx, pm, CL.PAIRS_192)
    lib = capi.load()

    def good(msg):
        _assert_equal(ctx.decode_pair_cdf(model, [25], [0.5]), CL.expected_192(small_problem, [25], [0.5]), msg)

    def refused(text, cuts=(), qs=()):
        bufs = _sentinels(len(cuts), len(qs), 192, pm.S)
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_cdf(model, cuts, qs, out=bufs)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert all(_untouched(b) for b in bufs)
        good("after: " + text)

    def raw(text, cuts, n_tail, tail_ptrs, qs, n_q, q_ptrs):
        """Straight through ctypes: what the binding would not let through."""
        rc = lib.fsmc_decode_pair_cdf(ctx._h, model._h, cuts, n_tail, tail_ptrs, qs, n_q, q_ptrs)
        assert rc == -1
        with pytest.raises(capi.FsmcError) as ei:
            ctx._check(rc)
        assert text in str(ei.value), (text, str(ei.value))
        good("after: " + text)

    refused("at least one output")
    refused("at most 8 tail states", cuts=[1] * 9)
    refused("at most 8 quantiles", qs=[0.5] * 9)
    for c in (0, -3, 70):
        refused("outside [1, K]", cuts=[25, c])
    for q in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused("not finite or outside (0, 1]", qs=[0.5, q])
    # null arrays where the count is not zero, null row pointers
    tail, qstate = _sentinels(2, 2, 192, pm.S)
    cuts = np.array([25, 69], np.int32)
    qs = np.array([0.5, 1.0], np.float32)
    tp = (C.c_void_p * 2)(tail[0].ctypes.data, tail[1].ctypes.data)
    qp = (C.c_void_p * 2)(qstate[0].ctypes.data, qstate[1].ctypes.data)
    vp = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    raw("tail_states or tail_rows is null", None, 2, vp(tp), qs.ctypes.data, 2, vp(qp))
    raw("tail_states or tail_rows is null", cuts.ctypes.data, 2, None, qs.ctypes.data, 2, vp(qp))
    raw("quantiles or quantile_rows is null", cuts.ctypes.data, 2, vp(tp), None, 2, vp(qp))
    raw("quantiles or quantile_rows is null", cuts.ctypes.data, 2, vp(tp), qs.ctypes.data, 2, None)
    tp_hole = (C.c_void_p * 2)(tail[0].ctypes.data, None)
    qp_hole = (C.c_void_p * 2)(None, qstate[1].ctypes.data)
    raw("tail_rows[1] is null", cuts.ctypes.data, 2, vp(tp_hole), qs.ctypes.data, 2, vp(qp))
    raw("quantile_rows[0] is null", cuts.ctypes.data, 2, vp(tp), qs.ctypes.data, 2, vp(qp_hole))
    assert _untouched(tail) and _untouched(qstate)
    # a windowed group
    groups = capi.whole_sequence_groups(len(CL.PAIRS_192), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(CL.PAIRS_192), groups)
    bufs = _sentinels(1, 1, 192, pm.S)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_cdf(model, [25], [0.5], out=bufs)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value)
    assert all(_untouched(b) for b in bufs)
    _upload(ctx, pm, CL.PAIRS_192)
    good("after the windowed group")


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

def _cdf(res):
    return np.array(res.per_pair_tail_probabilities), np.array(res.per_pair_quantile_states)


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, tail_times=[50, 200], quantiles=[0.025, 0.5, 0.975]) on a synthetic cohort's files: the
    two stacks equal the reduction of tests/pair_cdf_lists.py on the oracle's posteriors of the same pairs.  With
    FSMC_DIAG_FLUSH_PAIRS=128 the queue is decoded every 128 pairs: two flushes (128 and 72 pairs) fill the stacks at
    the pairs written so far.  With these outputs alone the tables, means and MAPs stay empty; together with
    per_pair_posteriors=True both sets of results are the ones each gives alone; tail_times=[params.time] cuts at the
    IBD scan's state threshold; a time no interval starts below and a bad quantile raise and leave the results."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, tables, haps, derived, folded = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    times, qs = [50, 200], [0.025, 0.5, 0.975]
    # the oracle on the data as the ASMC-mode readers see it
    gen = np.array(api.Data(p).geneticPositions, np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, N_HAP, time=p.time, no_conditional_age_estimates=False)
    cuts = api.tail_states(tables.discretization, times)
    want = CL.expected(pm, folded, pairs, cuts, qs)

    asmc.decodePairs(a, b, tail_times=times, quantiles=qs)
    res = asmc.get_copy_of_results()
    assert np.array(res.tail_times).tolist() == times and np.array(res.tail_states).tolist() == cuts.tolist()
    assert np.array_equal(np.array(res.quantiles), np.array(qs, np.float32))
    got = _cdf(res)
    assert got[0].shape == (2, N_PAIRS, SITES) and got[1].shape == (3, N_PAIRS, SITES)
    _assert_equal(got, want, "tails and quantiles alone")
    # nothing else was stored
    assert len(res.per_pair_posteriors) == 0 and np.array(res.sum_of_posteriors).size == 0
    assert np.array(res.per_pair_posterior_means).size == 0 and np.array(res.per_pair_MAPs).size == 0
    assert np.array(res.min_posterior_means).size == 0 and np.array(res.min_MAPs).size == 0
    # the decoding time cuts at the IBD scan's state threshold
    asmc.decodePairs(a[:70], b[:70], tail_times=[p.time])
    res = asmc.get_copy_of_results()
    threshold = int(asmc.hmm().preparedModel()["state_threshold"])
    assert np.array(res.tail_states).tolist() == [threshold] == [pm.state_threshold]
    assert np.array(res.per_pair_quantile_states).size == 0
    assert np.array_equal(np.array(res.per_pair_tail_probabilities),
                          CL.expected(pm, folded, pairs[:70], [threshold], [])[0])
    # the tables alone, then both together
    asmc.decodePairs(a, b, per_pair_posteriors=True)
    res = asmc.get_copy_of_results()
    tables_alone = np.array(res.per_pair_posteriors)
    assert tables_alone.shape[0] == N_PAIRS and tables_alone.size == N_PAIRS * 69 * SITES
    assert all(x.size == 0 for x in _cdf(res)) and np.array(res.tail_states).size == 0
    asmc.decodePairs(a, b, per_pair_posteriors=True, tail_times=times, quantiles=qs)
    res = asmc.get_copy_of_results()
    _assert_equal(_cdf(res), want, "together with the tables")
    assert np.array_equal(np.array(res.per_pair_posteriors), tables_alone)
    # refused arguments raise before anything is touched
    for kwargs, text in ((dict(tail_times=[0.0]), "no interval"), (dict(quantiles=[0.0]), "outside"),
                         (dict(quantiles=[0.5] * 9), "at most 8 quantiles"),
                         (dict(tail_times=[50] * 9), "at most 8 tail states")):
        with pytest.raises(RuntimeError, match=text):
            asmc.decodePairs(a, b, **kwargs)
        _assert_equal(_cdf(asmc.get_ref_of_results()), want, "after a refused call")
