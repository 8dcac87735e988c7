"""fsmc_decode_pair_bins on the GPU: per pair, the mean (in its defined fp64 order), min and argmin of the posterior-mean
row and the min and argmin (lowest site) of the MAP row over bins of sites, computed on the device without the
[pairs][sites] rows crossing the bus.  Everything is np.array_equal against the numpy statement of
tests/pair_bins_lists.py on the oracle's rows (tests/test_pair_bins_lists.py shows what the edge sets reach).  No test
here can put a NaN into the rows: the NaN rule of the kernel's comment is not tested."""

import numpy as np
import pytest

import pair_bins_lists as BL
from conftest import expected_member
from fastsmc_amd import api, capi
from oracle import oracle as O
from pair_common import (pairs_array as _pairs_array, upload as _upload, open_context as _open, gpu_context,
                         problem as _problem, example_files as _example_files, asmc as _asmc)

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(small_problem):
    yield from gpu_context(small_problem)


INT_MIN = np.iinfo(np.int32).min


def _assert_equal(got, want, msg=""):
    assert len(got) == len(want) == 5
    for name, g, w in zip(BL.NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{name} {msg}: {int((g != w).sum())} of {g.size} cells differ"


def _sentinels(n, B):
    """Five output arrays [n][B] prefilled with values no result has: NaN for the floats, INT_MIN for the ints."""
    return tuple(np.full((n, B), np.nan if dt == np.float32 else INT_MIN, dt) for dt in BL.DTYPES)


def _untouched(a):
    return bool(np.isnan(a).all()) if a.dtype == np.float32 else bool((a == INT_MIN).all())


@pytest.mark.parametrize("edges", ["E1", "E2", "E3", "E4"])
def test_all_outputs_on_the_192_pairs(gpu, small_problem, edges):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, BL.PAIRS_192)
    got = ctx.decode_pair_bins(model, pm.exp_times, BL.EDGE_SETS[edges])
    assert ctx.last_kernel() == 69
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_bins_slices() == 1
    _assert_equal(got, BL.expected_192(small_problem, edges), edges)


def test_k69_both_kernels(small_problem, window_waves):
    # (a context opened here: the two-wave / one-wave choice of `window_waves` is read at every launch)
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    _upload(ctx, pm, BL.PAIRS_192)
    got = ctx.decode_pair_bins(model, pm.exp_times, BL.E3)
    assert ctx.last_kernel() == 69
    assert ctx.last_waves_per_window() == (2 if window_waves == "two-waves-auto" else 1)
    _assert_equal(got, BL.expected_192(small_problem, "E3"), "against the oracle")
    # the same reduction of the library's own rows
    mean, mp = ctx.decode_per_pair(model, pm.exp_times)
    _assert_equal(got, BL.expected(mean, mp, BL.E3), "against decode_per_pair's rows")
    ctx.close()


def test_mean_outputs_only_then_map_outputs_only(gpu, small_problem):
    """The pointers not asked for are null; their buffers, prefilled, stay as they were (they never reach the library)."""
    ctx, model = gpu
    pm = small_problem["model"]
    want = BL.expected_192(small_problem, "E3")
    B = len(BL.E3) - 1
    _upload(ctx, pm, BL.PAIRS_192)
    for keep in ((0, 1, 2), (3, 4), (0,), (1, 2)):
        bufs = _sentinels(192, B)
        got = ctx.decode_pair_bins(model, pm.exp_times, BL.E3, out=tuple(b if i in keep else None
                                                                          for i, b in enumerate(bufs)))
        for i in range(5):
            if i in keep:
                assert got[i] is bufs[i] and np.array_equal(bufs[i], want[i]), (keep, BL.NAMES[i])
            else:
                assert got[i] is None and _untouched(bufs[i]), (keep, BL.NAMES[i])
    # by switch: the arrays the binding makes
    got = ctx.decode_pair_bins(model, pm.exp_times, BL.E3, want_min_map=False)
    assert got[3] is None and got[4] is None and all(np.array_equal(got[i], want[i]) for i in (0, 1, 2))
    got = ctx.decode_pair_bins(model, pm.exp_times, BL.E3, want_mean=False, want_min_mean=False)
    assert got[0] is None and got[1] is None and got[2] is None
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])


@pytest.mark.parametrize("edges", ["E3", "E2"])
def test_slices_do_not_show(gpu, small_problem, edges):
    ctx, model = gpu
    pm = small_problem["model"]
    want = BL.expected_192(small_problem, edges)
    _upload(ctx, pm, BL.PAIRS_192)
    for slice_groups, n_slices in ((1, 3), (2, 2), (0, 1)):
        ctx.set_pair_bins_slice(slice_groups)
        got = ctx.decode_pair_bins(model, pm.exp_times, BL.EDGE_SETS[edges])
        assert ctx.last_pair_bins_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


@pytest.mark.parametrize("slice_groups", [0, 1, 2])
def test_ragged_list_and_rows_beyond_it(gpu, small_problem, slice_groups):
    """150 pairs: the last group holds 22.  The output buffers have 170 rows; rows 150 ... 169 stay untouched."""
    ctx, model = gpu
    pm = small_problem["model"]
    want = BL.expected_192(small_problem, "E3")
    B = len(BL.E3) - 1
    _upload(ctx, pm, BL.PAIRS_192[:150])
    ctx.set_pair_bins_slice(slice_groups)
    bufs = _sentinels(170, B)
    got = ctx.decode_pair_bins(model, pm.exp_times, BL.E3, out=bufs)
    assert ctx.last_pair_bins_slices() == {0: 1, 1: 3, 2: 2}[slice_groups]
    for name, g, w in zip(BL.NAMES, got, want):
        assert np.array_equal(g[:150], w[:150]), name
        assert _untouched(g[150:]), name


def _other_kernel_case(pm, bits, folded, n_pairs):
    """E3 (cut to the model's sites) on a list of two groups, the second ragged, slices of one group, against this
    model's own oracle rows."""
    pairs = O.enumerate_all_pairs(32)[:n_pairs]
    edges = np.array([e for e in BL.E3 if e < pm.S] + [pm.S - 1], np.int32)
    assert (np.diff(edges) > 0).all()
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.set_pair_bins_slice(1)
    got = ctx.decode_pair_bins(model, pm.exp_times, edges)
    member, slices = ctx.last_kernel(), ctx.last_pair_bins_slices()
    ctx.close()
    assert member == expected_member(pm.K)
    assert slices == 2
    mean, mp = BL.oracle_rows(pm, folded, pairs)
    _assert_equal(got, BL.expected(mean, mp, edges), f"K = {pm.K}, S = {pm.S}")


@pytest.mark.parametrize("K,S,n_pairs", [(40, 200, 96), (200, 200, 96)])
def test_other_kernels(K, S, n_pairs):
    """A padded member with ghost states (40 -> 48) and the wave-group kernel (200 states); S = 200: E3 becomes
    [5, 70, 71, 199]."""
    pm, bits, folded = _problem(K, S=S)
    _other_kernel_case(pm, bits, folded, n_pairs)


def test_sequence_mode(seq_problem):
    _other_kernel_case(seq_problem["model"], seq_problem["bits"], seq_problem["folded"], 100)


def test_errors(gpu, small_problem):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, BL.PAIRS_192)
    B = len(BL.E3) - 1

    def refused(text, edges=BL.E3, keep=(0, 1, 2, 3, 4), times=pm.exp_times, n_bins=None):
        bufs = _sentinels(192, B if n_bins is None else n_bins)
        out = tuple(b if i in keep else None for i, b in enumerate(bufs))
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_bins(model, times, edges, out=out)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert all(_untouched(b) for b in bufs)

    refused("at least one output", keep=())
    refused("bin edges", edges=None, n_bins=0)  # (null edges)
    for keep in ((1,), (2,), (3,), (4,), (0, 1), (0, 2, 3, 4), (1, 2, 3)):  # a minimum without its argmin, or the reverse
        refused("come together", keep=keep)
    refused("one bin at least", edges=[7], n_bins=0)
    refused("strictly ascending", edges=[5, 70, 70, 200, 639])
    refused("strictly ascending", edges=[5, 70, 60, 200, 639])
    refused("[0, sites]", edges=[-1, 70, 71, 200, 639])
    refused("[0, sites]", edges=[5, 70, 71, 200, 641])
    # null times: the binding insists on an array, so straight through ctypes
    e3 = np.ascontiguousarray(BL.E3)
    bufs = _sentinels(192, B)
    rc = capi.load().fsmc_decode_pair_bins(ctx._h, model._h, None, e3.ctypes.data, B, *[b.ctypes.data for b in bufs])
    assert rc == -1 and all(_untouched(b) for b in bufs)
    assert ctx.last_pair_bins_slices() == 0  # (nothing ran)
    groups = capi.whole_sequence_groups(len(BL.PAIRS_192), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(BL.PAIRS_192), groups)
    refused("whole-sequence")
    # the context is usable afterwards; edges [0, S] are the widest allowed
    _upload(ctx, pm, BL.PAIRS_192)
    _assert_equal(ctx.decode_pair_bins(model, pm.exp_times, BL.E1), BL.expected_192(small_problem, "E1"),
                  "after the errors")


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

def _five(res):
    return (np.array(res.bin_mean_posterior_means), np.array(res.bin_min_posterior_means),
            np.array(res.bin_argmin_posterior_means), np.array(res.bin_min_MAPs), np.array(res.bin_argmin_MAPs))


def _product_pairs():
    rng = np.random.default_rng(3)
    all_pairs = [(x, y) for y in range(300) for x in range(y)]
    pick = rng.choice(len(all_pairs), 300, replace=False)
    return [all_pairs[i] for i in pick]


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, per_pair_posterior_means=True, per_pair_MAPs=True, site_bins=E3): the five matrices equal
    the reduction by pair_bins_lists of the SAME call's rows.  With FSMC_DIAG_FLUSH_PAIRS=128 the queue is decoded every
    128 pairs: three flushes fill the matrices at the pairs written so far.  With bins alone the row matrices are
    empty and the five matrices the same; site_bins() of the map's cM positions gives strictly ascending edges and
    matrices [pairs][B]; without site_bins the bin fields are empty; bad edges raise."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, cm = _example_files(tmp_path)
    asmc = _asmc(root)
    pairs = _product_pairs()
    a, b = [int(p[0]) for p in pairs], [int(p[1]) for p in pairs]
    edges = [int(e) for e in BL.E3]
    asmc.decodePairs(a, b, per_pair_posterior_means=True, per_pair_MAPs=True, site_bins=edges)
    res = asmc.get_copy_of_results()
    rows_mean, rows_map = np.array(res.per_pair_posterior_means), np.array(res.per_pair_MAPs)
    S = rows_mean.shape[1]
    assert rows_mean.shape == rows_map.shape == (len(pairs), S) and S > 640
    assert np.array(res.bin_edges).tolist() == edges
    want = BL.expected(rows_mean, rows_map, BL.E3)
    _assert_equal(_five(res), want, "rows stored as well")
    indices = res.per_pair_indices
    # bins alone: no rows on the host
    asmc.decodePairs(a, b, site_bins=edges)
    res = asmc.get_copy_of_results()
    _assert_equal(_five(res), want, "bins alone")
    assert np.array(res.per_pair_posterior_means).size == 0 and np.array(res.per_pair_MAPs).size == 0
    assert np.array(res.min_posterior_means).size == 0 and np.array(res.min_MAPs).size == 0
    assert res.per_pair_indices == indices
    # windows of 1 cM over the map
    e_cm = api.site_bins(cm, 1.0)
    assert e_cm[0] == 0 and e_cm[-1] == S and (np.diff(e_cm) > 0).all() and e_cm.size > 3
    asmc.decodePairs(a, b, site_bins=e_cm)
    res = asmc.get_copy_of_results()
    got = _five(res)
    assert all(g.shape == (len(pairs), e_cm.size - 1) for g in got)
    _assert_equal(got, BL.expected(rows_mean, rows_map, e_cm), "1-cM windows")
    # without the keyword: as before, no bin field, the same rows (both flags: the MAP rows are stored under the
    # posterior-mean flag, as in the reference, so per_pair_MAPs alone would leave them zero)
    asmc.decodePairs(a, b, per_pair_posterior_means=True, per_pair_MAPs=True)
    res = asmc.get_copy_of_results()
    assert np.array(res.bin_edges).size == 0 and all(g.size == 0 for g in _five(res))
    assert np.array_equal(np.array(res.per_pair_posterior_means), rows_mean)
    assert np.array_equal(np.array(res.per_pair_MAPs), rows_map)
    for bad, text in (([5], "one bin at least"), ([5, 5], "strictly ascending"), ([0, S + 1], "[0, sites]"),
                      ([-1, 4], "[0, sites]")):
        with pytest.raises(RuntimeError, match=text.replace("[", r"\[").replace("]", r"\]")):
            asmc.decodePairs(a, b, site_bins=bad)
