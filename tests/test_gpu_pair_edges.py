"""The five posterior-reducing decodePairs entry points at the numeric edges: fsmc_decode_pair_cdf, _tail_summaries,
_posteriors, _minima and _bins on the edge models of tests/edge_models.py, with the cuts, quantiles, bin edges, site weights
and expected coalescence times of tests/pair_edge_lists.py -- subnormal posteriors, tails, weights, means and quantiles,
runs of exactly-zero posteriors, a quantile the running sum meets with equality and stays on, ties between the pairs of a
site and the sites of a bin, times of +0.0 and -0.0.  tests/test_pair_edge_lists.py shows on the CPU that each case
reaches its regime and which wrong rule would change the expected values.

There is no tolerance here: float outputs are compared as bit patterns (pair_edge_lists.assert_same_bits: -0.0 is not
+0.0), integer outputs with np.array_equal.  No test here can put a NaN or an infinity into the posteriors or the times:
the kernels' NaN rules are stated, not tested."""
import numpy as np
import pytest

import pair_bins_lists as BL
import pair_edge_lists as PL
import pair_tail_lists as TL
from conftest import expected_member
from fastsmc_amd import capi
from pair_common import upload as _upload
from test_gpu_pair_cdf import _sentinels as _cdf_sentinels, _untouched
from test_gpu_pair_bins import _sentinels as _bins_sentinels
from test_gpu_pair_tail import NAMES as TAIL_NAMES, _run as _run_tail

pytestmark = pytest.mark.gpu

N = 96        # pairs of every case: a full group and a half-full one
SPLIT = 40    # the first call of a chain over two calls takes pairs [0, 40), the second the other 56


def _open(case, pairs=slice(None)):
    """A context on the case's model with the haplotypes and the pairs uploaded as whole-sequence groups."""
    pm, bits, _, all_pairs = PL.model(*case)
    assert len(all_pairs) == N
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, all_pairs[pairs])
    return ctx, model, pm


def _cdf_case(case, waves=None):
    ctx, model, pm = _open(case)
    cuts, qs = PL.cuts(case), PL.quantiles(case)
    want = PL.expected_cdf(case)
    for slice_groups in (0, 1):
        ctx.set_pair_cdf_slice(slice_groups)
        bufs = _cdf_sentinels(len(cuts), len(qs), N + 5, pm.S)
        ctx.decode_pair_cdf(model, cuts, qs, out=bufs)
        assert ctx.last_kernel() == expected_member(pm.K)
        if waves is not None:
            assert ctx.last_waves_per_window() == waves
        if slice_groups:
            assert ctx.last_pair_cdf_slices() == 2
        for name, got, w in zip(("tail", "qstate"), bufs, want):
            PL.assert_same_bits(got[:, :N], w, f"{name}, slice {slice_groups}, {PL.case_id(case)}")
            assert _untouched(got[:, N:]), name
    ctx.close()


@pytest.mark.parametrize("case", PL.K69_CASES, ids=PL.case_id)
def test_cdf_k69_both_kernels(case, window_waves):
    _cdf_case(case, waves=2 if window_waves == "two-waves-auto" else 1)


@pytest.mark.parametrize("case", PL.K33_CASES + PL.K200_CASES + [PL.SEQ_CASE], ids=PL.case_id)
def test_cdf_padded_member_wave_group_and_sequence_mode(case):
    """33 states run on the 48-state member: its ghost states enter no running sum, no cut of K and not q = 1.0."""
    _cdf_case(case)


@pytest.mark.parametrize("case", PL.DUMP_CASES, ids=PL.case_id)
def test_tail_summaries(case):
    """tail_sum, bin_tail_mean and bin_tail_length with both edge sets and the subnormal / zero / 2^100 weights, in slices
    of one group; then tail_sum as one chain over two calls, pairs [0, 40) and [40, 96)."""
    ctx, model, pm = _open(case)
    cuts = PL.cuts(case)
    w = PL.site_weights(pm.S)
    ctx.set_pair_tail_slice(1)
    for name, edges in PL.edge_sets(pm.S).items():
        got = _run_tail(ctx, model, N, pm.S, cuts, edges=edges, weights=w)
        assert ctx.last_kernel() == expected_member(pm.K)
        assert ctx.last_pair_tail_slices() == 2
        for out, g, want in zip(TAIL_NAMES, got, PL.expected_tail(case, name)):
            PL.assert_same_bits(g, want, f"{out}, edges {name}, {PL.case_id(case)}")
    ctx.close()
    tail = PL.expected_cdf(case)[0]
    ctx, model, pm = _open(case, slice(0, SPLIT))
    first = _run_tail(ctx, model, SPLIT, pm.S, cuts, edges=None, want=(True, False, False))[0]
    PL.assert_same_bits(first, TL.tail_sum(tail[:, :SPLIT]), "tail_sum of the first 40 pairs")
    _upload(ctx, pm, PL.model(*case)[3][SPLIT:])
    second = _run_tail(ctx, model, N - SPLIT, pm.S, cuts, edges=None, want=(True, False, False), seed=first)[0]
    ctx.close()
    PL.assert_same_bits(second, TL.tail_sum_in_parts(tail, [SPLIT]), "tail_sum continued over two calls")
    PL.assert_same_bits(second, PL.expected_tail(case, "wide")[0], "two calls against one")


# the exact member with every variant of the times the tables are multiplied by; the padded member and the wave-group
# member with the subnormal products and the negative zeros
POSTERIOR_RUNS = [(c, v) for c in PL.POSTERIOR_CASES for v in (("own", "2^-140", "+0", "-0") if c[1] == 69 else
                                                               ("2^-140", "-0"))]


@pytest.mark.parametrize("case,variant", POSTERIOR_RUNS, ids=lambda x: PL.case_id(x) if isinstance(x, tuple) else x)
def test_posterior_tables(case, variant):
    """Rows and sum from an accumulator of +0.0; the sum from an accumulator of -0.0 (-0.0 + -0.0 stays -0.0, which only
    the bit patterns tell from the +0.0 case); the sum continued from the first call's result."""
    ctx, model, pm = _open(case)
    times = PL.times(case, variant)
    ctx.set_pair_posterior_slice(1)
    what = f"{PL.case_id(case)}, times {variant}"
    acc = np.zeros((pm.K, pm.S), np.float32)
    rows, s = ctx.decode_pair_posteriors(model, times, sum_into=acc)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_pair_posterior_slices() == 2
    want_rows, want_sum = PL.expected_posteriors(case, variant)
    PL.assert_same_bits(rows, want_rows, f"rows, {what}")
    PL.assert_same_bits(s, want_sum, f"sum from +0.0, {what}")
    del rows, want_rows
    minus = np.full((pm.K, pm.S), -0.0, np.float32)
    _, s2 = ctx.decode_pair_posteriors(model, times, want_rows=False, sum_into=minus.copy())
    PL.assert_same_bits(s2, PL.expected_posteriors(case, variant, acc=minus)[1], f"sum from -0.0, {what}")
    _, s3 = ctx.decode_pair_posteriors(model, times, want_rows=False, sum_into=s.copy())
    ctx.close()
    PL.assert_same_bits(s3, PL.expected_posteriors(case, variant, acc=want_sum)[1], f"sum continued, {what}")
    if variant == "-0":
        assert (PL.bits(s) == 0).all() and (PL.bits(s2) == 0x80000000).all() and (PL.bits(s3) == 0).all()


MINIMA_NAMES = ("min_mean", "argmin_mean", "min_map", "argmin_map")


@pytest.mark.parametrize("variant", PL.TIMES)
@pytest.mark.parametrize("case", PL.MINIMA_CASES, ids=PL.case_id)
def test_minima(case, variant):
    """One call in slices of one group (the combine kernel crosses a slice), then the chain of two calls, pair_base 0 and
    40.  With means that tie en masse the first pair of equal minima must win in the ranges, across them and across the
    calls; with all-zero means every site reports pair 0, and pair_base shows only where the MAP rows say so."""
    times = PL.times(case, variant)
    what = f"{PL.case_id(case)}, times {variant}"
    ctx, model, pm = _open(case)
    ctx.set_pair_minima_slice(1)
    got = ctx.decode_pair_minima(model, times)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_pair_minima_slices() == 2
    ctx.close()
    for name, g, want in zip(MINIMA_NAMES, got, PL.expected_minima(case, variant)):
        PL.assert_same_bits(g, want, f"{name}, one call, {what}")
    ctx, model, pm = _open(case, slice(0, SPLIT))
    state = ctx.decode_pair_minima(model, times)
    _upload(ctx, pm, PL.model(*case)[3][SPLIT:])
    chained = ctx.decode_pair_minima(model, times, pair_base=SPLIT, state=state)
    ctx.close()
    want = PL.expected_minima(case, variant, split=SPLIT)
    for name, g, w, one in zip(MINIMA_NAMES, chained, want, got):
        PL.assert_same_bits(g, w, f"{name}, two calls, {what}")
        PL.assert_same_bits(g, one, f"{name}, two calls against one, {what}")
    if variant in ("+0", "-0"):
        assert (PL.bits(chained[0]) == 0).all() and (chained[1] == 0).all()


@pytest.mark.parametrize("variant", PL.TIMES)
@pytest.mark.parametrize("case", PL.BINS_CASES, ids=PL.case_id)
def test_bins(case, variant):
    """All five outputs with both edge sets, in slices of one group, inside arrays with sentinel rows beyond the list.  The
    float tie rule (of equal means the lowest site) is decided by the degenerate model and by the few-ulp times, the int
    rule by the degenerate model, whose MAP is 0 everywhere: every argmin is the bin's first site."""
    times = PL.times(case, variant)
    ctx, model, pm = _open(case)
    ctx.set_pair_bins_slice(1)
    for name, edges in PL.edge_sets(pm.S).items():
        bufs = _bins_sentinels(N + 4, len(edges) - 1)
        ctx.decode_pair_bins(model, times, edges, out=bufs)
        assert ctx.last_kernel() == expected_member(pm.K)
        assert ctx.last_pair_bins_slices() == 2
        for out, g, want in zip(BL.NAMES, bufs, PL.expected_bins(case, variant, name)):
            PL.assert_same_bits(g[:N], want, f"{out}, edges {name}, {PL.case_id(case)}, times {variant}")
            assert _untouched(g[N:]), out
        if case[0] == "degenerate":
            assert np.array_equal(bufs[4][:N], np.broadcast_to(edges[:-1], (N, len(edges) - 1)))
    ctx.close()
