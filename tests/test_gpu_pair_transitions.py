"""fsmc_decode_pair_transitions on the GPU: per pair and site, the posterior probability that the state is lower / higher
than at the site before.  Every array is np.array_equal (two NaNs counting as equal) to the numpy restatement of
tests/pair_transition_lists.py; tests/test_pair_transition_lists.py shows on the CPU that the restatement's backward
vector is the oracle's, that it agrees with the fp64 two-slice posterior, and what the inputs below reach."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
import pair_transition_lists as TL
from conftest import expected_member
from fastsmc_amd import api, capi
from pair_common import (pairs_array as _pairs_array, upload as _upload, cohort_files as _cohort_files, params as _params,
                         cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -4


def _open(pm, bits):
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    return ctx, model


def _assert_equal(got, want, msg=""):
    assert got.dtype == np.float32 and got.shape == want.shape, (msg, got.dtype, got.shape, want.shape)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{msg}: {int((~same).sum())} of {got.size} values differ, first at {np.argwhere(~same)[0]}"


def _rows(ctx, model, **kw):
    down, up, _, _ = ctx.decode_pair_transitions(model, **kw)
    return down, up


@pytest.mark.parametrize("name", TL.MODEL_CASES + TL.SITE_CASES)
def test_models_and_sites(name):
    """The members of the family (K = 2 ... 128, exact and padded) at 129 sites (300 at K = 40) and 1 ... 200 sites at
    K = 69 -- row ends of every alignment for the float4 stores -- with 70 pairs: a full group and a ragged one."""
    pm, bits, _, pairs, wd, wu = TL.case(name, first=70)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    down, up = _rows(ctx, model)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_transitions_slices() == 1
    info = ctx.info()
    assert info["chunk_sites"] == pm.S and info["max_chunks"] == 1
    ctx.close()
    _assert_equal(down, wd, name + " down")
    _assert_equal(up, wu, name + " up")


@pytest.fixture
def s65():
    pm, bits, _, pairs, _ = TL.problem("S65")
    ctx, model = _open(pm, bits)
    yield ctx, model, pm, pairs
    ctx.close()


def test_pair_counts(s65):
    """1, 63, 64, 65 and 200 pairs; rows beyond the list stay untouched (65 sites: neighbouring rows share float4s)."""
    ctx, model, pm, pairs = s65
    _, _, _, _, wd, wu = TL.case("S65")
    for n in TL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        bd, bu = np.full((n + 3, pm.S), -7, np.float32), np.full((n + 3, pm.S), -7, np.float32)
        out = ctx.decode_pair_transitions(model, out=(bd, bu, None, None))
        assert out[0] is bd and out[1] is bu
        _assert_equal(bd[:n], wd[:n], f"{n} pairs down")
        _assert_equal(bu[:n], wu[:n], f"{n} pairs up")
        assert (bd[n:] == -7).all() and (bu[n:] == -7).all(), n


def test_slices_and_order_do_not_show(s65):
    ctx, model, pm, pairs = s65
    _, _, _, _, wd, wu = TL.case("S65")
    _upload(ctx, pm, pairs)  # four groups, the last of 8 pairs
    for slice_groups, n_slices in ((1, 4), (3, 2), (0, 1)):
        ctx.set_pair_transitions_slice(slice_groups)
        down, up = _rows(ctx, model)
        assert ctx.last_pair_transitions_slices() == n_slices
        _assert_equal(down, wd, f"slice {slice_groups} down")
        _assert_equal(up, wu, f"slice {slice_groups} up")
    perm = np.random.default_rng(3).permutation(len(pairs))
    _upload(ctx, pm, [pairs[i] for i in perm])
    down, up = _rows(ctx, model)
    _assert_equal(down, wd[perm], "permuted down")
    _assert_equal(up, wu[perm], "permuted up")
    only_up = ctx.decode_pair_transitions(model, out=(None, np.zeros_like(wu), None, None))
    assert only_up[0] is None
    _assert_equal(only_up[1], wu[perm], "up alone")


@pytest.fixture
def rich():
    pm, bits, _, pairs, wd, wu = TL.case("rich")
    assert len(pairs) == TL.RICH_PAIRS
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    yield ctx, model, pm, pairs, wd, wu
    ctx.close()


def test_chunk_lengths(rich, s65):
    """Chunks of 1, 2, 27, 699 and 700 sites: a chunk edge at t = 1 and at S - 1, a ragged last chunk, one chunk.  Then the
    65-site case, whose rows start at every phase of the output's float4s and share float4s with their neighbours, in
    chunks of 2, 3, 4, 7 and 64 sites: edges inside a float4 and on float4 boundaries, a ragged last chunk; in chunks of 3
    the rows beyond the list stay untouched."""
    ctx, model, pm, pairs, wd, wu = rich
    for C in TL.CHUNKS_RICH:
        ctx.set_chunk_sites(C)
        down, up = _rows(ctx, model)
        info = ctx.info()
        assert info["chunk_sites"] == C and info["max_chunks"] == -(-pm.S // C), (C, info)
        _assert_equal(down, wd, f"chunk {C} down")
        _assert_equal(up, wu, f"chunk {C} up")
    ctx, model, pm, pairs = s65
    _, _, _, _, wd, wu = TL.case("S65")
    _upload(ctx, pm, pairs)
    for C in TL.CHUNKS_S65:
        ctx.set_chunk_sites(C)
        down, up = _rows(ctx, model)
        info = ctx.info()
        assert info["chunk_sites"] == C and info["max_chunks"] == -(-pm.S // C), (C, info)
        _assert_equal(down, wd, f"65 sites, chunk {C} down")
        _assert_equal(up, wu, f"65 sites, chunk {C} up")
    ctx.set_chunk_sites(3)
    for n in TL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        bd, bu = np.full((n + 3, pm.S), -7, np.float32), np.full((n + 3, pm.S), -7, np.float32)
        ctx.decode_pair_transitions(model, out=(bd, bu, None, None))
        _assert_equal(bd[:n], wd[:n], f"65 sites, chunk 3, {n} pairs down")
        _assert_equal(bu[:n], wu[:n], f"65 sites, chunk 3, {n} pairs up")
        assert (bd[n:] == -7).all() and (bu[n:] == -7).all(), n


def test_workspace_limit_forces_chunks(rich):
    """The workspace is the sampling kernel's: two mebibytes hold two waves at the smallest slot, one mebibyte one; 600
    KiB and 16 KiB none: refused before any launch, and the context goes on working."""
    ctx, model, pm, pairs, wd, wu = rich
    for limit in TL.LIMITS_RICH_PLANNED:
        ctx.set_workspace_limit(limit)
        down, up = _rows(ctx, model)
        info = ctx.info()
        chunk, chunks, waves = TL.planned(pm.S, 69, 2, limit)
        assert (info["chunk_sites"], info["max_chunks"], info["n_slots"]) == (chunk, chunks, waves), (limit, info)
        assert chunks >= 2
        _assert_equal(down, wd, f"{limit} bytes of workspace, down")
        _assert_equal(up, wu, f"{limit} bytes of workspace, up")
    for limit in TL.LIMITS_RICH_REFUSED:
        ctx.set_workspace_limit(limit)
        bd, bu = np.full(wd.shape, -7, np.float32), np.full(wd.shape, -7, np.float32)
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_transitions(model, out=(bd, bu, None, None))
        assert ei.value.code == ENOMEM and "workspace limit too small" in str(ei.value)
        assert (bd == -7).all() and (bu == -7).all()
    ctx.set_workspace_limit(0)
    _assert_equal(_rows(ctx, model)[0], wd, "after a refusal")


def test_row_drain_straddles_rows(rich, monkeypatch):
    """Copies of 1000 bytes through the pinned buffers: every copy ends inside a 2800-byte row."""
    ctx, model, pm, pairs, wd, wu = rich
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", "1000")
    ctx.set_pair_transitions_slice(1)
    down, up = _rows(ctx, model)
    assert ctx.last_pair_transitions_slices() == 2
    _assert_equal(down, wd, "copies of 1000 bytes, down")
    _assert_equal(up, wu, "copies of 1000 bytes, up")


@pytest.mark.parametrize("key", sorted(TL.EDGES))
def test_bins(key):
    """One bin over the whole sequence, single-site bins, bins of 64 and 65 sites, edges at no multiple of four: the
    defined fp64 sums of the rows; a call for the bins alone gives the same cells; slices do not show."""
    pm, bits, _, pairs, wd, wu = TL.case("S200")
    edges = TL.EDGES[key]
    want_d, want_u = TL.bin_sums(wd, edges), TL.bin_sums(wu, edges)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    down, up, bin_d, bin_u = ctx.decode_pair_transitions(model, bin_edges=edges)
    _assert_equal(down, wd, "rows with bins, down")
    _assert_equal(up, wu, "rows with bins, up")
    _assert_equal(bin_d, want_d, key + " down")
    _assert_equal(bin_u, want_u, key + " up")
    ctx.set_pair_transitions_slice(1)
    none_d, none_u, only_d, only_u = ctx.decode_pair_transitions(model, bin_edges=edges, want_rows=False)
    assert none_d is None and none_u is None and ctx.last_pair_transitions_slices() == 2
    ctx.close()
    _assert_equal(only_d, want_d, key + " bins alone, down")
    _assert_equal(only_u, want_u, key + " bins alone, up")
    if key == "single":
        assert np.array_equal(bin_d, wd) and np.array_equal(bin_u, wu)


@pytest.mark.parametrize("case", E.SWEEP_CASES, ids=E.sweep_id)
def test_numeric_edges(case):
    """The edge models of the decode kernels (subnormal table entries and vectors, states at exactly +0 beside the ghost
    states, every state equal, identical and complementary haplotypes) at an exact and two padded members: all 96 pairs,
    two groups, bit for bit."""
    name, K, _ = case
    pm, bits, _, pairs, wd, wu = TL.edge_case(name, K)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    down, up = _rows(ctx, model)
    assert ctx.last_kernel() == expected_member(K)
    ctx.close()
    _assert_equal(down, wd, E.sweep_id(case) + " down")
    _assert_equal(up, wu, E.sweep_id(case) + " up")


def test_one_state_holds_everything():
    """Sites where state 0 / the top state holds all of a pair's mass (a padded member): the moves that cannot happen
    have probability exactly 0.f."""
    pm, bits, _, pairs, wd, wu, het, (lo, hi) = TL.dominant_case()
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    down, up = _rows(ctx, model)
    ctx.close()
    _assert_equal(down, wd, "down")
    _assert_equal(up, wu, "up")
    assert not up[het[:, 0], lo].any() and not down[het[:, 1], hi].any()


def test_zero_and_nan_sums():
    """A zero scaling sum somewhere: the call ends without error, the values are what IEEE gives."""
    pm, bits, _, pairs, wd, wu, bad = TL.zero_sum_case()
    assert bad.any() and not bad.all()
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    down, up = _rows(ctx, model)
    ctx.close()
    assert np.isnan(wd[bad]).any()
    _assert_equal(down, wd, "down")
    _assert_equal(up, wu, "up")
    assert np.isfinite(down[~bad]).all()


def test_errors(s65):
    """Every FSMC_EINVAL, nothing touched and nothing launched, each followed by a good call."""
    ctx, model, pm, pairs = s65
    _, _, _, _, wd, wu = TL.case("S65")
    _upload(ctx, pm, pairs)
    n = len(pairs)

    def good():
        _assert_equal(_rows(ctx, model)[0], wd, "after an error")

    def refused(text, mdl=None, edges=None, raw=None):
        bufs = [np.full((n, pm.S), -7, np.float32) for _ in range(2)]
        if edges is not None:  # (a cell buffer large enough whatever the edges say)
            e = np.array(edges, np.int32)
            raw = (bufs[0].ctypes.data, bufs[1].ctypes.data, e.ctypes.data, len(e) - 1, cells.ctypes.data, None)
        if raw is not None:  # (what the wrapper never passes: the symbol itself)
            rc = ctx._L.fsmc_decode_pair_transitions(ctx._h, (mdl or model)._h, *raw)
            msg = (ctx._L.fsmc_last_error(ctx._h) or b"").decode()
            assert rc == EINVAL and text in msg, (rc, msg)
        else:
            with pytest.raises(capi.FsmcError) as ei:
                ctx.decode_pair_transitions(mdl or model, out=(bufs[0], bufs[1], None, None))
            assert ei.value.code == EINVAL and text in str(ei.value), (text, str(ei.value))
        assert all((b == -7).all() for b in bufs) and (cells == -7).all()
        good()

    cells = np.full((n, 4), -7, np.float32)
    good()
    refused("at least one output", raw=(None, None, None, 0, None, None))
    refused("need bin edges", raw=(None, None, None, 2, cells.ctypes.data, None))
    refused("one bin at least", edges=[5])
    refused("strictly ascending", edges=[0, 10, 10])
    refused("strictly ascending", edges=[10, 5, 20])
    refused("[0, sites]", edges=[-1, 10])
    refused("[0, sites]", edges=[0, pm.S + 1])
    groups = capi.whole_sequence_groups(n, pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(pairs), groups)
    buf = np.full(wd.shape, -7, np.float32)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_transitions(model, out=(buf, None, None, None))
    assert ei.value.code == EINVAL and "whole-sequence" in str(ei.value) and (buf == -7).all()
    _upload(ctx, pm, pairs)
    good()
    wide, wide_bits, _ = LL._problem(130, 65, seed=100 + 69 + 65)
    assert np.array_equal(wide_bits, TL.problem("S65")[1])
    refused("more than 128 states", mdl=ctx.create_model(wide))


def test_sequence_mode_is_refused():
    pm, bits, _, pairs, _, _ = LL.case("seq69")
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    buf = np.full((len(pairs), pm.S), -7, np.float32)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_transitions(model, out=(buf, None, None, None))
    assert ei.value.code == EINVAL and "sequence-mode" in str(ei.value) and (buf == -7).all()
    assert ctx.decode_pair_loglik(model)[0].shape == (len(pairs),)  # (the context is fine)
    ctx.close()


# ---------------------------------------------------------------- the product path: ASMC.decodePairTransitions

EDGES_700 = [5, 70, 71, 100, 400, 699]


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairTransitions on a synthetic cohort's files, by index and by id, in one flush and in flushes of 128
    pairs (200 pairs: two flushes): the restatement's arrays, equal to two separate calls concatenated; every other
    field of the results is empty, and decodePairs leaves the new fields empty."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, _, _, _, _ = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    pm, _, _, _ = LL.cohort_problem()
    assert np.array_equal(np.array(api.Data(p).geneticPositions, np.float32), pm.gen)  # (the restatement's model)
    wd, wu = TL.cohort_transitions()
    want_bd, want_bu = TL.bin_sums(wd, EDGES_700), TL.bin_sums(wu, EDGES_700)

    asmc.decodePairTransitions(a, b, site_bins=EDGES_700)
    res = asmc.get_copy_of_results()
    _assert_equal(np.array(res.per_pair_down_probabilities), wd, "down")
    _assert_equal(np.array(res.per_pair_up_probabilities), wu, "up")
    _assert_equal(np.array(res.bin_expected_downs), want_bd, "bin downs")
    _assert_equal(np.array(res.bin_expected_ups), want_bu, "bin ups")
    assert list(np.array(res.bin_edges)) == EDGES_700
    assert np.array(res.per_pair_MAPs).size == 0 and np.array(res.bin_mean_posterior_means).size == 0
    assert np.array(res.per_pair_sampled_states).size == 0
    idx = res.per_pair_indices
    assert [i[0] for i in idx] == a and [i[2] for i in idx] == b

    # by id, the bins alone
    asmc.decodePairTransitions([i[1] for i in idx], [i[3] for i in idx], rows=False, site_bins=EDGES_700)
    res = asmc.get_copy_of_results()
    assert np.array(res.per_pair_down_probabilities).size == 0
    _assert_equal(np.array(res.bin_expected_downs), want_bd, "bin downs by id")
    _assert_equal(np.array(res.bin_expected_ups), want_bu, "bin ups by id")

    # two separate calls concatenated
    halves = []
    for lo, hi in ((0, 128), (128, len(a))):
        asmc.decodePairTransitions(a[lo:hi], b[lo:hi])
        r = asmc.get_copy_of_results()
        halves.append((np.array(r.per_pair_down_probabilities), np.array(r.per_pair_up_probabilities)))
        assert np.array(r.bin_expected_downs).size == 0 and np.array(r.bin_edges).size == 0
    _assert_equal(np.concatenate([h[0] for h in halves]), wd, "two calls, down")
    _assert_equal(np.concatenate([h[1] for h in halves]), wu, "two calls, up")

    with pytest.raises(RuntimeError, match="at least one output"):
        asmc.decodePairTransitions(a[:3], b[:3], rows=False)
    with pytest.raises(RuntimeError, match="strictly ascending"):
        asmc.decodePairTransitions(a[:3], b[:3], site_bins=[0, 5, 5])
    asmc.decodePairs(a[:3], b[:3], per_pair_MAPs=True)
    res = asmc.get_copy_of_results()
    for field in (res.per_pair_down_probabilities, res.per_pair_up_probabilities, res.bin_expected_downs,
                  res.bin_expected_ups):
        empty = np.array(field)
        assert empty.size == 0 and empty.ndim == 2 and empty.dtype == np.float32
    assert np.array(res.per_pair_MAPs).shape == (3, pm.S)

    # the HMM's setter: the same request
    hmm = api.HMM(api.Data(p), p)
    hmm.setTransitionProbabilities(True, EDGES_700)
    with pytest.raises(RuntimeError, match=r"\[0, sites\]"):
        hmm.setTransitionProbabilities(False, [0, pm.S + 1])
    hmm.setTransitionProbabilities(False)
