"""fsmc_decode_pair_viterbi on the GPU: per pair the most probable joint state sequence and its probability as mantissa
and exponent.  States, mantissas and exponents are np.array_equal to the numpy restatement of
tests/pair_viterbi_lists.py (tests/test_pair_viterbi_lists.py shows on the CPU that the restatement's paths are the dense
fp64 Viterbi's and what the inputs reach).  The tie cases (edge_models.dyadic_ties) pin the five comparisons of the
contract: the same CPU tests show that each of them, flipped alone, changes a path of every tie case.  The edge models
(edge_models.SWEEP_CASES) are the numeric edges the decode kernels are tested at."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
import pair_viterbi_lists as VL
from conftest import expected_member
from fastsmc_amd import api, capi
from pair_common import (pairs_array as _pairs_array, upload as _upload, cohort_files as _cohort_files, params as _params,
                         cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu

INT_MIN = np.iinfo(np.int32).min
NAMES = ("states", "mant", "expo")


def _open(pm, bits):
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    return ctx, model


def _want(case):
    states, sums, last = case[4:7]
    return (states,) + VL.expected(sums, last)


def _assert_equal(got, want, msg=""):
    assert len(got) == len(want) == 3
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (name, msg)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, msg, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{name} {msg}: {int((g != w).sum())} of {g.size} values differ"


def _sentinels(n, S):
    """(states, mant, expo) prefilled with values no result has: 255, NaN and INT_MIN."""
    return np.full((n, S), 255, np.uint8), np.full(n, np.nan), np.full(n, INT_MIN, np.int32)


def _untouched(a):
    if a.dtype == np.uint8:
        return bool((a == 255).all())
    return bool(np.isnan(a).all()) if a.dtype == np.float64 else bool((a == INT_MIN).all())


MODELS = [n for n in VL.CASES if n.startswith("K")]
SITES = ["S1", "S2", "S63", "S64", "S65", "S200"]


@pytest.mark.parametrize("name", MODELS + SITES + ["dense40"])
def test_models_and_sites(name):
    """The members of the family (K = 2 ... 128, exact and padded: ghost states are never chosen) at 129 sites, 1 ... 200
    sites at K = 69, and the K = 40 case on the dense map, whose paths move every few sites."""
    case = VL.case(name)
    pm, bits, pairs = case[0], case[1], case[3]
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_viterbi(model)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_viterbi_slices() == 1
    info = ctx.info()
    assert info["chunk_sites"] == pm.S and info["max_chunks"] == 1
    ctx.close()
    assert (got[0] < pm.K).all()
    _assert_equal(got, _want(case), name)


@pytest.mark.parametrize("name", list(VL.TIE_CASES))
def test_tie_rules(name):
    """States in blocks of bitwise-equal values: every comparison of the step and the final argmax meet equal operands
    (thousands of times a case) and each one, taken the other way, changes a path.  Exact members, padded ones -- with
    the two top states at +0 like the ghosts above them in the `dead` cases --, the largest and the two smallest."""
    case = VL.case(name)
    pm, bits, pairs = case[0], case[1], case[3]
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_viterbi(model)
    assert ctx.last_kernel() == expected_member(pm.K)
    info = ctx.info()
    assert info["chunk_sites"] == pm.S and info["max_chunks"] == 1
    ctx.close()
    assert (got[0] < pm.K).all()
    _assert_equal(got, _want(case), name)


@pytest.fixture
def ties300():
    case = VL.case(VL.TIE_CHUNKED)
    ctx, model = _open(case[0], case[1])
    _upload(ctx, case[0], case[3])
    yield ctx, model, case[0], _want(case)
    ctx.close()


def test_tie_rules_in_chunks(ties300):
    """The 300-site tie case in chunks of 16 sites (a last chunk of 12), of 150 (two chunks) and automatic: sweep 2
    rebuilds the back-pointers from a checkpoint and breaks the same ties the same way, and the traceback hands over
    between chunks while the paths move through them."""
    ctx, model, pm, want = ties300
    for C in VL.CHUNKS_TIES:
        ctx.set_chunk_sites(C)
        got = ctx.decode_pair_viterbi(model)
        info = ctx.info()
        chunk = C if C else pm.S
        assert info["chunk_sites"] == chunk and info["max_chunks"] == -(-pm.S // chunk), (C, info)
        _assert_equal(got, want, f"chunk {C}")


def test_tie_rules_under_a_workspace_limit(ties300):
    """A megabyte of workspace for two waves' 1.4 MB of back-pointers each: the planner's four chunks of 75 sites."""
    ctx, model, pm, want = ties300
    ctx.set_workspace_limit(VL.LIMIT_TIES)
    got = ctx.decode_pair_viterbi(model)
    info = ctx.info()
    chunk, chunks, waves = VL.planned(pm.S, 69, 2, VL.LIMIT_TIES)
    assert (info["chunk_sites"], info["max_chunks"], info["n_slots"]) == (chunk, chunks, waves), info
    assert chunks >= 2
    _assert_equal(got, want, "a megabyte of workspace")


def test_tie_rules_probabilities_alone_and_the_likelihood():
    """Without states the probabilities take the same final tie; and on the same context one path stays below the sum
    over all paths, which the forward kernel gives."""
    case = VL.case("ties-K69")
    pm, bits, pairs = case[0], case[1], case[3]
    want = _want(case)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_viterbi(model, want_states=False)
    _assert_equal(got, (None,) + want[1:], "probabilities alone")
    lm, le, _, _ = ctx.decode_pair_loglik(model)
    ctx.close()
    lp, ll = capi.log_likelihood(got[1], got[2]), capi.log_likelihood(lm, le)
    assert (lp <= ll).all()


@pytest.mark.parametrize("case", E.SWEEP_CASES, ids=E.sweep_id)
def test_numeric_edges(case):
    """The edge models of the decode kernels (subnormal table entries and vectors, states at exactly +0 beside the ghost
    states, every state equal, identical and complementary haplotypes) at an exact and two padded members: all 96 pairs,
    two groups, bit for bit -- tests/test_pair_viterbi_lists.py shows that every pair has a finite, non-zero probability."""
    name, K, _ = case
    pm, bits, _, pairs, states, sums, last, _ = VL.edge_case(name, K)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_viterbi(model)
    assert ctx.last_kernel() == expected_member(K)
    ctx.close()
    assert (got[0] < K).all()
    _assert_equal(got, (states,) + VL.expected(sums, last), E.sweep_id(case))


@pytest.fixture
def s65():
    case = VL.case("S65")
    ctx, model = _open(case[0], case[1])
    yield ctx, model, case[0], case[3], _want(case)
    ctx.close()


def test_pair_counts(s65):
    """1, 63, 64, 65 and 200 pairs: a lone lane, a group one short, a full group, one lane in a second group, four
    groups; rows beyond the list stay untouched (65 sites: rows of neighbouring pairs share dwords)."""
    ctx, model, pm, pairs, want = s65
    for n in VL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        bufs = _sentinels(n + 3, pm.S)
        got = ctx.decode_pair_viterbi(model, out=bufs)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g[:n], w[:n]), (n, name)
            assert _untouched(g[n:]), (n, name)


def test_more_groups_than_waves(s65):
    """A list of more groups than the launch has waves, built from repeats of the 200 distinct pairs: every wave pulls
    several groups from the queue and uses its workspace again."""
    ctx, model, pm, pairs, want = s65
    n_groups = ctx.info()["n_cu"] * 8 + 37
    idx = (np.arange(n_groups * 64 - 5) * 7) % len(pairs)  # (7 and 200 are coprime: every lane sees every pair)
    _upload(ctx, pm, [pairs[i] for i in idx])
    got = ctx.decode_pair_viterbi(model)
    assert ctx.last_pair_viterbi_slices() == 1
    assert 0 < ctx.info()["n_slots"] < n_groups
    _assert_equal(got, tuple(w[idx] for w in want), f"{n_groups} groups")


def test_slices_do_not_show(s65):
    ctx, model, pm, pairs, want = s65
    _upload(ctx, pm, pairs)  # four groups, the last of 8 pairs
    for slice_groups, n_slices in ((1, 4), (2, 2), (0, 1)):
        ctx.set_pair_viterbi_slice(slice_groups)
        got = ctx.decode_pair_viterbi(model)
        assert ctx.last_pair_viterbi_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


@pytest.fixture
def rich():
    case = VL.case("rich")
    ctx, model = _open(case[0], case[1])
    _upload(ctx, case[0], case[3])
    yield ctx, model, case[0], case[3], _want(case)
    ctx.close()


def test_chunk_lengths(rich, s65):
    """Chunks of 16, 64, 150 (does not divide 700), 700 sites and automatic: the same bytes throughout.  Then the 65-site
    case, whose rows start at every phase of the output's dwords and share dwords with their neighbours, in chunks of 2, 3,
    4, 7 and 64 sites: edges inside a dword and on dword boundaries, a chunk that ends at t = 1, a ragged last chunk; in
    chunks of 3 the rows beyond the list stay untouched."""
    ctx, model, pm, pairs, want = rich
    for C in VL.CHUNKS_RICH:
        ctx.set_chunk_sites(C)
        got = ctx.decode_pair_viterbi(model)
        info = ctx.info()
        chunk = C if C else pm.S
        assert info["chunk_sites"] == chunk and info["max_chunks"] == -(-pm.S // chunk), (C, info)
        _assert_equal(got, want, f"chunk {C}")
    ctx, model, pm, pairs, want = s65
    _upload(ctx, pm, pairs)
    for C in VL.CHUNKS_S65:
        ctx.set_chunk_sites(C)
        got = ctx.decode_pair_viterbi(model)
        info = ctx.info()
        assert info["chunk_sites"] == C and info["max_chunks"] == -(-pm.S // C), (C, info)
        _assert_equal(got, want, f"65 sites, chunk {C}")
    ctx.set_chunk_sites(3)
    for n in VL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        got = ctx.decode_pair_viterbi(model, out=_sentinels(n + 3, pm.S))
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g[:n], w[:n]), (n, name)
            assert _untouched(g[n:]), (n, name)


def test_workspace_limit_forces_chunks(rich):
    """A megabyte of workspace holds 3.2 MB of back-pointers a wave only in chunks, 600 KiB hold one wave's smallest slot
    (0.5 MB) once: the plan is the one pair_viterbi_lists.planned states (tests/test_pair_viterbi_lists.py shows that
    paths change state across these chunks' boundaries); then 16 KiB, refused for states and enough for the
    probabilities, which need one row."""
    ctx, model, pm, pairs, want = rich
    for limit in VL.LIMITS_RICH:
        ctx.set_workspace_limit(limit)
        got = ctx.decode_pair_viterbi(model)
        info = ctx.info()
        chunk, chunks, waves = VL.planned(pm.S, 69, 2, limit)
        assert (info["chunk_sites"], info["max_chunks"], info["n_slots"]) == (chunk, chunks, waves), (limit, info)
        assert chunks >= 2
        _assert_equal(got, want, f"{limit} bytes of workspace")
    ctx.set_workspace_limit(16 << 10)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_viterbi(model)
    assert ei.value.code == -4 and "workspace limit too small" in str(ei.value)  # FSMC_ENOMEM
    _assert_equal(ctx.decode_pair_viterbi(model, want_states=False), (None,) + want[1:], "probabilities, 16 KiB")


def test_row_drain_straddles_rows(rich, monkeypatch):
    """Copies of 1000 bytes through the pinned buffers: every copy ends inside a 700-byte row."""
    ctx, model, pm, pairs, want = rich
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", "1000")
    _assert_equal(ctx.decode_pair_viterbi(model), want, "copies of 1000 bytes")
    ctx.set_pair_viterbi_slice(1)
    _assert_equal(ctx.decode_pair_viterbi(model), want, "copies of 1000 bytes, slices of a group")
    assert ctx.last_pair_viterbi_slices() == 2


def test_probabilities_alone_and_states_alone(rich):
    ctx, model, pm, pairs, want = rich
    _assert_equal(ctx.decode_pair_viterbi(model, want_states=False), (None,) + want[1:], "null states")
    ctx.set_chunk_sites(64)
    _assert_equal(ctx.decode_pair_viterbi(model, want_states=False), (None,) + want[1:], "null states, chunk 64")
    _assert_equal(ctx.decode_pair_viterbi(model, want_prob=False), want[:1] + (None, None), "states alone")


def test_zero_and_nan_sums():
    """A zero scaling sum somewhere: the pair's mantissa (0 or NaN) and exponent are the restatement's, its states only lie
    in [0, K); the other pairs of its group are exact."""
    pm, bits, _, pairs, states, sums, last = VL.zero_sum_viterbi()
    mant, expo = VL.expected(sums, last)
    bad = (mant == 0) | ~np.isfinite(mant)
    assert bad.any() and not bad.all()
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_viterbi(model)
    ctx.close()
    assert np.array_equal(got[1], mant, equal_nan=True) and np.array_equal(got[2], expo)
    assert (got[0] < pm.K).all()
    assert np.array_equal(got[0][~bad], states[~bad])
    lp = capi.log_likelihood(got[1], got[2])
    assert np.isfinite(lp[~bad]).all() and not np.isfinite(lp[bad]).any()


def test_below_the_likelihood(s65):
    """One path against the sum over all paths, on the same context."""
    ctx, model, pm, pairs, want = s65
    _upload(ctx, pm, pairs)
    _, mant, expo = ctx.decode_pair_viterbi(model, want_states=False)
    lm, le, _, _ = ctx.decode_pair_loglik(model)
    lp, ll = capi.log_likelihood(mant, expo), capi.log_likelihood(lm, le)
    assert (lp <= ll).all() and (lp < ll).any()
    _assert_equal(ctx.decode_pair_viterbi(model), want, "after the forward kernel")


def test_errors(s65):
    """Every FSMC_EINVAL, nothing touched, each followed by a good call."""
    ctx, model, pm, pairs, want = s65
    _upload(ctx, pm, pairs)

    def good():
        _assert_equal(ctx.decode_pair_viterbi(model), want, "after an error")

    def refused(text, keep=(0, 1, 2), mdl=None):
        bufs = _sentinels(len(pairs), pm.S)
        out = tuple(b if i in keep else None for i, b in enumerate(bufs))
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_viterbi(mdl or model, out=out)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert all(_untouched(b) for b in bufs)
        good()

    good()
    for keep in ((1,), (2,), (0, 1), (0, 2)):  # a mantissa without its exponent or the reverse
        refused("come together", keep=keep)
    refused("at least one output", keep=())
    assert ctx.last_pair_viterbi_slices() == 1  # (of the good call)
    groups = capi.whole_sequence_groups(len(pairs), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(pairs), groups)
    bufs = _sentinels(len(pairs), pm.S)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_viterbi(model, out=bufs)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value) and all(_untouched(b) for b in bufs)
    _upload(ctx, pm, pairs)
    good()
    # a model of more than 128 states on the same haplotypes: the wave-group family has no Viterbi kernel
    wide, wide_bits, _ = LL._problem(130, 65, seed=100 + 69 + 65)
    assert np.array_equal(wide_bits, VL.case("S65")[1])
    refused("more than 128 states", mdl=ctx.create_model(wide))


def test_sequence_mode_is_refused():
    pm, bits, _, pairs, _, _ = LL.case("seq69")
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    bufs = _sentinels(len(pairs), pm.S)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_viterbi(model, out=bufs)
    assert ei.value.code == -1 and "sequence-mode" in str(ei.value) and all(_untouched(b) for b in bufs)
    assert ctx.decode_pair_loglik(model)[0].shape == (len(pairs),)  # (the context is fine)
    ctx.close()


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

FIELDS = ("per_pair_viterbi_states", "per_pair_viterbi_mantissas", "per_pair_viterbi_exponents")


def _within_4_ulp(got, mant, expo):
    want = np.log(mant) + expo * np.log(2)
    return bool((np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all())


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, viterbi_paths=True) on a synthetic cohort's files, in one flush and in flushes of 128 pairs,
    beside per_pair_MAPs and log_likelihoods, twice in a row: states, mantissas and exponents are the restatement's, the
    logarithms log(m) + e ln 2 to 4 ulp (two implementations of log and one add); the other outputs are what they are
    without the request; without the keyword every new field is empty."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, _, _, _, _ = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    pm = VL.cohort_problem()[0]
    assert np.array_equal(np.array(api.Data(p).geneticPositions, np.float32), pm.gen)  # (the restatement's model)
    states, sums, last = VL.cohort_viterbi()
    want = (states,) + VL.expected(sums, last)

    def three(res):
        return tuple(np.array(getattr(res, f)) for f in FIELDS)

    asmc.decodePairs(a, b, per_pair_MAPs=True, log_likelihoods=True)
    res = asmc.get_copy_of_results()
    maps, lm = np.array(res.per_pair_MAPs), np.array(res.per_pair_likelihood_mantissas)
    assert all(g.size == 0 for g in three(res)) and np.array(res.per_pair_viterbi_log_probabilities).size == 0

    for _ in range(2):  # two calls in a row
        asmc.decodePairs(a, b, per_pair_MAPs=True, log_likelihoods=True, viterbi_paths=True)
        res = asmc.get_copy_of_results()
        got = three(res)
        for name, g, w in zip(FIELDS, got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
        lp = np.array(res.per_pair_viterbi_log_probabilities)
        assert lp.dtype == np.float64 and lp.shape == (len(pairs),) and _within_4_ulp(lp, got[1], got[2])
        assert np.array_equal(np.array(res.per_pair_MAPs), maps)
        assert np.array_equal(np.array(res.per_pair_likelihood_mantissas), lm)
        assert (lp <= np.array(res.per_pair_log_likelihoods)).all()

    asmc.decodePairs(a, b, viterbi_paths=True)
    res = asmc.get_copy_of_results()
    assert np.array_equal(three(res)[0], want[0]) and np.array(res.per_pair_MAPs).size == 0
    starts, ends, st = api.state_runs(three(res)[0][0])
    assert starts[0] == 0 and ends[-1] == pm.S and np.array_equal(starts[1:], ends[:-1]) and (st[1:] != st[:-1]).all()


# ---------------------------------------------------------------- the host's own check: PairOutputs::check

SEQUENCE_TEXT = "per-pair Viterbi paths: no Viterbi kernel for a sequence-mode model"
WIDE_TEXT = r"per-pair Viterbi paths: no Viterbi kernel for a model of more than 128 states \(130\)"
A, B = [1, 2, 3, 10, 40, 63, 7], [2, 3, 4, 11, 41, 0, 9]


def _refused_then_good(p, text):
    """ASMC.decodePairs(viterbi_paths=True) and HMM.setStoreViterbiPaths(True) raise RuntimeError with the ABI's message
    before anything is decoded; the request stays what it was (the results of the call before are still there, the
    same call gives them again, no Viterbi field is filled) and the objects go on working."""
    asmc = api.ASMC(p)
    asmc.decodePairs(A, B, per_pair_posterior_means=True, per_pair_MAPs=True)
    maps = np.array(asmc.get_copy_of_results().per_pair_MAPs)
    assert maps.shape[0] == len(A) and maps.any()
    for extra in ({}, {"per_pair_posterior_means": True, "per_pair_MAPs": True}):  # (alone, and beside other outputs)
        with pytest.raises(RuntimeError, match=text):
            asmc.decodePairs(A, B, viterbi_paths=True, **extra)
        res = asmc.get_copy_of_results()
        assert np.array_equal(np.array(res.per_pair_MAPs), maps)
        assert all(np.array(getattr(res, f)).size == 0 for f in FIELDS)
    asmc.decodePairs(A, B, per_pair_posterior_means=True, per_pair_MAPs=True)
    res = asmc.get_copy_of_results()
    assert np.array_equal(np.array(res.per_pair_MAPs), maps)
    assert all(np.array(getattr(res, f)).size == 0 for f in FIELDS)

    hmm = api.HMM(api.Data(p), p)
    hmm.setStorePerPairPosteriorMean(True)
    with pytest.raises(RuntimeError, match=text):
        hmm.setStoreViterbiPaths(True)
    hmm.setStoreViterbiPaths(False)  # (nothing to refuse)
    hmm.setStorePerPairPosteriorMean(True)  # (a good setter follows)
    res = hmm.getDecodePairsReturnStruct()
    assert all(np.array(getattr(res, f)).size == 0 for f in FIELDS)


def test_host_check_refuses_sequence_mode(tmp_path, seq_problem):
    from fastsmc_amd import synth

    root = str(tmp_path / "seq")
    synth.write_haps_files(root, seq_problem["haps"], fastsmc_map=False)
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", seq_problem["tables"])
    p = api.DecodingParams(root, root + ".decodingQuantities.gz", decodingModeString="sequence",
                           doPerPairPosteriorMean=True)
    p.doPerPairMAP = True
    p.useKnownSeed = True
    assert p.decodingSequence
    _refused_then_good(p, SEQUENCE_TEXT)


def test_host_check_refuses_more_than_128_states(tmp_path):
    from fastsmc_amd import synth

    root = str(tmp_path / "wide")
    synth.write_haps_files(root, synth.make_haps(64, 100, seed=31, cm_per_mb=25.0, switch_per_cm=0.6), fastsmc_map=False)
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", synth.make_model_tables(130))
    p = _params(root)
    p.doPerPairMAP = True
    assert not p.decodingSequence
    _refused_then_good(p, WIDE_TEXT)


def test_host_accepts_128_states_in_array_mode(tmp_path):
    """The other side of both limits: 128 states, array mode -- the path through the files is the C ABI's."""
    from fastsmc_amd import synth

    root = str(tmp_path / "k128")
    synth.write_haps_files(root, synth.make_haps(64, 200, seed=31, cm_per_mb=25.0, switch_per_cm=0.6), fastsmc_map=False)
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", synth.make_model_tables(128))
    asmc = api.ASMC(_params(root))
    asmc.decodePairs(A, B, viterbi_paths=True, log_likelihoods=True)
    res = asmc.get_copy_of_results()
    states = np.array(res.per_pair_viterbi_states)
    assert states.shape == (len(A), 200) and states.dtype == np.uint8 and (states < 128).all()
    assert (np.array(res.per_pair_viterbi_log_probabilities) <= np.array(res.per_pair_log_likelihoods)).all()
