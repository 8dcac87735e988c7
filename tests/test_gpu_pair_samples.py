"""fsmc_decode_pair_samples on the GPU: per pair, state sequences drawn from the joint posterior over sequences (forward
filtering with backward sampling).  Every array is np.array_equal to the numpy restatement of tests/pair_sample_lists.py;
tests/test_pair_sample_lists.py shows on the CPU that the restatement's law is the exact path posterior of a tiny model,
that its marginals are the oracle's at working size, and what the inputs below reach.  The edge models
(edge_models.SWEEP_CASES) are the numeric edges the decode kernels are tested at."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
import pair_sample_lists as SL
from conftest import expected_member
from fastsmc_amd import api, capi
from pair_common import (pairs_array as _pairs_array, upload as _upload, cohort_files as _cohort_files, params as _params,
                         cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu


def _open(pm, bits):
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    return ctx, model


def _assert_equal(got, want, msg=""):
    assert got.dtype == np.uint8 and got.shape == want.shape, (msg, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), f"{msg}: {int((got != want).sum())} of {got.size} states differ"


MODELS = [n for n in SL.CASES if n.startswith("K")]
SITES = ["S1", "S2", "S3", "S4", "S5", "S63", "S64", "S65", "S200"]


@pytest.mark.parametrize("name", MODELS + SITES)
def test_models_and_sites(name):
    """The members of the family (K = 2 ... 128, exact and padded: ghost states are never chosen) at 129 sites and 1 ...
    200 sites at K = 69, three samples a pair."""
    pm, bits, _, pairs, want = SL.case(name, first=70)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_samples_slices() == 1
    info = ctx.info()
    assert info["chunk_sites"] == pm.S and info["max_chunks"] == 1
    ctx.close()
    assert (got < pm.K).all()
    _assert_equal(got, want, name)


@pytest.fixture
def s65():
    pm, bits, folded, pairs, alpha = SL.problem("S65")
    ctx, model = _open(pm, bits)
    yield ctx, model, pm, pairs
    ctx.close()


def test_pair_counts(s65):
    """1, 63, 64, 65 and 200 pairs: a lone lane, a group one short, a full group, one lane in a second group, four
    groups; rows beyond the list stay untouched (65 sites: neighbouring rows share dwords)."""
    ctx, model, pm, pairs = s65
    want = SL.case("S65")[4]
    for n in SL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        buf = np.full((n + 3, SL.N_MODELS, pm.S), 255, np.uint8)
        got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS, out=buf)
        assert got is buf
        _assert_equal(got[:n], want[:n], f"{n} pairs")
        assert (got[n:] == 255).all(), n


def test_more_groups_than_waves(s65):
    """A list of more groups than the launch has waves, built from repeats of the 200 distinct pairs: every wave pulls
    several groups from the queue and uses its workspace and its samples' dwords again; a pair gets the same row
    wherever it stands."""
    ctx, model, pm, pairs = s65
    want = SL.case("S65", n=1)[4]
    n_groups = ctx.info()["n_cu"] * 8 + 37
    idx = (np.arange(n_groups * 64 - 5) * 7) % len(pairs)  # (7 and 200 are coprime: every lane sees every pair)
    _upload(ctx, pm, [pairs[i] for i in idx])
    got = ctx.decode_pair_samples(model, 1, SL.SEED_MODELS)
    assert ctx.last_pair_samples_slices() == 1
    assert 0 < ctx.info()["n_slots"] < n_groups
    _assert_equal(got, want[idx], f"{n_groups} groups")


@pytest.mark.parametrize("n", SL.N_COUNTS)
def test_sample_counts(s65, n):
    """1, 2, 33 and 64 samples a pair: sample r is the same in each."""
    ctx, model, pm, pairs = s65
    want = SL.case("S65", n=n, first=70)[4]
    _upload(ctx, pm, pairs[:70])
    _assert_equal(ctx.decode_pair_samples(model, n, SL.SEED_MODELS), want, f"{n} samples")
    if n == 64:
        assert np.array_equal(want[:, :3], SL.case("S65")[4][:70])


@pytest.mark.parametrize("seed", SL.SEEDS)
def test_seeds(s65, seed):
    ctx, model, pm, pairs = s65
    want = SL.case("S65", seed=seed, first=70)[4]
    _upload(ctx, pm, pairs[:70])
    _assert_equal(ctx.decode_pair_samples(model, SL.N_MODELS, seed), want, f"seed {seed}")
    assert not np.array_equal(want, SL.case("S65")[4][:70])


def test_slices_do_not_show(s65):
    ctx, model, pm, pairs = s65
    want = SL.case("S65")[4]
    _upload(ctx, pm, pairs)  # four groups, the last of 8 pairs
    for slice_groups, n_slices in ((1, 4), (2, 2), (0, 1)):
        ctx.set_pair_samples_slice(slice_groups)
        got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
        assert ctx.last_pair_samples_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


def test_order_repeats_and_direction(s65):
    """The list reversed gives the rows permuted; a pair listed twice gets the same rows; (a, b) and (b, a) see the same
    observations and are different streams."""
    ctx, model, pm, pairs = s65
    want = SL.case("S65")[4]
    _upload(ctx, pm, pairs[::-1])
    _assert_equal(ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS), want[::-1], "reversed")
    twice = [pairs[3], pairs[100], pairs[3]] + list(pairs[:70]) + [pairs[100]]
    _upload(ctx, pm, twice)
    got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
    _assert_equal(got, want[[3, 100, 3] + list(range(70)) + [100]], "listed twice")
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[-1])
    swapped = [(b, a) for a, b in pairs[:70]]
    _upload(ctx, pm, swapped)
    got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
    _assert_equal(got, SL.sample(pm, None, swapped, SL.N_MODELS, SL.SEED_MODELS, alpha=SL.problem("S65")[4][:, :, :70]),
                  "swapped")
    assert not np.array_equal(got, want[:70])


@pytest.fixture
def rich():
    pm, bits, _, pairs, want = SL.case("rich", n=SL.RICH_N)
    assert len(pairs) == SL.RICH_PAIRS
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    yield ctx, model, pm, pairs, want
    ctx.close()


def test_chunk_lengths(rich, s65):
    """Chunks of 16, 64, 150 (does not divide 700), 700 sites and automatic: the same bytes throughout.  Then the 65-site
    case, whose rows start at every phase of the output's dwords and share dwords with their neighbours, in chunks of 2, 3,
    4, 7 and 64 sites: edges inside a dword and on dword boundaries, a chunk that ends at t = 1, a ragged last chunk
    (tests/test_pair_sample_lists.py shows that samples change state across every one of these edges); in chunks of 3 the
    rows beyond the list stay untouched."""
    ctx, model, pm, pairs, want = rich
    for C in SL.CHUNKS_RICH:
        ctx.set_chunk_sites(C)
        got = ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS)
        info = ctx.info()
        chunk = C if C else pm.S
        assert info["chunk_sites"] == chunk and info["max_chunks"] == -(-pm.S // chunk), (C, info)
        _assert_equal(got, want, f"chunk {C}")
    ctx, model, pm, pairs = s65
    want = SL.case("S65")[4]
    _upload(ctx, pm, pairs)
    for C in SL.CHUNKS_S65:
        ctx.set_chunk_sites(C)
        got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
        info = ctx.info()
        assert info["chunk_sites"] == C and info["max_chunks"] == -(-pm.S // C), (C, info)
        _assert_equal(got, want, f"65 sites, chunk {C}")
    ctx.set_chunk_sites(3)
    for n in SL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        buf = np.full((n + 3, SL.N_MODELS, pm.S), 255, np.uint8)
        got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS, out=buf)
        _assert_equal(got[:n], want[:n], f"65 sites, chunk 3, {n} pairs")
        assert (got[n:] == 255).all(), n


def test_workspace_limit_forces_chunks(rich):
    """Two mebibytes of workspace hold two waves only at the smallest slot, one mebibyte holds one: the plan is the one
    pair_sample_lists.planned states (tests/test_pair_sample_lists.py shows that samples change state across these chunks'
    boundaries).  600 KiB are less than any slot of a wave (53 rows of 18 KiB at the least): refused, like 16 KiB, and
    the context goes on working."""
    ctx, model, pm, pairs, want = rich
    for limit in SL.LIMITS_RICH_PLANNED:
        ctx.set_workspace_limit(limit)
        got = ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS)
        info = ctx.info()
        chunk, chunks, waves = SL.planned(pm.S, 69, 2, limit)
        assert (info["chunk_sites"], info["max_chunks"], info["n_slots"]) == (chunk, chunks, waves), (limit, info)
        assert chunks >= 2
        _assert_equal(got, want, f"{limit} bytes of workspace")
    for limit in SL.LIMITS_RICH_REFUSED:
        ctx.set_workspace_limit(limit)
        buf = np.full(want.shape, 255, np.uint8)
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS, out=buf)
        assert ei.value.code == -4 and "workspace limit too small" in str(ei.value)  # FSMC_ENOMEM
        assert (buf == 255).all()
    ctx.set_workspace_limit(0)
    _assert_equal(ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS), want, "after a refusal")


def test_row_drain_straddles_rows(rich, monkeypatch):
    """Copies of 1000 bytes through the pinned buffers: every copy ends inside a 700-byte row."""
    ctx, model, pm, pairs, want = rich
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", "1000")
    _assert_equal(ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS), want, "copies of 1000 bytes")
    for slice_groups, n_slices in ((1, 2), (2, 1)):
        ctx.set_pair_samples_slice(slice_groups)
        _assert_equal(ctx.decode_pair_samples(model, SL.RICH_N, SL.SEED_MODELS), want,
                      f"copies of 1000 bytes, slices of {slice_groups}")
        assert ctx.last_pair_samples_slices() == n_slices


@pytest.mark.parametrize("case", E.SWEEP_CASES, ids=E.sweep_id)
def test_numeric_edges(case):
    """The edge models of the decode kernels (subnormal table entries and vectors, states at exactly +0 beside the ghost
    states, every state equal, identical and complementary haplotypes) at an exact and two padded members: all 96 pairs,
    two groups, bit for bit."""
    name, K, _ = case
    pm, bits, _, pairs, want = SL.edge_case(name, K)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
    assert ctx.last_kernel() == expected_member(K)
    ctx.close()
    assert (got < K).all()
    _assert_equal(got, want, E.sweep_id(case))


def test_zero_and_nan_sums():
    """A zero scaling sum somewhere: the pair's states only lie in [0, K); the other pairs of its group are exact."""
    pm, bits, _, pairs, want, bad = SL.zero_sum_case()
    assert bad.any() and not bad.all()
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS)
    ctx.close()
    assert (got < pm.K).all()
    _assert_equal(got[~bad], want[~bad], "the pairs with positive sums")


def test_errors(s65):
    """Every FSMC_EINVAL, nothing touched, each followed by a good call."""
    ctx, model, pm, pairs = s65
    want = SL.case("S65")[4]
    _upload(ctx, pm, pairs)

    def good():
        _assert_equal(ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS), want, "after an error")

    def refused(text, n=SL.N_MODELS, mdl=None, null=False):
        buf = np.full((len(pairs), min(max(n, 1), 64), pm.S), 255, np.uint8)
        if null:  # (the wrapper never passes a null pointer: the symbol itself)
            rc = ctx._L.fsmc_decode_pair_samples(ctx._h, (mdl or model)._h, n, 0, None)
            msg = (ctx._L.fsmc_last_error(ctx._h) or b"").decode()
            assert rc == -1 and text in msg, (rc, msg)
        else:
            with pytest.raises(capi.FsmcError) as ei:
                ctx.decode_pair_samples(mdl or model, n, SL.SEED_MODELS, out=buf)
            assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert (buf == 255).all()
        good()

    good()
    for n in (0, -1, 65, 1 << 20):
        refused("n_samples must be 1 ... 64", n=n)
    refused("states is null", null=True)
    assert ctx.last_pair_samples_slices() == 1  # (of the good call)
    groups = capi.whole_sequence_groups(len(pairs), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(pairs), groups)
    buf = np.full(want.shape, 255, np.uint8)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_samples(model, SL.N_MODELS, SL.SEED_MODELS, out=buf)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value) and (buf == 255).all()
    _upload(ctx, pm, pairs)
    good()
    # a model of more than 128 states on the same haplotypes: the wave-group family has no sampling kernel
    wide, wide_bits, _ = LL._problem(130, 65, seed=100 + 69 + 65)
    assert np.array_equal(wide_bits, SL.problem("S65")[1])
    refused("more than 128 states", mdl=ctx.create_model(wide))


def test_sequence_mode_is_refused():
    pm, bits, _, pairs, _, _ = LL.case("seq69")
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    buf = np.full((len(pairs), 2, pm.S), 255, np.uint8)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_samples(model, 2, out=buf)
    assert ei.value.code == -1 and "sequence-mode" in str(ei.value) and (buf == 255).all()
    assert ctx.decode_pair_loglik(model)[0].shape == (len(pairs),)  # (the context is fine)
    ctx.close()


# ---------------------------------------------------------------- the product path: ASMC.samplePairs

@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.samplePairs(a, b, samples, seed) on a synthetic cohort's files, in one flush and in flushes of 128 pairs, twice
    in a row: the restatement's array each time; another seed differs; every other field of the results is empty, and
    decodePairs leaves the new field empty."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, _, _, _, _ = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    pm, _, folded, _ = LL.cohort_problem()
    assert np.array_equal(np.array(api.Data(p).geneticPositions, np.float32), pm.gen)  # (the restatement's model)
    want = SL.cohort_samples()

    for _ in range(2):  # two calls in a row
        asmc.samplePairs(a, b, samples=SL.COHORT_N, seed=SL.SEED_MODELS)
        res = asmc.get_copy_of_results()
        _assert_equal(np.array(res.per_pair_sampled_states), want, "samplePairs")
        assert np.array(res.per_pair_MAPs).size == 0 and np.array(res.per_pair_viterbi_states).size == 0
    asmc.samplePairs(a, b, SL.COHORT_N, SL.SEED_MODELS + 1)
    other = np.array(asmc.get_ref_of_results().per_pair_sampled_states)
    assert other.shape == want.shape and not np.array_equal(other, want)
    assert (other < pm.K).all()
    asmc.samplePairs(a[:3], b[:3])  # the defaults: one sample, seed 0
    one = np.array(asmc.get_copy_of_results().per_pair_sampled_states)
    _assert_equal(one, SL.sample(pm, folded, pairs[:3], 1, 0), "defaults")
    starts, ends, st = api.state_runs(one[0, 0])
    assert starts[0] == 0 and ends[-1] == pm.S and np.array_equal(starts[1:], ends[:-1]) and (st[1:] != st[:-1]).all()
    asmc.decodePairs(a[:3], b[:3], per_pair_MAPs=True)
    res = asmc.get_copy_of_results()
    empty = np.array(res.per_pair_sampled_states)
    assert empty.size == 0 and empty.ndim == 3 and empty.dtype == np.uint8
    assert np.array(res.per_pair_MAPs).shape == (3, pm.S)


SEQUENCE_TEXT = "sampled paths: no sampling kernel for a sequence-mode model"
WIDE_TEXT = r"sampled paths: no sampling kernel for a model of more than 128 states \(130\)"
COUNT_TEXT = r"sampled paths: n_samples must be 1 \.\.\. 64"
A, B = [1, 2, 3, 10, 40, 63, 7], [2, 3, 4, 11, 41, 0, 9]


def _write_quantities(root, tables, haps):
    """The decoding quantities restricted to the rows this map uses (as pair_common.cohort_files does): a small file."""
    import copy

    from fastsmc_amd import synth
    from oracle import oracle as O

    gen = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
    t = copy.copy(tables)
    used = np.unique(np.concatenate([[0.0], O.step_rows(t.keys, gen)[1][1:]]))
    sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
    t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)


def _refused_then_good(p, text):
    """ASMC.samplePairs and HMM.setSampledPaths raise RuntimeError with the ABI's message before anything is decoded; the
    results of the call before are still there and the objects go on working."""
    asmc = api.ASMC(p)
    asmc.decodePairs(A, B, per_pair_posterior_means=True, per_pair_MAPs=True)
    maps = np.array(asmc.get_copy_of_results().per_pair_MAPs)
    assert maps.shape[0] == len(A) and maps.any()
    with pytest.raises(RuntimeError, match=text):
        asmc.samplePairs(A, B, samples=2)
    res = asmc.get_copy_of_results()
    assert np.array_equal(np.array(res.per_pair_MAPs), maps) and np.array(res.per_pair_sampled_states).size == 0
    asmc.decodePairs(A, B, per_pair_posterior_means=True, per_pair_MAPs=True)
    assert np.array_equal(np.array(asmc.get_copy_of_results().per_pair_MAPs), maps)

    hmm = api.HMM(api.Data(p), p)
    hmm.setStorePerPairPosteriorMean(True)
    with pytest.raises(RuntimeError, match=text):
        hmm.setSampledPaths(2, 5)
    hmm.setSampledPaths(0)  # (nothing to refuse)
    hmm.setStorePerPairPosteriorMean(True)  # (a good setter follows)
    assert np.array(hmm.getDecodePairsReturnStruct().per_pair_sampled_states).size == 0


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
    haps = synth.make_haps(64, 100, seed=31, cm_per_mb=25.0, switch_per_cm=0.6)
    synth.write_haps_files(root, haps, fastsmc_map=False)
    _write_quantities(root, synth.make_model_tables(130), haps)
    p = _params(root)
    p.doPerPairMAP = True
    assert not p.decodingSequence
    _refused_then_good(p, WIDE_TEXT)


def test_host_accepts_128_states_and_refuses_sample_counts(tmp_path):
    """The other side of both limits: 128 states, array mode -- the path through the files is the C ABI's; and the sample
    counts the ABI refuses, refused with its message."""
    from fastsmc_amd import synth

    root = str(tmp_path / "k128")
    haps = synth.make_haps(64, 200, seed=31, cm_per_mb=25.0, switch_per_cm=0.6)
    synth.write_haps_files(root, haps, fastsmc_map=False)
    _write_quantities(root, synth.make_model_tables(128), haps)
    asmc = api.ASMC(_params(root))
    asmc.samplePairs(A, B, samples=4, seed=9)
    states = np.array(asmc.get_copy_of_results().per_pair_sampled_states)
    assert states.shape == (len(A), 4, 200) and states.dtype == np.uint8 and (states < 128).all()
    for n in (0, -1, 65):
        with pytest.raises(RuntimeError, match=COUNT_TEXT):
            asmc.samplePairs(A, B, samples=n)
    assert np.array_equal(np.array(asmc.get_copy_of_results().per_pair_sampled_states), states)
    # the overload that takes "<ID>#<1|2>" strings: the same pairs, the same array
    idx = asmc.get_copy_of_results().per_pair_indices
    assert [i[0] for i in idx] == A and [i[2] for i in idx] == B
    asmc.samplePairs([i[1] for i in idx], [i[3] for i in idx], samples=4, seed=9)
    assert np.array_equal(np.array(asmc.get_copy_of_results().per_pair_sampled_states), states)
