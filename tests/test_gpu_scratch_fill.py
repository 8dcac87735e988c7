"""Every kernel on scratch memory an earlier launch left dirty.

The library allocates its scratch memory once and reuses it: the decode workspace, the staging, row and accumulator
buffers of the fsmc_decode_pair_* entry points, the two pinned row buffers, the per-call buffers of fsmc_identify.  Only a
few regions are cleared, so every result is right only if each kernel writes every cell before any kernel reads it.  The
other GPU tests cannot see a break of that rule: a fresh context's first hipMalloc reads as zeros, and a fixture that
reuses a context reruns the same entry point on the same inputs.  Here FSMC_DIAG_SCRATCH_FILL=<byte> makes every entry
point fill every scratch buffer it is about to use, the whole allocation, before anything it writes there
(fsmc_capi.hip, ensure()), and every case asserts
  (a) what the existing test of that configuration asserts: its restatement or oracle, bit for bit;
  (b) np.array_equal (NaNs equal) with the same call on a fresh context without the variable;
  (c) fsmc_ctx_scratch_filled() is 0 without the variable and grows strictly over every entry-point call with it.

Three fill bytes, because each reaches reads the others cannot:
  0xFF  NaN as float and double, -1 as int, state 255 as a byte: survives a multiplication by zero (the ghost mask,
        a zero table entry) and poisons every sum -- but fmaxf / fminf and every comparison drop a NaN, so a stale cell
        that only takes part in a max, a min or an argmax / argmin goes unseen.
  0x7F  3.39e38f, finite, and a huge positive int: wins every max and argmax and overflows sums; loses every min.
  0x80  -1.18e-38f and a very negative int: wins every min and argmin over non-negative probabilities, the one case
        the other two bytes cannot reach.

Every dirty case runs its calls twice on one context: the first round on buffers just allocated, the second on buffers
held from the first -- which the fill dirties again, behind the right answers of round one."""
import ctypes as C

import numpy as np
import pytest

import identify_edges as IE
import pair_bins_lists as BL
import pair_cdf_lists as CL
import pair_loglik_lists as LL
import pair_minima_lists as ML
import pair_sample_lists as SL
import pair_tail_lists as PT
import pair_transition_lists as TL
import pair_viterbi_lists as VL
from conftest import expected_member
from fastsmc_amd import api, capi
from oracle import oracle as O
from pair_common import (EDGES_700, cohort_files, cohort_pairs, params, posterior_tables, problem as _k_problem,
                         upload as _upload)
from test_gpu_beta_stride import _assert_records_equal, _ctx, _pairs_array
from test_gpu_chunk_pool import AGES, CHUNK, _limit, _oracle_records, _work_list
from test_gpu_decode_pairs_together import FIELDS as TOGETHER_FIELDS
from test_gpu_identify_edges import FSMC_EOVERFLOW, FSMC_OK, as_list, device_inputs, fetch, raw_identify
from test_gpu_scale_carry import SHAPES, _check_plan, _context, _oracle_ibd, _oracle_sums, _problem as _carry_problem
from test_gpu_two_wave_windows import _oracle_consumers

pytestmark = pytest.mark.gpu

VAR = "FSMC_DIAG_SCRATCH_FILL"
FILLS = (0xFF, 0x7F, 0x80)
EINVAL = -1


@pytest.fixture(params=FILLS, ids=[f"fill-{b:#04x}" for b in FILLS])
def fill(request):
    return request.param


# ---------------------------------------------------------------- the three assertions

def _same(got, want, what):
    """Equal in type, shape and every bit that is a value: tuples and lists element by element, None with None, records
    byte for byte, arrays np.array_equal with NaNs equal."""
    if want is None:
        assert got is None, what
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{what}[{i}]")
    else:
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
        if want.dtype.names:
            assert got.tobytes() == want.tobytes(), what
        else:
            same = np.array_equal(got, want, equal_nan=want.dtype.kind == "f")
            assert same, f"{what}: {int((~((got == want) | ((got != got) & (want != want)))).sum())} of {got.size} differ"


_clean = {}  # the results of a case's calls on a fresh context without the variable, once a process, read-only


class Call:
    """One entry-point call of a case: `run(ctx)` gives the result, `check(result)` asserts (a) -- or `want`, compared
    with _same."""

    def __init__(self, name, run, want=None, check=None, counts=True):
        self.name, self.run, self.counts = name, run, counts
        self.check = check if check is not None else (lambda got: _same(got, want, name))


def _run_case(monkeypatch, fill, key, open_ctx, calls, rounds=2, before_round=None):
    """(a), (b) and (c) for `calls` on the context `open_ctx()` gives: once without the variable on a fresh context (kept
    for the other fill bytes of the case), then `rounds` times over with it on another."""
    if key not in _clean:
        monkeypatch.delenv(VAR, raising=False)
        ctx = open_ctx()
        if before_round:
            before_round(ctx, 0)
        _clean[key] = [c.run(ctx) for c in calls]
        assert ctx.scratch_filled() == 0, key
        ctx.close()
        for c, res in zip(calls, _clean[key]):
            c.check(res)
    monkeypatch.setenv(VAR, str(fill))
    ctx = open_ctx()
    for rnd in range(rounds):
        if before_round:
            before_round(ctx, rnd)
        for c, clean in zip(calls, _clean[key]):
            filled = ctx.scratch_filled()
            got = c.run(ctx)
            if c.counts:
                assert ctx.scratch_filled() > filled, (key, c.name, rnd)
            c.check(got)
            _same(got, clean, f"{key} {c.name} round {rnd}: differs from a fresh context without {VAR}")
    monkeypatch.delenv(VAR)
    filled = ctx.scratch_filled()
    assert filled > 0
    for c, clean in zip(calls[:1], _clean[key]):  # (the variable is read at every call: unset, nothing is filled)
        _same(c.run(ctx), clean, f"{key} {c.name} after {VAR} was unset")
    assert ctx.scratch_filled() == filled
    ctx.close()


def _open(pm, bits):
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    ctx.model = model
    return ctx


# ---------------------------------------------------------------- the nine fsmc_decode_pair_* entry points

PROBLEMS = ("S65", "S200", "dense40")  # K = 69 at 65 and 200 sites; K = 40 on the dense map, the 48-state member
N_PAIRS = 70                           # a full group and a ragged one of 6: two slices of one group
CHUNK_SITES = 27                       # 3 / 8 / 12 chunks, the last ragged
ROW_COPY = 1000                        # bytes a copy through the pinned buffers: copies end inside rows
N_SAMPLES = 3
ENTRIES = ("posteriors", "minima", "bins", "cdf", "tail", "loglik", "viterbi", "samples", "transitions")
SWEEPS = ("viterbi", "samples", "transitions")  # their own kernels on the workspace: chunks and checkpoints of their own


def _pair_problem(prob):
    pm, bits, folded, pairs, _ = SL.problem(prob)
    return pm, bits, folded, pairs[:N_PAIRS]


def _odd_edges(pm):
    """Bin edges at no multiple of four, a one-site bin among them: pair_transition_lists.EDGES["odd"] where the
    sequence holds it, the same edges cut to 65 sites where not."""
    odd = TL.EDGES["odd"]
    return odd if pm.S >= int(odd[-1]) else np.array([3, 10, 11, 50, 65], np.int32)


def _cuts(pm):
    return sorted({1, min(int(pm.state_threshold), pm.K), min(25, pm.K), pm.K})


_wants = {}


def _pair_calls(entry, prob):
    """(set-up of the context, the entry point's call with the restatement's result) on the problem `prob`."""
    pm, bits, folded, pairs = _pair_problem(prob)
    edges, K, S = _odd_edges(pm), pm.K, pm.S
    key = (entry, prob)
    if entry == "posteriors":
        if key not in _wants:
            _wants[key] = posterior_tables(pm, folded, pairs)
        run = lambda ctx: ctx.decode_pair_posteriors(ctx.model, pm.exp_times, sum_into=np.zeros((K, S), np.float32))
        slicer = "set_pair_posterior_slice"
    elif entry in ("minima", "bins"):
        if ("rows", prob) not in _wants:
            _wants["rows", prob] = ML.oracle_rows(pm, folded, pairs)
        mean, mp = _wants["rows", prob]
        if entry == "minima":
            _wants.setdefault(key, ML.first_minima(mean) + ML.first_minima(mp))
            run = lambda ctx: ctx.decode_pair_minima(ctx.model, pm.exp_times)
            slicer = "set_pair_minima_slice"
        else:
            _wants.setdefault(key, BL.expected(mean, mp, edges))
            run = lambda ctx: ctx.decode_pair_bins(ctx.model, pm.exp_times, edges)
            slicer = "set_pair_bins_slice"
    elif entry in ("cdf", "tail"):
        cuts = _cuts(pm)
        if entry == "cdf":
            if key not in _wants:
                _wants[key] = CL.expected(pm, folded, pairs, cuts, CL.QS)
            run = lambda ctx: ctx.decode_pair_cdf(ctx.model, cuts, CL.QS)
            slicer = "set_pair_cdf_slice"
        else:
            w = PT.widths(pm.gen)
            if key not in _wants:
                _wants[key] = PT.expected(CL.expected(pm, folded, pairs, cuts, [])[0], edges, w)
            run = lambda ctx: ctx.decode_pair_tail_summaries(ctx.model, cuts, edges, w)
            slicer = "set_pair_tail_slice"
    elif entry == "loglik":
        if key not in _wants:
            _wants[key] = LL.expected(LL.forward(pm, folded, pairs)[0], edges)
        run = lambda ctx: ctx.decode_pair_loglik(ctx.model, bin_edges=edges)
        slicer = "set_pair_loglik_slice"
    elif entry == "viterbi":
        if key not in _wants:
            states, sums, last = VL.case(prob)[4:7]
            _wants[key] = (states[:N_PAIRS],) + VL.expected(sums[:N_PAIRS], last[:N_PAIRS])
        run = lambda ctx: ctx.decode_pair_viterbi(ctx.model)
        slicer = "set_pair_viterbi_slice"
    elif entry == "samples":
        if key not in _wants:
            _wants[key] = SL.case(prob, n=N_SAMPLES, first=N_PAIRS)[4]
        run = lambda ctx: ctx.decode_pair_samples(ctx.model, N_SAMPLES, SL.SEED_MODELS)
        slicer = "set_pair_samples_slice"
    else:
        if key not in _wants:
            down, up = TL.case(prob, first=N_PAIRS)[4:6]
            _wants[key] = (down, up, TL.bin_sums(down, edges), TL.bin_sums(up, edges))
        run = lambda ctx: ctx.decode_pair_transitions(ctx.model, bin_edges=edges)
        slicer = "set_pair_transitions_slice"
    want = _wants[key]

    def open_ctx():
        ctx = _open(pm, bits)
        _upload(ctx, pm, pairs)
        getattr(ctx, slicer)(1)
        ctx.set_chunk_sites(CHUNK_SITES)
        return ctx

    def run_and_look(ctx):
        got = run(ctx)
        assert getattr(ctx, "last_pair_" + slicer[len("set_pair_"):] + "s")() == 2  # the second slice reuses the buffers
        assert ctx.last_kernel() == expected_member(K)
        info = ctx.info()
        if entry in SWEEPS or (entry != "loglik" and ctx.last_waves_per_window() == 1):  # (two waves: whole windows)
            chunk = CHUNK_SITES if entry in SWEEPS else (CHUNK_SITES + 15) // 16 * 16  # (the decode: multiples of 16)
            assert info["chunk_sites"] == chunk and info["max_chunks"] == -(-S // chunk) >= 3, info
        if entry not in SWEEPS and entry != "loglik":
            assert ctx.last_waves_per_window() == 2 - ctx.one_wave, (ctx.one_wave, info)
        return got

    return open_ctx, Call(entry, run_and_look, want)


@pytest.mark.parametrize("prob", PROBLEMS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_pair_entry_points(monkeypatch, fill, entry, prob):
    """70 pairs in slices of one group, chunks of 27 sites, copies of 1000 bytes through both pinned buffers, the minima in
    ranges of 16 pairs; the decode-fed entry points once with two waves per window and once on the one-wave kernels."""
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", str(ROW_COPY))
    monkeypatch.setenv("FSMC_DIAG_MINIMA_RANGE", "16")
    open_ctx, call = _pair_calls(entry, prob)

    def waves(ctx, rnd):
        ctx.one_wave = rnd & 1
        ctx.set_two_wave_windows(ctx.one_wave)

    _run_case(monkeypatch, fill, ("pair", entry, prob), open_ctx, [call], before_round=waves)


# ---------------------------------------------------------------- the IBD decode: pool, resident chunks, strides, pairing

IBD_CONFIGS = {  # name: (beta stride, pairing, chunk pool mode, resident chunks, workspace limit in _limit()s or bytes)
    "pool-stride1": (1, 0, 1, -1, 1), "pool-stride2": (2, 0, 1, -1, 1),
    "static-resident0-stride1": (1, 0, 0, 0, 64 << 20), "static-resident0-stride2": (2, 0, 0, 0, 64 << 20),
    "static-auto-stride1": (1, 0, 0, -1, 64 << 20), "static-auto-stride2": (2, 0, 0, -1, 64 << 20),
    "pool-beside-paired": (2, 1, 1, -1, 2),
}


@pytest.mark.parametrize("config", sorted(IBD_CONFIGS))
def test_ibd_windows_over_several_rounds(small_problem, monkeypatch, fill, config):
    """The thirty windows of test_gpu_chunk_pool.py on three waves (ten rounds a slot, FSMC_DIAG_MAX_SLOTS=3), chunks of
    48 sites: the forced pool (a buffer handed from wave to wave), the static layout with no and with every resident
    chunk the limit holds, strides 1 and 2, and half-full groups paired beside the pool."""
    stride, pairing, pool, resident, limit = IBD_CONFIGS[config]
    _, pairs, groups = _work_list()
    monkeypatch.setenv("FSMC_DIAG_MAX_SLOTS", "3")
    want = _oracle_records(small_problem, AGES)

    def open_ctx():
        ctx, model = _ctx(small_problem, stride, limit=limit * _limit(small_problem, stride, 3, 2) if limit < 16 else limit,
                          chunk=CHUNK)
        ctx.model = model
        ctx.set_pairing(pairing)
        ctx.set_chunk_pool(pool, 700)
        ctx.set_resident_chunks(resident)
        return ctx

    def run(ctx):
        got = ctx.decode_ibd(ctx.model, pairs, groups, AGES)
        state = ctx.last_chunk_pool()
        assert ctx.info()["max_chunks"] == 14 and state["outstanding"] == 0
        assert (state["buffers"] > 0 and state["kept"] > 0) if pool else state["buffers"] == 0
        if not pairing:
            assert ctx.info()["n_slots"] == 3
        else:
            assert ctx.last_items() > 0
        return got

    _run_case(monkeypatch, fill, ("ibd", config), open_ctx, [Call("decode_ibd", run, check=lambda got: _assert_records_equal(got, want))])


@pytest.mark.parametrize("variant", ["res0", "resall", "pool"])
def test_ibd_and_sums_with_carried_scales(monkeypatch, fill, variant):
    """test_gpu_scale_carry.py's whole sequences of a few chunks (70 sites in chunks of 16, stride 2: the stored beta rows
    carry the recomputed row's scale): the IBD records and the sums over pairs."""
    S = 70
    pm, bits, _, pairs = _carry_problem(69, S)
    groups = capi.whole_sequence_groups(len(pairs), S)
    pr = _pairs_array(pairs)
    want_ibd, want_sums = _oracle_ibd(69, S, AGES), _oracle_sums(69, S)

    def open_ctx():
        ctx, model = _context(pm, bits, 2, SHAPES[S], variant, monkeypatch, len(groups))
        ctx.model = model
        return ctx

    def ibd(ctx):
        got = ctx.decode_ibd(ctx.model, pr, groups, AGES)
        _check_plan(ctx, pm.K, 2, variant)
        return got

    def sums(ctx):
        ctx.upload_worklist(pr, groups)
        s, mm = ctx.decode_sums(ctx.model, major_minor=True)
        _check_plan(ctx, pm.K, 2, variant)
        return [s, *mm]

    _run_case(monkeypatch, fill, ("carry", variant), open_ctx,
              [Call("decode_ibd", ibd, check=lambda got: _assert_records_equal(got, want_ibd)),
               Call("decode_sums", sums, want_sums)])


# ---------------------------------------------------------------- the whole-sequence consumers

_consumers = {}


def _consumer_calls(sp, pairs, key):
    """decode_posteriors (the lanes of the groups' pairs), decode_per_pair and decode_sums with the 00 / 01 / 11 split of
    whole-sequence groups over `pairs`, against the oracle."""
    pm = sp["model"]
    if key not in _consumers:
        _consumers[key] = _oracle_consumers(sp, pairs)
    posts, means, maps, sums = _consumers[key]
    counts = [min(64, len(pairs) - b0) for b0 in range(0, len(pairs), 64)]

    def dump(ctx):
        return [g[:, :, :n] for g, n in zip(ctx.decode_posteriors(ctx.model), counts)]

    def all_sums(ctx):
        s, mm = ctx.decode_sums(ctx.model, major_minor=True)
        return [s, *mm]

    return [Call("decode_posteriors", dump, posts), Call("decode_per_pair", lambda ctx: ctx.decode_per_pair(ctx.model, pm.exp_times), (means, maps)),
            Call("decode_sums", all_sums, sums)]


@pytest.mark.parametrize("chunk", [0, CHUNK])
def test_whole_sequence_consumers(small_problem, monkeypatch, fill, window_waves, chunk):
    """The dump, the per-pair rows and the sums of 100 pairs (a full group and a ragged one) on small_problem, whole
    windows and chunks of 48 sites with resident chunks, with two waves per window and on the one-wave kernels."""
    pm = small_problem["model"]
    pairs = O.enumerate_all_pairs(32)[:100]

    def open_ctx():
        ctx = _open(pm, small_problem["bits"])
        if chunk:
            ctx.set_workspace_limit(64 << 20)
            ctx.set_chunk_sites(chunk)
        _upload(ctx, pm, pairs)
        return ctx

    _run_case(monkeypatch, fill, ("consumers", window_waves, chunk), open_ctx, _consumer_calls(small_problem, pairs, "small"))


def test_sequence_mode(seq_problem, monkeypatch, fill):
    """decodingSequence (two transition steps a site): records, dump, per-pair rows and sums of 100 pairs."""
    pm = seq_problem["model"]
    pairs = O.enumerate_all_pairs(32)[:100]
    pr, groups = _pairs_array(pairs), capi.whole_sequence_groups(len(pairs), pm.S)
    if "seq-ibd" not in _consumers:
        _consumers["seq-ibd"] = O.decode_pairs_ibd(pm, seq_problem["folded"], pairs, batch_size=64)
    want = _consumers["seq-ibd"]
    calls = [Call("decode_ibd", lambda ctx: ctx.decode_ibd(ctx.model, pr, groups), check=lambda got: _assert_records_equal(got, want))]
    _run_case(monkeypatch, fill, "sequence", lambda: _open(pm, seq_problem["bits"]),
              calls + _consumer_calls(seq_problem, pairs, "seq"))


# ---------------------------------------------------------------- the other kernels: wave groups and any K

_wide = {}  # a wide model's problem and its oracle records (_consumers holds the oracle's consumers under the same key)


@pytest.mark.parametrize("K", [130, 1025])
def test_wide_models(monkeypatch, fill, K):
    """The smallest member of the wave-group kernel (130 states: four waves of 48) and the any-K kernel, which keeps a
    pair's whole K-vectors in the workspace (1025 states), at the 200 sites of test_gpu_generic_k.py: records and the
    three consumers of 70 pairs."""
    key = ("wide", K)
    if key not in _wide:
        pm, bits, folded = _k_problem(K)
        pairs = O.enumerate_all_pairs(32)[:N_PAIRS]
        _wide[key] = (pm, bits, folded, pairs, O.decode_pairs_ibd(pm, folded, pairs, batch_size=64))
    pm, bits, folded, pairs, want = _wide[key]
    pr, groups = _pairs_array(pairs), capi.whole_sequence_groups(len(pairs), pm.S)

    def ibd(ctx):
        got = ctx.decode_ibd(ctx.model, pr, groups)
        assert ctx.last_kernel() == expected_member(K)
        return got

    calls = [Call("decode_ibd", ibd, check=lambda got: _assert_records_equal(got, want))]
    _run_case(monkeypatch, fill, key, lambda: _open(pm, bits),
              calls + _consumer_calls(dict(model=pm, folded=folded), pairs, key))


# ---------------------------------------------------------------- fsmc_identify

IDENTIFY = ("chunk_runs-W100-gap1",            # the default kernel
            "deep_split-ra32-hap-gap1",        # the general kernel with split seeds: the depth bytes
            IE.names("stage_overflow")[0])     # more reports of a tile than its LDS stage holds: straight appends


@pytest.mark.parametrize("name", IDENTIFY)
def test_identify(monkeypatch, fill, name):
    c = IE.case(name)
    words, ids = device_inputs(c)

    def run(ctx):
        rec = ctx.identify(words, ids, c.gen, **c.kw)
        assert as_list(rec) == c.want
        return rec

    _run_case(monkeypatch, fill, ("identify", name), lambda: capi.Context(0), [Call("identify", run, check=lambda rec: None)])


def test_identify_through_the_stash(monkeypatch, fill):
    """cap below the count: the complete list is ordered into the context's stash and leaves through fsmc_identify_fetch
    -- the stash is filled before the sort writes it, never between the two calls."""
    c = IE.case("chunk_runs-W100-gap1")
    count = len(c.want)

    def run(ctx):
        rc, n, _ = raw_identify(ctx, c, count - 1)
        assert (rc, n) == (FSMC_EOVERFLOW, count)
        filled = ctx.scratch_filled()
        rc, n, out = fetch(ctx, count)
        assert (rc, n) == (FSMC_OK, count) and as_list(out) == c.want
        assert ctx.scratch_filled() == filled  # (the fetch takes no scratch)
        return out

    _run_case(monkeypatch, fill, "identify-stash", lambda: capi.Context(0), [Call("identify + fetch", run, check=lambda rec: None)])


# ---------------------------------------------------------------- one context, many tenants

def _rich():
    pm, bits, folded, pairs, _ = SL.problem("rich")
    return pm, bits, folded, pairs


def _tenants(pm, bits, folded, pairs, tag, samples, windows=True):
    """The entry points as tenants of one context, each with the restatement's result: name -> Call.  The tenant sets what
    it needs on the context (work list, chunk length) and leaves the chunk length automatic."""
    K, S = pm.K, pm.S
    edges = np.array([e for e in EDGES_700 if e <= S] + ([] if S >= EDGES_700[-1] else [S]), np.int32)
    cuts = _cuts(pm)
    w = PT.widths(pm.gen)

    def want(name, make):
        if (tag, name) not in _wants:
            _wants[tag, name] = make()
        return _wants[tag, name]

    def whole(run, chunk=0):
        def go(ctx):
            _upload(ctx, pm, pairs)
            ctx.set_chunk_sites(chunk)
            got = run(ctx)
            ctx.set_chunk_sites(0)
            return got
        return go

    rows = lambda: want("rows", lambda: ML.oracle_rows(pm, folded, pairs))  # noqa: E731
    tails = lambda: want("tails", lambda: CL.expected(pm, folded, pairs, cuts, [])[0])  # noqa: E731
    trans = lambda: want("trans", lambda: (lambda d, u, _: (d, u, TL.bin_sums(d, edges), TL.bin_sums(u, edges)))(
        *TL.transitions(pm, folded, pairs)))  # noqa: E731
    t = {
        "samples": Call("samples", whole(lambda ctx: ctx.decode_pair_samples(ctx.model, samples, SL.SEED_MODELS)),
                        want("samples", lambda: SL.sample(pm, folded, pairs, samples, SL.SEED_MODELS))),
        "transitions-27": Call("transitions-27", whole(lambda ctx: ctx.decode_pair_transitions(ctx.model, bin_edges=edges),
                                                       CHUNK_SITES), trans()),
        "viterbi": Call("viterbi", whole(lambda ctx: ctx.decode_pair_viterbi(ctx.model)),
                        want("viterbi", lambda: (lambda st, su, la: (st,) + VL.expected(su, la))(*VL.viterbi(pm, folded, pairs)))),
        "loglik": Call("loglik", whole(lambda ctx: ctx.decode_pair_loglik(ctx.model, bin_edges=edges)),
                       want("loglik", lambda: LL.expected(LL.forward(pm, folded, pairs)[0], edges))),
        "posteriors": Call("posteriors", whole(lambda ctx: ctx.decode_pair_posteriors(
            ctx.model, pm.exp_times, sum_into=np.zeros((K, S), np.float32))), want("post", lambda: posterior_tables(pm, folded, pairs))),
        "tail": Call("tail", whole(lambda ctx: ctx.decode_pair_tail_summaries(ctx.model, cuts, edges, w)),
                     want("tail", lambda: PT.expected(tails(), edges, w))),
        "minima": Call("minima", whole(lambda ctx: ctx.decode_pair_minima(ctx.model, pm.exp_times)),
                       want("minima", lambda: ML.first_minima(rows()[0]) + ML.first_minima(rows()[1]))),
        "transitions": Call("transitions", whole(lambda ctx: ctx.decode_pair_transitions(ctx.model, bin_edges=edges)), trans()),
    }
    ibd_whole = want("ibd", lambda: O.decode_pairs_ibd(pm, folded, pairs, batch_size=64))
    pr = _pairs_array(pairs)
    t["ibd-whole"] = Call("ibd-whole", lambda ctx: ctx.decode_ibd(ctx.model, pr, capi.whole_sequence_groups(len(pairs), S)),
                          check=lambda got: _assert_records_equal(got, ibd_whole))
    if windows:
        wins = [(0, 40, 3, S - 4, 3, S - 4), (40, len(pairs) - 40, 10, S // 2, 37, S // 2 - 30)]
        groups = np.zeros(len(wins), capi.GROUP_DTYPE)
        for g, win in zip(groups, wins):
            g["first_pair"], g["n_pairs"], g["from"], g["to"], g["scan_from"], g["scan_to"] = win

        def windowed():
            out = []
            for first, cnt, frm, to, sfrm, sto in wins:
                sub = pairs[first:first + cnt]
                ob = np.stack([(folded[a] ^ folded[b])[frm:to] for a, b in sub])
                hb = np.stack([(folded[a] & folded[b])[frm:to] for a, b in sub])
                full = np.zeros((S, K, cnt), np.float32)
                full[frm:to] = O.decode_batch(pm, ob, hb, frm, to)[0][frm:to]
                out += [O.ibd_scan_pair(pm, full, v, sfrm, sto, pair_ordinal=first + v) for v in range(cnt)]
            return np.concatenate(out)

        ibd_win = want("ibd-windows", windowed)
        t["ibd-windows"] = Call("ibd-windows", lambda ctx: ctx.decode_ibd(ctx.model, pr, groups),
                                check=lambda got: _assert_records_equal(got, ibd_win))
    return t


ORDER = ("samples", "transitions-27", "viterbi", "loglik", "posteriors", "tail", "minima", "ibd-windows", "ibd-whole")


@pytest.mark.parametrize("dirt", ["natural", 0xFF, 0x7F, 0x80], ids=lambda d: d if d == "natural" else f"fill-{d:#04x}")
def test_one_context_many_tenants(monkeypatch, dirt):
    """What the product does: one context for its lifetime, the entry points one after another with different layouts
    over the same bytes.  On the rich problem (K = 69, 700 sites, 70 pairs): eight samples, transitions in chunks of 27,
    Viterbi, log-likelihoods with bins, posteriors, tail summaries, minima, the IBD decode of a windowed list and of the
    whole-sequence one; transitions and samples under a workspace limit of a mebibyte; everything in reverse order; then
    a K = 32 and a K = 128 model on the same context, whose buffers are larger than they need and every offset differs.
    Once with the fill and once on the dirt the tenants leave each other."""
    if dirt == "natural":
        monkeypatch.delenv(VAR, raising=False)
    else:
        monkeypatch.setenv(VAR, str(dirt))
    pm, bits, folded, pairs = _rich()
    ctx = _open(pm, bits)
    tenants = _tenants(pm, bits, folded, pairs, "rich", 8)
    filled = [0]

    def serve(call):
        got = call.run(ctx)
        call.check(got)
        now = ctx.scratch_filled()
        assert (now == 0) if dirt == "natural" else (now > filled[0]), call.name
        filled[0] = now

    for name in ORDER:
        serve(tenants[name])
    ctx.set_workspace_limit(1 << 20)
    serve(tenants["transitions"])
    assert ctx.info()["max_chunks"] >= 2
    serve(tenants["samples"])
    ctx.set_workspace_limit(0)
    for name in reversed(ORDER):
        serve(tenants[name])
    for K in (32, 128):  # (pair_common.problem: 64 haplotypes x 200 sites)
        pm2, bits2, folded2 = _k_problem(K)
        ctx.model = ctx.create_model(pm2)
        ctx.upload_haps(bits2, pm2.S)
        other = _tenants(pm2, bits2, folded2, pairs, f"K{K}", 2, windows=False)
        for name in ORDER:
            if name in other:
                serve(other[name])
        assert ctx.last_kernel() == K
    ctx.close()


# ---------------------------------------------------------------- the product path

def _together_fields(res):
    return {name: np.array(getattr(res, name)) for name in TOGETHER_FIELDS}


_product = {}


def test_product_path(tmp_path, monkeypatch, fill):
    """One ASMC object on the 64 x 700 cohort, flushes of 128 pairs: decodePairs with every output, samplePairs,
    decodePairTransitions, decodePairs again.  The sampled paths and the change probabilities are the restatements'; every
    decodePairs field is that of the same sequence on an ASMC object without the variable (whose fields
    test_gpu_decode_pairs_together.py ties to one call a family and tests/test_gpu_pair_*.py to the oracle), both times.
    The object keeps its context to itself, so (c) is shown through the refusal: a bad value reaches this path, and the
    flush it fails leaves nothing queued -- the same call decodes once the variable is gone."""
    monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", "128")
    p = params(cohort_files(tmp_path)[0])
    _, a, b = cohort_pairs()
    w = api.site_widths(np.array(api.Data(p).geneticPositions, np.float32))
    everything = dict(per_pair_posteriors=True, sum_of_posteriors=True, per_pair_posterior_means=True, per_pair_MAPs=True,
                      min_posterior_means=True, min_MAPs=True, site_bins=EDGES_700, tail_times=[50, 200], quantiles=[0.5],
                      tail_summary_times=[50, 200], site_weights=w)
    wd, wu = TL.cohort_transitions()
    want_t = (wd, wu, TL.bin_sums(wd, EDGES_700), TL.bin_sums(wu, EDGES_700))

    def sequence(asmc):
        asmc.decodePairs(a, b, **everything)
        first = _together_fields(asmc.get_copy_of_results())
        asmc.samplePairs(a, b, samples=SL.COHORT_N, seed=SL.SEED_MODELS)
        _same(np.array(asmc.get_copy_of_results().per_pair_sampled_states), SL.cohort_samples(), "samplePairs")
        asmc.decodePairTransitions(a, b, site_bins=EDGES_700)
        res = asmc.get_copy_of_results()
        _same(tuple(np.array(x) for x in (res.per_pair_down_probabilities, res.per_pair_up_probabilities,
                                          res.bin_expected_downs, res.bin_expected_ups)), want_t, "decodePairTransitions")
        asmc.decodePairs(a, b, **everything)
        return first, _together_fields(asmc.get_copy_of_results())

    if "clean" not in _product:
        monkeypatch.delenv(VAR, raising=False)
        first, again = sequence(api.ASMC(p))
        assert all(first[name].size > 0 for name in TOGETHER_FIELDS)
        for name in TOGETHER_FIELDS:
            _same(again[name], first[name], name + " (again, clean)")
        _product["clean"] = first
    monkeypatch.setenv(VAR, str(fill))
    asmc = api.ASMC(p)
    for got in sequence(asmc):
        for name in TOGETHER_FIELDS:
            _same(got[name], _product["clean"][name], name)
    monkeypatch.setenv(VAR, "256")
    with pytest.raises(RuntimeError, match=VAR):
        asmc.decodePairs(a[:3], b[:3], per_pair_MAPs=True)
    monkeypatch.delenv(VAR)
    asmc.decodePairs(a[:3], b[:3], per_pair_MAPs=True)
    assert np.array(asmc.get_copy_of_results().per_pair_MAPs).shape == (3, 700)


# ---------------------------------------------------------------- the refusal

@pytest.mark.parametrize("bad", ["256", "ff", "", "-1", "12 ", "0x7f"])
def test_a_bad_value_is_refused(monkeypatch, bad):
    """A value that is no integer in 0..255: FSMC_EINVAL naming the variable from every kind of entry point, nothing
    launched, no output touched, nothing counted; the context works once the variable is gone."""
    pm, bits, folded, pairs = _pair_problem("S65")
    ctx = _open(pm, bits)
    _upload(ctx, pm, pairs)
    monkeypatch.setenv(VAR, bad)
    n, S = len(pairs), pm.S
    down, up = np.full((n, S), -7, np.float32), np.full((n, S), -7, np.float32)
    states = np.full((n, 2, S), 255, np.uint8)
    mean = np.full((n, S), -7, np.float32)
    refused = [
        lambda: ctx.decode_pair_transitions(ctx.model, out=(down, up, None, None)),
        lambda: ctx.decode_pair_samples(ctx.model, 2, 1, out=states),
        lambda: ctx.decode_pair_loglik(ctx.model),
        lambda: ctx.decode_pair_cdf(ctx.model, [1], []),
        lambda: ctx.decode_ibd_launch(ctx.model),
        lambda: ctx.decode_sums(ctx.model),
        lambda: ctx._check(ctx._L.fsmc_decode_per_pair(ctx._h, ctx.model._h, capi._p(np.ascontiguousarray(pm.exp_times, np.float32)),
                                                        capi._p(mean), None)),
    ]
    for call in refused:
        with pytest.raises(capi.FsmcError) as ei:
            call()
        assert ei.value.code == EINVAL and VAR in str(ei.value), str(ei.value)
    c = IE.case("chunk_runs-W100-gap1")
    out = np.zeros(len(c.want), capi.CANDIDATE_DTYPE)
    rc, n_out, _ = raw_identify(ctx, c, len(c.want), out=out)
    assert rc == EINVAL and n_out == 0 and VAR in (ctx._L.fsmc_last_error(ctx._h) or b"").decode() and not out.view(np.uint8).any()
    assert (down == -7).all() and (up == -7).all() and (states == 255).all() and (mean == -7).all()
    assert ctx.scratch_filled() == 0
    with pytest.raises(capi.FsmcError):  # (nothing was launched: no IBD decode is in flight)
        ctx.decode_ibd_fetch()
    monkeypatch.delenv(VAR)
    _same(ctx.decode_pair_transitions(ctx.model)[:2], TL.case("S65", first=N_PAIRS)[4:6], "after the refusal")
    rc, n_out, out = raw_identify(ctx, c, len(c.want))
    assert (rc, n_out) == (FSMC_OK, len(c.want)) and as_list(out) == c.want
    ctx.close()
