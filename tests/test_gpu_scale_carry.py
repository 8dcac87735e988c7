"""Beta stride 2 with a carried scale (csrc/fsmc_decode_kernel_body.h, kCarryScale): a member whose rows have a spare
float (69 and 50 states) stores, beside a beta row, the scaling reciprocal of the row above it, and the alpha sweep
scales the row it recomputes with that float instead of summing the row and dividing.  The first site of a chunk takes
the value from the chunk's checkpoint, the first site of a window from checkpoint slot 0.  The carried float is the
float the sweep would have computed, so every record field, and every sums plane, must be the bits of

  * the stride-1 decode of the same input, which never reads a pad, and
  * the oracle.

Shapes: whole sequences of 70, 65 and 64 sites at a chunk of 16 (a last chunk of 6 sites, of one site, none short) and
61 sites at a requested chunk of 15 (the planner rounds a chunk length up to a multiple of 16, so this runs chunks of 16
too: an odd chunk length cannot be planned); each with 0, 1 and every chunk resident and through the forced pool -- the
kept and the rebuilt writer; windows of 2 and 3 sites; a window that fits one chunk (the single-chunk path); a window
whose scan stops short of it (the checkpoint at scan_to).  Models: the synthetic 69-state tables, the edge models of
tests/edge_models.py (subnormal and zero rows: the carried value may be huge, infinite or scale a zero row), and one
chunked case of the exact 50-state member (IBD only: its stride-2 sums kernel is not built).  At most 96 pairs a case."""
import functools

import numpy as np
import pytest

import edge_models as E
from fastsmc_amd import capi
from oracle import oracle as O
from test_gpu_beta_stride import _assert_records_equal, _pairs_array, _window_oracle

pytestmark = pytest.mark.gpu

AGES = capi.FSMC_WANT_MEAN | capi.FSMC_WANT_MAP
LIMIT = 1 << 30  # room for every chunk of these windows
SIDE_ROWS = 4    # park and per-state-sum rows of a slot (tests/test_gpu_chunk_pool.py, _limit)


def _pool_limit(K, S, chunk, slots, resident):
    """The workspace limit that leaves `resident` stride-2 chunk buffers a wave (tests/test_gpu_chunk_pool.py)."""
    chunk = (chunk + 15) // 16 * 16
    rows = chunk // 2 * (1 + resident) + (S + chunk - 1) // chunk + SIDE_ROWS + 1
    return rows * ((K + 3) // 4) * 64 * 16 * slots


def _context(pm, bits, stride, chunk, variant, monkeypatch, n_groups, L=None):
    """variant: "res0" / "res1" / "resall" = that many resident chunks in the static layout, "pool" = the forced pool
    with two buffers a wave, "whole" = no chunk length, no limit."""
    if variant == "pool":
        monkeypatch.setenv("FSMC_DIAG_MAX_SLOTS", str(n_groups))
    ctx = capi.Context(0)
    ctx.set_beta_stride(stride)
    ctx.set_pairing(0)
    ctx.set_two_wave_windows(1)
    if variant != "whole":
        ctx.set_chunk_sites(chunk)
        if variant == "pool":
            ctx.set_workspace_limit(_pool_limit(pm.K, L or pm.S, chunk, n_groups, 2))
            ctx.set_chunk_pool(1, 700)  # (a window asks for every chunk)
        else:
            ctx.set_workspace_limit(LIMIT)
            ctx.set_chunk_pool(0)
            ctx.set_resident_chunks({"res0": 0, "res1": 1, "resall": -1}[variant])
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    return ctx, model


def _check_plan(ctx, K, stride, variant):
    assert ctx.last_kernel() == K and ctx.last_beta_stride() == stride
    if variant == "whole":
        assert ctx.info()["max_chunks"] == 1
        return
    chunks = ctx.info()["max_chunks"]
    assert chunks > 1 and ctx.info()["chunk_sites"] == 16
    pool = ctx.last_chunk_pool()
    if variant == "pool":
        assert pool["buffers"] > 0 and pool["outstanding"] == 0 and pool["kept"] > 0, pool
    else:
        assert pool["buffers"] == 0
        assert ctx.last_resident_chunks() == {"res0": 0, "res1": 1, "resall": chunks}[variant]


def _ibd(pm, bits, pairs, groups, stride, chunk, variant, flags, monkeypatch, L=None):
    ctx, model = _context(pm, bits, stride, chunk, variant, monkeypatch, len(groups), L)
    got = ctx.decode_ibd(model, _pairs_array(pairs), groups, flags)
    _check_plan(ctx, pm.K, stride, variant)
    ctx.close()
    return got


def _sums(pm, bits, pairs, stride, chunk, variant, monkeypatch):
    groups = capi.whole_sequence_groups(len(pairs), pm.S)
    ctx, model = _context(pm, bits, stride, chunk, variant, monkeypatch, len(groups))
    ctx.upload_worklist(_pairs_array(pairs), groups)
    s, mm = ctx.decode_sums(model, major_minor=True)
    _check_plan(ctx, pm.K, stride, variant)
    ctx.close()
    return [s, *mm]


def _bits_equal(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{what}: plane {i}"


def _records_bits_equal(got, want, what):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), what


# ------------------------------------------------------------ whole sequences of a few chunks (69 synthetic states)

SHAPES = {70: 16, 65: 16, 64: 16, 61: 15}  # sites: requested chunk length


@functools.lru_cache(maxsize=None)
def _problem(K, S):
    return E.benign(K, S=S)


@functools.lru_cache(maxsize=None)
def _oracle_ibd(K, S, flags):
    pm, _, folded, pairs = _problem(K, S)
    return O.decode_pairs_ibd(pm, folded, pairs, batch_size=64, want_mean=bool(flags & capi.FSMC_WANT_MEAN),
                              want_map=bool(flags & capi.FSMC_WANT_MAP))


def _oracle_sums_of(pm, folded, pairs):
    want = [np.zeros((pm.S, pm.K), np.float32) for _ in range(4)]
    for post, ob, hb in E.oracle_posteriors(pm, folded, pairs):
        O.augment_sum_over_pairs(pm, post, post.shape[2], ob, hb, *want)
    return want


@functools.lru_cache(maxsize=None)
def _oracle_sums(K, S):
    pm, _, folded, pairs = _problem(K, S)
    return _oracle_sums_of(pm, folded, pairs)


_stride1 = {}


def _stride1_of(key, run):
    """The stride-1 result of an input, computed once and shared by the cases that compare against it."""
    if key not in _stride1:
        _stride1[key] = run()
    return _stride1[key]


@pytest.mark.parametrize("variant", ["res0", "res1", "resall", "pool"])
@pytest.mark.parametrize("S", sorted(SHAPES))
def test_chunked_windows_ibd(monkeypatch, S, variant):
    pm, bits, _, pairs = _problem(69, S)
    groups = capi.whole_sequence_groups(len(pairs), S)
    for flags in (AGES, 0):
        want1 = _stride1_of(("ibd", S, flags),
                            lambda: _ibd(pm, bits, pairs, groups, 1, SHAPES[S], "res0", flags, monkeypatch))
        got = _ibd(pm, bits, pairs, groups, 2, SHAPES[S], variant, flags, monkeypatch)
        _records_bits_equal(got, want1, f"flags {flags}")
        _assert_records_equal(got, _oracle_ibd(69, S, flags))
    assert _oracle_ibd(69, S, AGES).size > 0


@pytest.mark.parametrize("variant", ["res0", "res1", "resall", "pool"])
@pytest.mark.parametrize("S", sorted(SHAPES))
def test_chunked_windows_sums(monkeypatch, S, variant):
    pm, bits, _, pairs = _problem(69, S)
    want1 = _stride1_of(("sums", S), lambda: _sums(pm, bits, pairs, 1, SHAPES[S], "res0", monkeypatch))
    got = _sums(pm, bits, pairs, 2, SHAPES[S], variant, monkeypatch)
    _bits_equal(got, want1, "stride 1")
    _bits_equal(got, _oracle_sums(69, S), "oracle")


def test_single_chunk_window(monkeypatch):
    """A window under the default chunk length: one chunk, the rows in the chunk buffer, c of the first site in
    checkpoint slot 0."""
    pm, bits, _, pairs = _problem(69, 70)
    groups = capi.whole_sequence_groups(len(pairs), 70)
    for flags in (AGES, 0):
        want1 = _ibd(pm, bits, pairs, groups, 1, 0, "whole", flags, monkeypatch)
        got = _ibd(pm, bits, pairs, groups, 2, 0, "whole", flags, monkeypatch)
        _records_bits_equal(got, want1, f"flags {flags}")
        _assert_records_equal(got, _oracle_ibd(69, 70, flags))
    got = _sums(pm, bits, pairs, 2, 0, "whole", monkeypatch)
    _bits_equal(got, _sums(pm, bits, pairs, 1, 0, "whole", monkeypatch), "stride 1")
    _bits_equal(got, _oracle_sums(69, 70), "oracle")


# ------------------------------------------------------------ windows inside a longer sequence

# first pair, pairs, from, to, scan_from, scan_to
TINY = [(0, 64, 200, 202, 200, 202), (64, 33, 300, 303, 301, 303)]
SHORT_SCAN = [(0, 64, 10, 90, 12, 71), (64, 33, 101, 190, 101, 165)]  # the sweep stops 19 / 25 sites short of the window


def _windows(sp, wins, stride, chunk, variant, monkeypatch):
    n = wins[-1][0] + wins[-1][1]
    pairs = O.enumerate_all_pairs(32)[700:700 + n]
    groups = np.zeros(len(wins), capi.GROUP_DTYPE)
    for g, w in zip(groups, wins):
        g["first_pair"], g["n_pairs"], g["from"], g["to"], g["scan_from"], g["scan_to"] = w
    L = max(w[5] - w[2] for w in wins)
    return pairs, _ibd(sp["model"], sp["bits"], pairs, groups, stride, chunk, variant, AGES, monkeypatch, L)


def _windows_oracle(sp, wins, pairs):
    want = []
    for first, cnt, frm, to, sfrm, sto in wins:
        full = _window_oracle(sp, pairs[first:first + cnt], frm, to, sfrm, sto)
        for v in range(cnt):
            want.append(O.ibd_scan_pair(sp["model"], full, v, sfrm, sto, pair_ordinal=first + v))
    return np.concatenate(want)


def test_windows_of_two_and_three_sites(small_problem, monkeypatch):
    pairs, got = _windows(small_problem, TINY, 2, 0, "whole", monkeypatch)
    _, want1 = _windows(small_problem, TINY, 1, 0, "whole", monkeypatch)
    _records_bits_equal(got, want1, "stride 1")
    _assert_records_equal(got, _windows_oracle(small_problem, TINY, pairs))


@pytest.mark.parametrize("variant", ["res0", "res1", "resall", "pool"])
def test_scan_stops_short_of_the_window(small_problem, monkeypatch, variant):
    """aEnd < to: pass B writes a checkpoint at scan_to, from which the last chunk is rebuilt (or kept)."""
    pairs, got = _windows(small_problem, SHORT_SCAN, 2, 16, variant, monkeypatch)
    want1 = _stride1_of("short-scan", lambda: _windows(small_problem, SHORT_SCAN, 1, 16, "res0", monkeypatch)[1])
    want = _stride1_of("short-scan-oracle", lambda: _windows_oracle(small_problem, SHORT_SCAN, pairs))
    assert want.size > 0
    _records_bits_equal(got, want1, "stride 1")
    _assert_records_equal(got, want)


# ------------------------------------------------------------ the edge models, the 50-state member

@pytest.mark.parametrize("name", sorted(E.SWEEP_BUILDERS))
def test_edge_models(monkeypatch, name):
    """400 sites in chunks of 16, the first chunk kept and the others rebuilt: IBD records and sums."""
    pm, bits, folded, pairs = E.sweep_model(name, 69)
    groups = capi.whole_sequence_groups(len(pairs), pm.S)
    got = _ibd(pm, bits, pairs, groups, 2, 16, "res1", AGES, monkeypatch)
    _records_bits_equal(got, _ibd(pm, bits, pairs, groups, 1, 16, "res0", AGES, monkeypatch), "stride 1")
    _assert_records_equal(got, O.decode_pairs_ibd(pm, folded, pairs, batch_size=64))
    got = _sums(pm, bits, pairs, 2, 16, "res1", monkeypatch)
    _bits_equal(got, _sums(pm, bits, pairs, 1, 16, "res0", monkeypatch), "stride 1")
    _bits_equal(got, _oracle_sums_of(pm, folded, pairs), "oracle")


def test_fifty_state_member(monkeypatch):
    """The exact 50-state member: two spare floats a row, the carried one is float 50 (.z of the last float4)."""
    pm, bits, _, pairs = _problem(50, 70)
    groups = capi.whole_sequence_groups(len(pairs), 70)
    got = _ibd(pm, bits, pairs, groups, 2, 16, "res1", AGES, monkeypatch)
    _records_bits_equal(got, _ibd(pm, bits, pairs, groups, 1, 16, "res0", AGES, monkeypatch), "stride 1")
    _assert_records_equal(got, _oracle_ibd(50, 70, AGES))
    assert _oracle_ibd(50, 70, AGES).size > 0
