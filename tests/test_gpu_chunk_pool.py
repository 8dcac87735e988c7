"""The chunk pool (fsmc_ctx_set_chunk_pool): the resident chunk buffers of a launch lie behind the waves' slots and are
claimed chunk by chunk while the kernel runs -- a wave keeps the rows of a chunk if a buffer is free when its backward
pass enters the chunk, rebuilds the chunk otherwise, and gives the buffer back when its forward sweep has passed it.  A
kept row and a rebuilt row are the same bits, so the records and the sums must not depend on who got which buffer: one
wave re-using buffers across its own groups, three waves competing, a pool that holds one or two chunks a wave, a
request capped at the wave's share, at twice that, at every chunk; beta stride 1 and 2; with and without segment ages;
windows whose scan ends inside a chunk, windows of one to three sites, groups of 9 to 64 pairs.  References: the same
list with the pool off and no resident chunk, byte for byte, and the oracle."""
import numpy as np
import pytest

from fastsmc_amd import capi
from oracle import oracle as O
from test_gpu_beta_stride import _assert_records_equal, _ctx, _pairs_array, _window_oracle
from test_gpu_resident_chunks import WINS

pytestmark = pytest.mark.gpu

CHUNK = 48
REPS = 3  # the window list three times over: 30 groups
AGES = capi.FSMC_WANT_MEAN | capi.FSMC_WANT_MAP
N_WIN_PAIRS = WINS[-1][0] + WINS[-1][1]


def _work_list():
    """WINS, REPS times: repetition r decodes the same haplotype pairs as list positions r * n ... (r + 1) * n - 1."""
    base = O.enumerate_all_pairs(32)[500:500 + N_WIN_PAIRS]
    groups = np.zeros(REPS * len(WINS), capi.GROUP_DTYPE)
    for r in range(REPS):
        for g, w in zip(groups[r * len(WINS):(r + 1) * len(WINS)], WINS):
            g["first_pair"], g["n_pairs"], g["from"], g["to"], g["scan_from"], g["scan_to"] = w
            g["first_pair"] += r * N_WIN_PAIRS
    return base, _pairs_array(base * REPS), groups


def _multi_chunk_chunks(groups):
    """Chunks of the windows that have more than one: each is either kept or rebuilt (the sweep ends at scan_to)."""
    n = 0
    for g in groups:
        chunks = (int(g["scan_to"]) - int(g["from"]) + CHUNK - 1) // CHUNK
        n += chunks if chunks > 1 else 0
    return n


def _limit(sp, stride, slots, resident):
    """The workspace limit that leaves `resident` pool buffers a wave: a slot's chunk buffer, 14 checkpoints, four side
    rows and the table row, and `resident` chunk buffers, rows of K/4 x 64 float4."""
    rows_per_chunk = CHUNK // stride
    chunks = (sp["model"].S + CHUNK - 1) // CHUNK
    rows = rows_per_chunk * (1 + resident) + chunks + 4 + 1
    return rows * ((sp["model"].K + 3) // 4) * 64 * 16 * slots


_static = {}
_oracle = {}


def _static_records(sp, stride, flags):
    """Reference: no pool, no resident chunk, every group a wave of its own (computed once per stride and flags)."""
    if (stride, flags) not in _static:
        _, pairs, groups = _work_list()
        ctx, model = _ctx(sp, stride, limit=64 << 20, chunk=CHUNK)
        ctx.set_pairing(0)
        ctx.set_chunk_pool(0)
        ctx.set_resident_chunks(0)
        _static[stride, flags] = ctx.decode_ibd(model, pairs, groups, flags)
        assert ctx.last_resident_chunks() == 0 and ctx.last_chunk_pool()["buffers"] == 0
        ctx.close()
    return _static[stride, flags]


def _oracle_records(sp, flags):
    if "post" not in _oracle:
        base, _, _ = _work_list()
        _oracle["post"] = [_window_oracle(sp, base[first:first + cnt], frm, to, sfrm, sto)
                           for first, cnt, frm, to, sfrm, sto in WINS]
    if flags not in _oracle:
        want = []
        for r in range(REPS):
            for full, (first, cnt, frm, to, sfrm, sto) in zip(_oracle["post"], WINS):
                for v in range(cnt):
                    want.append(O.ibd_scan_pair(sp["model"], full, v, sfrm, sto, pair_ordinal=r * N_WIN_PAIRS + first + v,
                                                want_mean=bool(flags & capi.FSMC_WANT_MEAN),
                                                want_map=bool(flags & capi.FSMC_WANT_MAP)))
        _oracle[flags] = np.concatenate(want)
        assert _oracle[flags].size > 60
    return _oracle[flags]


def _pooled_run(sp, monkeypatch, stride, flags, slots, resident, phi):
    _, pairs, groups = _work_list()
    monkeypatch.setenv("FSMC_DIAG_MAX_SLOTS", str(slots))
    ctx, model = _ctx(sp, stride, limit=_limit(sp, stride, slots, resident), chunk=CHUNK)
    ctx.set_pairing(0)
    ctx.set_chunk_pool(1, phi)
    got = ctx.decode_ibd(model, pairs, groups, flags)
    info, pool = ctx.info(), ctx.last_chunk_pool()
    assert info["n_slots"] == slots and info["max_chunks"] == 14
    assert ctx.last_resident_chunks() == resident
    ctx.close()
    assert pool["buffers"] == slots * resident
    assert pool["outstanding"] == 0
    assert pool["kept"] + pool["rebuilt"] == _multi_chunk_chunks(groups), pool
    assert got.tobytes() == _static_records(sp, stride, flags).tobytes()
    _assert_records_equal(got, _oracle_records(sp, flags))
    return pool


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("flags", [AGES, 0])
@pytest.mark.parametrize("phi", [100, 200, 700])
@pytest.mark.parametrize("slots", [1, 3])
def test_forced_pool_over_several_rounds(small_problem, monkeypatch, slots, phi, flags, stride):
    """Two buffers a wave of fourteen chunks a window; one wave that re-uses its buffers group after group, three that
    compete for six.  phi = 7 asks for every chunk: with three waves both paths -- kept and rebuilt -- run in one launch."""
    pool = _pooled_run(small_problem, monkeypatch, stride, flags, slots, 2, phi)
    assert pool["kept"] > 0
    if phi == 100:
        assert pool["kept"] <= 2 * REPS * len(WINS)  # (a window asks for its first two chunks only)
    if phi == 700 and slots == 3:
        assert pool["rebuilt"] > 0


@pytest.mark.parametrize("stride", [1, 2])
def test_starved_pool(small_problem, monkeypatch, stride):
    """Three buffers for three waves that each ask for all fourteen chunks of a window: most claims fail."""
    pool = _pooled_run(small_problem, monkeypatch, stride, AGES, 3, 1, 700)
    assert pool["rebuilt"] > pool["kept"] > 0


def test_pool_beside_the_paired_kernel(small_problem, monkeypatch):
    """With pairing left on, the half-full groups ride two to a wave in the paired kernel (static layout) and the others
    beside it on half the workspace, through the pool: the same records."""
    _, pairs, groups = _work_list()
    monkeypatch.setenv("FSMC_DIAG_MAX_SLOTS", "3")
    ctx, model = _ctx(small_problem, 2, limit=2 * _limit(small_problem, 2, 3, 2), chunk=CHUNK)
    ctx.set_chunk_pool(1, 700)
    got = ctx.decode_ibd(model, pairs, groups, AGES)
    pool = ctx.last_chunk_pool()
    ctx.close()
    assert pool["buffers"] > 0 and pool["outstanding"] == 0 and pool["kept"] > 0
    assert got.tobytes() == _static_records(small_problem, 2, AGES).tobytes()


@pytest.mark.parametrize("stride", [1, 2])
def test_sums_over_pairs_through_the_pool(small_problem, monkeypatch, stride):
    """decode_sums runs the same kernel path: two batches of two and three groups, a wave each, forced pool against pool
    off."""
    pm = small_problem["model"]
    pairs = _pairs_array(O.enumerate_all_pairs(32)[:300])
    groups = capi.whole_sequence_groups(300, pm.S)
    batches = np.array([0, 2, len(groups)], np.uint32)
    monkeypatch.setenv("FSMC_DIAG_MAX_SLOTS", "3")
    out = {}
    for mode in (0, 1):
        ctx, model = _ctx(small_problem, stride, limit=_limit(small_problem, stride, 3, 2), chunk=CHUNK)
        ctx.set_two_wave_windows(1)
        ctx.set_chunk_pool(mode, 700)
        ctx.upload_worklist(pairs, groups)
        out[mode] = ctx.decode_sums(model, major_minor=True, batch_first_group=batches)
        pool = ctx.last_chunk_pool()
        assert ctx.last_beta_stride() == stride and ctx.info()["max_chunks"] == 14
        ctx.close()
        assert pool["outstanding"] == 0
        assert (pool["buffers"] > 0 and pool["kept"] > 0 and pool["rebuilt"] > 0) if mode else pool["buffers"] == 0
    assert np.array_equal(out[1][0], out[0][0])
    for a, b in zip(out[1][1], out[0][1]):
        assert np.array_equal(a, b)


def test_static_layout_where_the_pool_does_not_apply(small_problem):
    """Left to itself (mode -1) a launch of one round keeps the static layout, and so does an explicit resident count in
    any mode: the plans test_gpu_resident_chunks.py expects."""
    _, pairs, groups = _work_list()
    ctx, model = _ctx(small_problem, 2, limit=_limit(small_problem, 2, len(groups), 2), chunk=CHUNK)
    ctx.set_pairing(0)
    ctx.set_chunk_pool(-1)
    got = ctx.decode_ibd(model, pairs, groups, AGES)
    assert ctx.info()["n_slots"] == len(groups)  # one round
    assert ctx.last_chunk_pool() == {"buffers": 0, "kept": 0, "rebuilt": 0, "outstanding": 0}
    assert ctx.last_resident_chunks() == 2
    ctx.close()
    assert got.tobytes() == _static_records(small_problem, 2, AGES).tobytes()
    for resident in (1, 2):
        ctx, model = _ctx(small_problem, 2, limit=64 << 20, chunk=CHUNK)
        ctx.set_pairing(0)
        ctx.set_chunk_pool(1)
        ctx.set_resident_chunks(resident)
        ctx.decode_ibd(model, pairs, groups, AGES)
        assert ctx.last_resident_chunks() == resident and ctx.last_chunk_pool()["buffers"] == 0
        ctx.close()
    ctx, model = _ctx(small_problem, 2, limit=1 << 30, chunk=CHUNK)  # every chunk resident: nothing to share
    ctx.set_pairing(0)
    ctx.set_chunk_pool(1)
    ctx.decode_ibd(model, pairs, groups, AGES)
    assert ctx.last_resident_chunks() == ctx.info()["max_chunks"] and ctx.last_chunk_pool()["buffers"] == 0
    ctx.close()


def test_chunk_pool_setting_is_validated(small_problem):
    ctx = capi.Context(0)
    for mode, phi in ((-2, 0), (2, 0), (1, 99), (1, 100001)):
        with pytest.raises(capi.FsmcError):
            ctx.set_chunk_pool(mode, phi)
    for mode, phi in ((-1, 0), (0, 0), (1, 100), (1, 100000)):
        ctx.set_chunk_pool(mode, phi)
    assert ctx.last_chunk_pool() == {"buffers": 0, "kept": 0, "rebuilt": 0, "outstanding": 0}
    ctx.close()
