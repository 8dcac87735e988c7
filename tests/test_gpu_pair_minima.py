"""fsmc_decode_pair_minima on the GPU: per site the smallest posterior mean / MAP over the pairs of the work list and the
FIRST pair that has it (DecodePairsReturnStruct::finaliseCalculations, DecodePairsReturnStruct.hpp:105-118), computed on
the device without the [pairs][sites] rows crossing the bus.  Everything is np.array_equal against numpy's first argmin
of the oracle's rows (tests/pair_minima_lists.py; tests/test_pair_minima_lists.py shows what the list reaches)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_minima_lists as L
from conftest import expected_member
from fastsmc_amd import capi, synth
from oracle import oracle as O
from pair_common import (pairs_array as _pairs_array, upload as _upload, open_context as _open, gpu_context,
                         problem as _problem, example_files as _example_files, asmc as _asmc)

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu(small_problem):
    yield from gpu_context(small_problem)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = np.iinfo(np.int32).min


def _want(mean, mp, base=0):
    return L.first_minima(mean, base) + L.first_minima(mp, base)


def _assert_equal(got, want, msg=""):
    for name, g, w in zip(("min_mean", "argmin_mean", "min_map", "argmin_map"), got, want):
        assert g.dtype == w.dtype, (name, g.dtype, w.dtype)
        assert np.array_equal(g, w), f"{name} {msg}: {int((g != w).sum())} of {g.size} sites differ"


@pytest.fixture(scope="module")
def want_192(small_problem):
    mean, mp = L.rows_192(small_problem)
    return _want(mean, mp)


def test_minima_k69_both_kernels(small_problem, want_192, window_waves):
    # (a context opened here: the two-wave / one-wave choice of `window_waves` is read at every launch)
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)
    got = ctx.decode_pair_minima(model, pm.exp_times)
    assert ctx.last_kernel() == 69
    assert ctx.last_waves_per_window() == (2 if window_waves == "two-waves-auto" else 1)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_minima_slices() == 1
    _assert_equal(got, want_192, "against the oracle")
    # the same reduction of the library's own rows
    mean, mp = ctx.decode_per_pair(model, pm.exp_times)
    _assert_equal(got, _want(mean, mp), "against decode_per_pair's rows")
    ctx.close()


def test_slices_do_not_show(gpu, small_problem, want_192):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)
    for slice_groups, n_slices in ((1, 3), (2, 2), (0, 1)):
        ctx.set_pair_minima_slice(slice_groups)
        got = ctx.decode_pair_minima(model, pm.exp_times)
        assert ctx.last_pair_minima_slices() == n_slices
        _assert_equal(got, want_192, f"slice {slice_groups}")


@pytest.mark.parametrize("range_len,slice_groups", [(40, 0), (40, 2), (7, 1), (1, 0)])
def test_short_ranges_do_not_show(small_problem, want_192, monkeypatch, range_len, slice_groups):
    """Ranges of 40 pairs: five in the one slice of 192 pairs, boundaries at 40, 80, 120, 160 -- inside every group; with
    slices of two groups four and two.  Ranges of 7 in slices of one group; ranges of one pair."""
    monkeypatch.setenv("FSMC_DIAG_MINIMA_RANGE", str(range_len))
    ctx, model = _open(small_problem)
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)
    ctx.set_pair_minima_slice(slice_groups)
    got = ctx.decode_pair_minima(model, pm.exp_times)
    ctx.close()
    _assert_equal(got, want_192, f"ranges of {range_len}")


def test_one_chain_over_two_calls(gpu, small_problem, want_192):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192[:100])  # (ragged: 64 + 36)
    state = ctx.decode_pair_minima(model, pm.exp_times)
    mean, mp = L.rows_192(small_problem)
    _assert_equal(state, _want(mean[:100], mp[:100]), "first part")
    _upload(ctx, pm, L.PAIRS_192[100:])
    got = ctx.decode_pair_minima(model, pm.exp_times, pair_base=100, state=state)
    assert all(g is s for g, s in zip(got, state))
    _assert_equal(got, want_192, "two calls")


@pytest.mark.parametrize("slice_groups", [0, 1])
def test_a_carried_state_that_is_lower_or_equal_stays(gpu, small_problem, want_192, slice_groups):
    """The state of a chain over OTHER pairs (indices 3 and 5, before pair_base = 1000), built from the winners' own
    values: exactly equal to the list's minimum at sites 0, 3, 6, ..., just below it at sites 1, 4, 7, ... -- the carried
    value and index stay in both cases -- and above it at sites 2, 5, 8, ..., where the list's first winner takes over."""
    ctx, model = gpu
    pm = small_problem["model"]
    mean, mp = L.rows_192(small_problem)
    wmin_mean, _, wmin_map, _ = want_192
    s = np.arange(pm.S)
    cm = wmin_mean.copy()
    cm[s % 3 == 1] = np.nextafter(cm[s % 3 == 1], np.float32(-np.inf))
    cm[s % 3 == 2] = np.nextafter(cm[s % 3 == 2], np.float32(np.inf))
    cq = wmin_map.copy()
    cq[s % 3 == 1] -= 1
    cq[s % 3 == 2] += 1
    am = np.where(s % 2 == 0, 3, 5).astype(np.int32)
    aq = np.where(s % 2 == 0, 5, 3).astype(np.int32)
    want = L.continue_minima(cm, am, mean, 1000) + L.continue_minima(cq, aq, mp, 1000)
    for w_arg, carried in ((want[1], am), (want[3], aq)):  # (what the expectation itself says)
        assert np.array_equal(w_arg[s % 3 != 2], carried[s % 3 != 2]) and (w_arg[s % 3 == 2] >= 1000).all()
    _upload(ctx, pm, L.PAIRS_192)
    ctx.set_pair_minima_slice(slice_groups)
    got = ctx.decode_pair_minima(model, pm.exp_times, pair_base=1000, state=(cm.copy(), am.copy(), cq.copy(), aq.copy()))
    _assert_equal(got, want, "carried state")


def test_pair_base_zero_ignores_the_arrays(gpu, small_problem, want_192):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)
    state = (np.full(pm.S, np.nan, np.float32), np.full(pm.S, -7, np.int32), np.full(pm.S, -7, np.int32),
             np.full(pm.S, -7, np.int32))
    got = ctx.decode_pair_minima(model, pm.exp_times, pair_base=0, state=state)
    _assert_equal(got, want_192, "pair_base 0")


def test_mean_only_and_map_only(gpu, small_problem, want_192):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)
    m, am, q, aq = ctx.decode_pair_minima(model, pm.exp_times, want_map=False)
    assert q is None and aq is None
    assert np.array_equal(m, want_192[0]) and np.array_equal(am, want_192[1])
    m, am, q, aq = ctx.decode_pair_minima(model, pm.exp_times, want_mean=False)
    assert m is None and am is None
    assert np.array_equal(q, want_192[2]) and np.array_equal(aq, want_192[3])


def test_nothing_is_written_outside_the_outputs(gpu, small_problem, want_192):
    """Every output lies inside a band (NaN for the float array, INT_MIN for the int arrays) that must stay untouched."""
    ctx, model = gpu
    pm = small_problem["model"]
    guard = 256
    fbuf = np.full(pm.S + 2 * guard, np.nan, np.float32)
    ibufs = [np.full(pm.S + 2 * guard, INT_MIN, np.int32) for _ in range(3)]
    state = (fbuf[guard:guard + pm.S],) + tuple(b[guard:guard + pm.S] for b in ibufs)
    _upload(ctx, pm, L.PAIRS_192)
    got = ctx.decode_pair_minima(model, pm.exp_times, state=state)
    _assert_equal(got, want_192, "inside the band")
    assert np.isnan(fbuf[:guard]).all() and np.isnan(fbuf[guard + pm.S:]).all()
    for b in ibufs:
        assert (b[:guard] == INT_MIN).all() and (b[guard + pm.S:] == INT_MIN).all()


def _other_kernel_case(pm, bits, folded, n_pairs):
    """A list whose second group repeats pairs of the first (ties across the slice boundary), slices of one group."""
    base = O.enumerate_all_pairs(32)[:n_pairs]
    pairs = base[:64] + [base[i % 64] for i in range(5, 5 + n_pairs - 64)]
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.set_pair_minima_slice(1)
    got = ctx.decode_pair_minima(model, pm.exp_times)
    member, slices = ctx.last_kernel(), ctx.last_pair_minima_slices()
    ctx.close()
    assert member == expected_member(pm.K)
    assert slices == 2
    mean, mp = L.oracle_rows(pm, folded, pairs)
    _assert_equal(got, _want(mean, mp), f"K = {pm.K}, S = {pm.S}")


@pytest.mark.parametrize("K,S,n_pairs", [(40, 200, 96), (69, 37, 96), (200, 200, 96), (1030, 120, 70)])
def test_other_kernels(K, S, n_pairs):
    """A padded member with ghost states (40 -> 48; S = 200: a tail block of 8 sites), fewer sites than a wave (S = 37),
    the wave-group kernel (200 states), the any-K kernel (1030)."""
    pm, bits, folded = _problem(K, S=S)
    _other_kernel_case(pm, bits, folded, n_pairs)


def test_sequence_mode(seq_problem):
    _other_kernel_case(seq_problem["model"], seq_problem["bits"], seq_problem["folded"], 100)


def test_errors(gpu, small_problem, want_192):
    ctx, model = gpu
    pm = small_problem["model"]
    _upload(ctx, pm, L.PAIRS_192)

    def arrays():
        return (np.full(pm.S, 7.0, np.float32), np.full(pm.S, 7, np.int32), np.full(pm.S, 7, np.int32),
                np.full(pm.S, 7, np.int32))

    def untouched(st):
        return all(a is None or (a == 7).all() for a in st)

    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_minima(model, pm.exp_times, want_mean=False, want_map=False)
    assert ei.value.code == -1 and "at least one output" in str(ei.value)  # FSMC_EINVAL
    for keep in ((0,), (1,), (2,), (3,), (0, 1, 2), (0, 2, 3)):  # half of an output pair
        st = tuple(a if i in keep else None for i, a in enumerate(arrays()))
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_minima(model, pm.exp_times, state=st)
        assert ei.value.code == -1 and "come together" in str(ei.value), keep
        assert untouched(st)
    st = arrays()
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_minima(model, pm.exp_times, pair_base=2**31 - 10, state=st)
    assert ei.value.code == -1 and "int32" in str(ei.value)
    assert untouched(st)
    assert ctx.last_pair_minima_slices() == 0  # (nothing ran)
    groups = capi.whole_sequence_groups(len(L.PAIRS_192), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(L.PAIRS_192), groups)
    st = arrays()
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_minima(model, pm.exp_times, state=st)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value)
    assert untouched(st)
    # the context is usable afterwards
    _upload(ctx, pm, L.PAIRS_192)
    _assert_equal(ctx.decode_pair_minima(model, pm.exp_times), want_192, "after the errors")


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

def _four(res):
    return (np.array(res.min_posterior_means), np.array(res.argmin_posterior_means), np.array(res.min_MAPs),
            np.array(res.argmin_MAPs))


def _product_lists():
    rng = np.random.default_rng(3)
    all_pairs = [(x, y) for y in range(300) for x in range(y)]
    pick = rng.choice(len(all_pairs), 300, replace=False)
    plain = [all_pairs[i] for i in pick]
    repeated = plain[:150] + [plain[17]] + plain[150:200] + plain[:64]  # (265 pairs, 65 of them seen before)
    return {"300 pairs": plain, "a repeated pair": repeated}


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path_minima_equal_those_of_the_rows_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, min_posterior_means=True, min_MAPs=True) returns the four vectors of
    per_pair_posterior_means=True, per_pair_MAPs=True bit for bit, and no rows.  With FSMC_DIAG_FLUSH_PAIRS=128 the
    queue is decoded every 128 pairs: three flushes continue one chain (pair_base = pairs written so far)."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    asmc = _asmc(_example_files(tmp_path)[0])
    for name, pairs in _product_lists().items():
        a, b = [int(p[0]) for p in pairs], [int(p[1]) for p in pairs]
        asmc.decodePairs(a, b, per_pair_posterior_means=True, per_pair_MAPs=True)
        res = asmc.get_copy_of_results()
        want = _four(res)
        rows_mean, rows_map = np.array(res.per_pair_posterior_means), np.array(res.per_pair_MAPs)
        assert rows_mean.shape == rows_map.shape == (len(pairs), want[0].size)
        _assert_equal(want, _want(rows_mean, rows_map), name + ": the rows path itself")
        first, last = rows_map.argmin(0), len(pairs) - 1 - rows_map[::-1].argmin(0)
        if name == "a repeated pair":
            assert (first != last).any()  # (ties exist: the first winner is not the last)
        indices = res.per_pair_indices
        asmc.decodePairs(a, b, min_posterior_means=True, min_MAPs=True)
        res = asmc.get_copy_of_results()
        _assert_equal(_four(res), want, name)
        assert np.array(res.per_pair_posterior_means).size == 0 and np.array(res.per_pair_MAPs).size == 0
        assert res.per_pair_indices == indices
        # one of the two, by keyword, beside stored rows of the other kind
        asmc.decodePairs(a, b, per_pair_posterior_means=True, min_MAPs=True)
        res = asmc.get_copy_of_results()
        _assert_equal(_four(res), want, name + ": mean rows stored, MAP minima from the device")
        assert np.array(res.per_pair_MAPs).size == 0
        asmc.decodePairs(a, b, min_posterior_means=True)
        res = asmc.get_copy_of_results()
        assert np.array_equal(np.array(res.min_posterior_means), want[0])
        assert np.array_equal(np.array(res.argmin_posterior_means), want[1])
        assert np.array(res.min_MAPs).size == 0 and np.array(res.argmin_MAPs).size == 0


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from fastsmc_amd import api
root = sys.argv[2]


def vm(key):
    # VmRSS: the resident set at this moment; VmHWM: its peak since this program was started.  (ru_maxrss is no use
    # here: across fork and exec it keeps the peak of the process that started this one, the test run's.)
    for line in open("/proc/self/status"):
        if line.startswith(key + ":"):
            return int(line.split()[1]) * 1024
    raise KeyError(key)


ab = np.load(root + ".pairs.npy")
a, b = [int(x) for x in ab[0]], [int(x) for x in ab[1]]
p = api.DecodingParams(root, root + ".decodingQuantities.gz", root, 1, 1, "array", False, True, False, False, 0.0, False,
                       True, False, "", False, True)
p.useKnownSeed = True
asmc = api.ASMC(p)
asmc.decodePairs(a[:64], b[:64], min_posterior_means=True, min_MAPs=True)
# Start-up leaves the peak above what is resident now; rows held during the call could hide in that room.  Fill it.
room = vm("VmHWM") - vm("VmRSS")
ballast = np.ones(max(room, 0) // 8 + 1, np.float64)
before, resident = vm("VmHWM"), vm("VmRSS")
asmc.decodePairs(a, b, min_posterior_means=True, min_MAPs=True)
after = vm("VmHWM")
res = asmc.get_copy_of_results()
amean, amap = np.array(res.argmin_posterior_means), np.array(res.argmin_MAPs)
out = {"room_filled": room, "before": before, "after": after, "resident_before": resident, "sites": int(amean.size),
       "finite": bool(np.isfinite(np.array(res.min_posterior_means)).all()),
       "arg_lo": int(min(amean.min(), amap.min())), "arg_hi": int(max(amean.max(), amap.max())),
       "winners": int(np.unique(amean).size)}
del res
# the control: the same measure sees the rows when the call does hold them
asmc.decodePairs(a, b, per_pair_posterior_means=True, per_pair_MAPs=True)
out["after_rows_path"] = vm("VmHWM")
out["ballast"] = float(ballast[-1])
print(json.dumps(out))
"""


def test_product_path_minima_alone_do_not_hold_the_rows(tmp_path):
    """ASMC.decodePairs(a, b, min_posterior_means=True, min_MAPs=True) for 8192 pairs of a cohort of the C1 shape (300
    haplotypes x 6760 sites, K = 69), in a child process.  The mean and MAP rows the rows path holds for this call are
    8192 x 6760 x 8 B = 443 MB; the peak resident set of the process may grow by less than a QUARTER of that over the
    call (what it needs on the host is four [sites] vectors, 108 kB, and the pair list with its indices).  The child
    reads its own peak (VmHWM), fills the room that start-up left between the peak and the resident set before the
    call, so that rows held during the call cannot hide in it, and then makes the same call with the rows stored: there
    the same measure must grow by the rows at least."""
    n_hap, S, n_pairs = 300, 6760, 8192
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(n_hap, S, seed=1234)
    root = str(tmp_path / "cohort")
    synth.write_haps_files(root, haps, fastsmc_map=False)
    gen_file = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
    gen_synth = (haps.cm / 100.0).astype(np.float32)
    t = copy.copy(tables)
    used = np.unique(np.concatenate([[0.0], O.step_rows(t.keys, gen_file)[1][1:], O.step_rows(t.keys, gen_synth)[1][1:]]))
    sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
    t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)
    all_pairs = [(x, y) for y in range(n_hap) for x in range(y)][:n_pairs]
    np.save(root + ".pairs.npy", np.array([[p[0] for p in all_pairs], [p[1] for p in all_pairs]], np.int64))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    rows_bytes = n_pairs * S * 8
    growth = stats["after"] - stats["before"]
    above_start = stats["after"] - stats["resident_before"]
    growth_rows_path = stats["after_rows_path"] - stats["after"]
    print(f"peak resident set: {stats['before']} -> {stats['after']} bytes (+{growth}), {above_start} above the set "
          f"resident at the start of the call ({stats['resident_before']}; {stats['room_filled']} of room filled); the "
          f"rows would be {rows_bytes}; with the rows stored the peak grows by {growth_rows_path}")
    assert growth < rows_bytes // 4
    assert above_start < rows_bytes // 4
    assert growth_rows_path >= rows_bytes
    assert stats["sites"] == S and stats["finite"]
    assert 0 <= stats["arg_lo"] and stats["arg_hi"] < n_pairs
    assert stats["winners"] > 1
