"""fsmc_decode_pair_posteriors on the GPU against the oracle, bit for bit: per pair a [K][S] table of posterior x
expected coalescence time, and the sum of those tables over the pairs in pair order (HMM::writePerPairOutput,
HMM.cpp:1378-1392; the tables ASMC::decodePairs hands out, ASMC.cpp:80-128).  Expected values: O.decode_batch per batch
of 64 pairs, then O.per_pair_output with one accumulator carried across the batches."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import expected_member
from fastsmc_amd import api, capi, synth
from oracle import oracle as O
from pair_common import (pairs_array as _pairs_array, posterior_tables as _oracle, problem as _problem,
                         upload as _upload)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


PAIRS_150 = O.enumerate_all_pairs(32)[100:100 + 150]  # three groups, the last with 22 pairs


@pytest.fixture(scope="module")
def want_150(small_problem):
    return _oracle(small_problem["model"], small_problem["folded"], PAIRS_150)


@pytest.fixture
def gpu(small_problem, window_waves):
    # (a context per test: the two-wave / one-wave choice of `window_waves` is read at every launch)
    ctx = capi.Context(0)
    model = ctx.create_model(small_problem["model"])
    ctx.upload_haps(small_problem["bits"], small_problem["model"].S)
    yield ctx, model
    ctx.close()


def test_rows_and_sum_k69(gpu, small_problem, want_150, window_waves):
    ctx, model = gpu
    pm = small_problem["model"]
    wrows, wsum = want_150
    _upload(ctx, pm, PAIRS_150)
    rows, s = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=np.zeros((pm.K, pm.S), np.float32))
    assert ctx.last_kernel() == 69
    assert ctx.last_waves_per_window() == (2 if window_waves == "two-waves-auto" else 1)
    assert ctx.last_kernel_ms() > 0
    assert rows.shape == (150, pm.K, pm.S)
    np.testing.assert_array_equal(rows, wrows)
    np.testing.assert_array_equal(s, wsum)
    # the sum alone
    rows2, s2 = ctx.decode_pair_posteriors(model, pm.exp_times, want_rows=False,
                                           sum_into=np.zeros((pm.K, pm.S), np.float32))
    assert rows2 is None
    np.testing.assert_array_equal(s2, wsum)
    # the rows alone
    rows3, s3 = ctx.decode_pair_posteriors(model, pm.exp_times)
    assert s3 is None
    np.testing.assert_array_equal(rows3, wrows)


def test_the_chain_continues_across_calls(gpu, small_problem, want_150):
    ctx, model = gpu
    pm, folded = small_problem["model"], small_problem["folded"]
    _, wsum = want_150
    acc = np.zeros((pm.K, pm.S), np.float32)
    _upload(ctx, pm, PAIRS_150[:100])
    _, got = ctx.decode_pair_posteriors(model, pm.exp_times, want_rows=False, sum_into=acc)
    assert got is acc
    _upload(ctx, pm, PAIRS_150[100:])
    ctx.decode_pair_posteriors(model, pm.exp_times, want_rows=False, sum_into=acc)
    np.testing.assert_array_equal(acc, wsum)
    # a non-zero start: the oracle's accumulator after some other batch
    other = O.enumerate_all_pairs(32)[400:430]
    _, start = _oracle(pm, folded, other)
    assert np.count_nonzero(start) > 0
    acc = start.copy()
    _upload(ctx, pm, PAIRS_150[:70])
    rows, _ = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=acc)
    wrows, want = _oracle(pm, folded, PAIRS_150[:70], acc=start.copy())
    np.testing.assert_array_equal(acc, want)
    np.testing.assert_array_equal(rows, wrows)


def test_slices_do_not_show(gpu, small_problem, want_150):
    ctx, model = gpu
    pm = small_problem["model"]
    wrows, wsum = want_150
    _upload(ctx, pm, PAIRS_150)
    for slice_groups, n_slices in ((1, 3), (2, 2), (0, None)):
        ctx.set_pair_posterior_slice(slice_groups)
        rows, s = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=np.zeros((pm.K, pm.S), np.float32))
        if n_slices is None:
            assert ctx.last_pair_posterior_slices() >= 1
        else:
            assert ctx.last_pair_posterior_slices() == n_slices
        np.testing.assert_array_equal(rows, wrows, err_msg=f"slice {slice_groups}")
        np.testing.assert_array_equal(s, wsum, err_msg=f"slice {slice_groups}")


@pytest.mark.parametrize("copy_bytes,slice_groups", [(529920, 1), (529920, 0), (1000, 1)])
def test_short_row_copies_do_not_show(small_problem, want_150, monkeypatch, copy_bytes, slice_groups):
    """Pinned buffers of 529920 bytes, three tables of 69 x 640 floats: a slice of 64 pairs leaves in 22 copies, the
    last of one pair, the slice of 22 pairs in 8, the last of one pair; the automatic slice, all 150 pairs, in 50 full
    copies.  1000 bytes are less than one table: one pair a copy."""
    monkeypatch.setenv("FSMC_DIAG_ROW_COPY_BYTES", str(copy_bytes))
    ctx = capi.Context(0)
    pm = small_problem["model"]
    model = ctx.create_model(pm)
    ctx.upload_haps(small_problem["bits"], pm.S)
    _upload(ctx, pm, PAIRS_150)
    ctx.set_pair_posterior_slice(slice_groups)
    rows, s = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=np.zeros((pm.K, pm.S), np.float32))
    slices = ctx.last_pair_posterior_slices()
    ctx.close()
    assert slices == (3 if slice_groups else 1)
    wrows, wsum = want_150
    np.testing.assert_array_equal(rows, wrows)
    np.testing.assert_array_equal(s, wsum)


@pytest.mark.parametrize("K,S,n_pairs", [(40, 200, 96), (200, 200, 96), (1030, 120, 70)])
def test_other_kernels(K, S, n_pairs):
    """A padded member with ghost states (40 -> 48), the wave-group kernel (200 states), the any-K kernel (1030)."""
    pm, bits, folded = _problem(K, S=S)
    pairs = O.enumerate_all_pairs(32)[:n_pairs]
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.set_pair_posterior_slice(1)  # (two slices: the second starts inside the resident group list)
    rows, s = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=np.zeros((pm.K, pm.S), np.float32))
    assert ctx.last_kernel() == expected_member(K)
    assert ctx.last_pair_posterior_slices() == 2
    ctx.close()
    wrows, wsum = _oracle(pm, folded, pairs)
    np.testing.assert_array_equal(rows, wrows)
    np.testing.assert_array_equal(s, wsum)


def test_sequence_mode(seq_problem):
    pm, folded = seq_problem["model"], seq_problem["folded"]
    pairs = O.enumerate_all_pairs(32)[:100]
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(seq_problem["bits"], pm.S)
    _upload(ctx, pm, pairs)
    rows, s = ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=np.zeros((pm.K, pm.S), np.float32))
    assert ctx.last_kernel() == expected_member(pm.K)
    ctx.close()
    wrows, wsum = _oracle(pm, folded, pairs)
    np.testing.assert_array_equal(rows, wrows)
    np.testing.assert_array_equal(s, wsum)


@pytest.mark.parametrize("S", [100, 50])
def test_tail_block_writes_nothing_outside_the_tables(S):
    """S = 100: a full block of 64 sites and a tail of 36; S = 50: one short block.  Every output lies inside a band
    of NaN that must stay untouched."""
    pm, bits, folded = _problem(69, S=S, seed=3)
    pairs = O.enumerate_all_pairs(32)[:70]
    n, plane, guard = len(pairs), pm.K * pm.S, 256
    buf = np.full((n, plane + 2 * guard), np.nan, np.float32)
    rows_out = [buf[i, guard:guard + plane] for i in range(n)]
    sbuf = np.full(plane + 2 * guard, np.nan, np.float32)
    acc = sbuf[guard:guard + plane].reshape(pm.K, pm.S)
    acc[:] = 0.0
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    _upload(ctx, pm, pairs)
    ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=acc, rows_out=rows_out)
    ctx.close()
    wrows, wsum = _oracle(pm, folded, pairs)
    np.testing.assert_array_equal(buf[:, guard:guard + plane].reshape(n, pm.K, pm.S), wrows)
    np.testing.assert_array_equal(acc, wsum)
    assert np.isnan(buf[:, :guard]).all() and np.isnan(buf[:, guard + plane:]).all()
    assert np.isnan(sbuf[:guard]).all() and np.isnan(sbuf[guard + plane:]).all()


def test_errors(small_problem):
    pm = small_problem["model"]
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(small_problem["bits"], pm.S)
    _upload(ctx, pm, PAIRS_150)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_posteriors(model, pm.exp_times, want_rows=False, sum_into=None)
    assert ei.value.code == -1 and "at least one output" in str(ei.value)  # FSMC_EINVAL
    assert ctx.last_pair_posterior_slices() == 0  # (nothing ran)
    groups = capi.whole_sequence_groups(len(PAIRS_150), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(PAIRS_150), groups)
    acc = np.full((pm.K, pm.S), 7.0, np.float32)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_posteriors(model, pm.exp_times, sum_into=acc)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value)
    assert ctx.last_pair_posterior_slices() == 0 and (acc == 7.0).all()
    with pytest.raises(capi.FsmcError):
        ctx.last_kernel_ms()  # no launch has been timed in this context
    ctx.close()


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

_CHILD = r"""
import json, resource, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from fastsmc_amd import api
root, out = sys.argv[2], sys.argv[3]
ab = np.load(root + ".pairs.npy")
a, b = [int(x) for x in ab[0]], [int(x) for x in ab[1]]
p = api.DecodingParams(root, root + ".decodingQuantities.gz", root, 1, 1, "array", False, True, False, False, 0.0, False,
                       True, False, "", False, True)
p.useKnownSeed = True
asmc = api.ASMC(p)
peak = lambda: resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024  # (Linux: kilobytes)
asmc.decodePairs(a[:64], b[:64], False, True, False, False)
before = peak()
asmc.decodePairs(a, b, False, True, False, False)
after = peak()
total = np.array(asmc.get_copy_of_results().sum_of_posteriors)
asmc.decodePairs(a[:256], b[:256], False, True, False, False)
np.save(out, np.array(asmc.get_copy_of_results().sum_of_posteriors))
print(json.dumps({"before": before, "after": after, "total_finite": bool(np.isfinite(total).all()),
                  "total_mass": float(total.sum())}))
"""


def test_product_path_sum_only_does_not_hold_the_dump(tmp_path):
    """ASMC.decodePairs(a, b, False, True, False, False) for 2048 pairs of a 128-haplotype x 2000-site cohort, K = 69, in
    a child process.  The dump in the reference's batch layout that the host path used to allocate for this call is
    32 groups x 64 x 69 x 2000 x 4 B = 1.13 GB; the peak resident set of the process may grow by less than HALF of that
    over the call (what the call needs on the host is the [K][S] sum, 552 kB, the per-pair mean / MAP staging of
    writePerPairOutput, 2 x 16 MB, and the pair list).  The sum of the first 256 pairs, decoded alone in a second
    call, equals the oracle's (measured on the CPU: the oracle takes 1.05 s for those 256 pairs, so about 8.4 s for
    all 2048 -- left out of the test's run time)."""
    n_hap, S, n_pairs = 128, 2000, 2048
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(n_hap, S, seed=17, cm_per_mb=25.0, switch_per_cm=0.6)
    _, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    root = str(tmp_path / "cohort")
    synth.write_haps_files(root, haps, fastsmc_map=False)
    # the decoding quantities file with the rows the genetic map uses (ASMC mode reads gen = stof(cM) / 100.f)
    gen_file = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
    gen_synth = (haps.cm / 100.0).astype(np.float32)
    t = copy.copy(tables)
    used = np.unique(np.concatenate([[0.0], O.step_rows(t.keys, gen_file)[1][1:], O.step_rows(t.keys, gen_synth)[1][1:]]))
    sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
    t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)
    rng = np.random.default_rng(5)
    all_pairs = [(x, y) for x in range(n_hap) for y in range(x + 1, n_hap)]
    pick = rng.choice(len(all_pairs), n_pairs, replace=False)
    a = [all_pairs[i][0] for i in pick]
    b = [all_pairs[i][1] for i in pick]
    np.save(root + ".pairs.npy", np.array([a, b], np.int64))
    out = str(tmp_path / "sum256.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, root, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    dump_bytes = 32 * 64 * 69 * S * 4
    growth = stats["after"] - stats["before"]
    print(f"peak resident set: {stats['before']} -> {stats['after']} bytes (+{growth}); the dump would be {dump_bytes}")
    assert growth < dump_bytes // 2
    assert stats["total_finite"]
    # every column of a pair's posterior sums to one before the multiplication: the whole call's sum is not empty
    assert stats["total_mass"] > 0
    # the oracle on the data as the ASMC-mode readers see it
    p = api.DecodingParams(root, root + ".decodingQuantities.gz")
    p.useKnownSeed = True
    data = api.Data(p)
    gen = np.array(data.geneticPositions, np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, n_hap, time=p.time, no_conditional_age_estimates=False)
    _, want = _oracle(pm, folded, list(zip(a[:256], b[:256])))
    np.testing.assert_array_equal(np.load(out), want)
