"""Kernel parity at the numeric edges (tests/edge_models.py): subnormal and exactly-zero posteriors, states whose
emission is exactly 0 beside the ghost states of a padded member and on a wave boundary, bitwise ties between states
(the MAP's "first strictly larger wins" in every place it is implemented), an IBD probability exactly equal to the
scan's threshold, identical and complementary haplotypes.  Every consumer of every kernel family -- exact, padded,
wave-group and any-K members, array and sequence mode -- against the oracle, bit for bit."""
import functools

import numpy as np
import pytest

import edge_models as E
from conftest import expected_member
from fastsmc_amd import capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = [69, 50, 100, 33, 105]  # exact and padded members of the lane-per-pair family
WIDE = [200, 300, 402, 600, 1030]  # wave-group members (4x48, 4x80, 7x64, 8x80) and the any-K kernel
BUILDERS = {
    "subnormal-1e-30": lambda K, seq: E.subnormal(K, 1e-30, seq),
    "subnormal-1e-38": lambda K, seq: E.subnormal(K, 1e-38, seq),
    "zero-states": lambda K, seq: E.zero_states(K),
    "degenerate": lambda K, seq: E.degenerate(K, seq),
    "threshold-equal": lambda K, seq: E.threshold_equal(K),
    "identical-complement": lambda K, seq: E.identical_and_complement_pairs(K),
}
SEQ = [(b, K, True) for b in ("subnormal-1e-30", "degenerate") for K in (69, 200, 1030)]
SMALL_CASES = [(b, K, False) for K in SMALL for b in BUILDERS] + [c for c in SEQ if c[1] <= 128]
WIDE_CASES = [(b, K, False) for K in WIDE for b in BUILDERS] + [c for c in SEQ if c[1] > 128]
FIELDS = (("pair", "pair"), ("start", "start"), ("end", "end"), ("prob", "prob"), ("post_mean", "postMean"),
          ("map", "map"))
ALL_FLAGS = (capi.FSMC_WANT_MEAN | capi.FSMC_WANT_MAP, capi.FSMC_WANT_MAP, 0)


@functools.lru_cache(maxsize=4)
def _case(name, K, seq):
    """The builder's model and the oracle's answers: records of every pair for each flag set, and posterior, per-pair
    mean / MAP and sums (plain and 00 / 01 / 11) of the first group of 64 pairs."""
    pm, bits, folded, pairs = BUILDERS[name](K, seq)
    batches = E.oracle_posteriors(pm, folded, pairs)
    recs = []
    for b, (post, _, _) in enumerate(batches):
        for v in range(post.shape[2]):
            recs.append(O.ibd_scan_pair(pm, post, v, 0, pm.S, pair_ordinal=64 * b + v))
    recs = np.concatenate(recs)
    want = {ALL_FLAGS[0]: recs}
    want[capi.FSMC_WANT_MAP] = recs.copy()
    want[capi.FSMC_WANT_MAP]["postMean"] = 0.0  # (what the scan writes for a field it was not asked for)
    want[0] = want[capi.FSMC_WANT_MAP].copy()
    want[0]["map"] = 0.0
    post, ob, hb = batches[0]
    mean, mp, _ = O.per_pair_output(pm, post, 64)
    sums = [np.zeros((pm.S, pm.K), np.float32) for _ in range(4)]
    O.augment_sum_over_pairs(pm, post, 64, ob, hb, *sums)
    pr = np.array(pairs, dtype=np.uint32).view(capi.PAIR_DTYPE).reshape(-1)
    return pm, bits, pr, want, dict(post=post, mean=mean, map=mp, sums=sums)


def _assert_records(got, want, what):
    assert got.size == want.size, what
    for f_got, f_want in FIELDS:
        np.testing.assert_array_equal(got[f_got], want[f_want], err_msg=f"{f_got} {what}")


def _check(case, stride=0, chunk=0, resident=None, consumers=True, waves=None):
    name, K, seq = case
    pm, bits, pr, want, first = _case(name, K, seq)
    what = f"{name} K={K} seq={seq} stride={stride} chunk={chunk} resident={resident}"
    ctx = capi.Context(0)
    if stride:
        ctx.set_beta_stride(stride)
    if chunk:
        ctx.set_chunk_sites(chunk)
    if resident is not None:
        ctx.set_workspace_limit(1 << 30)
        ctx.set_resident_chunks(resident)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    groups = capi.whole_sequence_groups(len(pr), pm.S)
    for flags in ALL_FLAGS:
        got = ctx.decode_ibd(model, pr, groups, flags)
        assert ctx.last_kernel() == expected_member(K), what
        if stride:  # (sequence mode has no stride-2 kernels: chooseKernel, csrc/fsmc_capi.hip)
            assert ctx.last_beta_stride() == (1 if seq else stride), what
        if chunk:
            assert ctx.info()["max_chunks"] > 1, what
        if resident is not None:
            assert ctx.last_resident_chunks() > 0, what
        _assert_records(got, want[flags], f"{what} flags={flags}")
    if consumers:
        ctx.upload_worklist(pr[:64], capi.whole_sequence_groups(64, pm.S))
        post = ctx.decode_posteriors(model)[0]
        assert ctx.last_kernel() == expected_member(K), what
        np.testing.assert_array_equal(post, first["post"], err_msg=f"posterior {what}")
        mean, mp = ctx.decode_per_pair(model, pm.exp_times)
        assert ctx.last_kernel() == expected_member(K), what
        np.testing.assert_array_equal(mean, first["mean"], err_msg=f"per-pair mean {what}")
        np.testing.assert_array_equal(mp, first["map"], err_msg=f"per-pair MAP {what}")
        s, _ = ctx.decode_sums(model)
        assert ctx.last_kernel() == expected_member(K), what
        if waves is not None:
            assert ctx.last_waves_per_window() == waves, what
        np.testing.assert_array_equal(s, first["sums"][0], err_msg=f"sums {what}")
        s2, mm = ctx.decode_sums(model, major_minor=True)
        for got, w, part in zip((s2, *mm), first["sums"], ("sums", "00", "01", "11")):
            np.testing.assert_array_equal(got, w, err_msg=f"major/minor {part} {what}")
    ctx.close()


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: f"{c[0]}-K{c[1]}{'-seq' if c[2] else ''}")
def test_lane_per_pair_members_at_the_edges(case, window_waves):
    """Exact (69, 50, 100) and padded (33, 105) members: beta strides 1 and 2, two waves per window on and off (the
    fixture), the checkpoint / rebuild layout with 16-site chunks."""
    seq = case[2]
    waves = None if seq else (2 if window_waves == "two-waves-auto" else 1)
    for stride in (1, 2):
        _check(case, stride=stride, waves=waves)
    _check(case, chunk=16, consumers=False)


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: f"{c[0]}-K{c[1]}{'-seq' if c[2] else ''}")
def test_wave_group_and_any_k_kernels_at_the_edges(case):
    """Wave-group members (200: 4x48, 300: 4x80, 402: 7x64, 600: 8x80) and the any-K kernel (1030); 16-site chunks;
    resident chunks for the four-wave members that keep them (200, 300)."""
    _check(case)
    _check(case, chunk=16, consumers=False)
    if case[1] in (200, 300) and not case[2]:
        _check(case, chunk=48, resident=-1)
