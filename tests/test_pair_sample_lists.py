"""What tests/pair_sample_lists.py claims, shown on the CPU: its Philox is Philox4x32-10 and the library's integer text
gives the same words and uniforms; its forward vectors are the oracle's; its law is the exact joint posterior over the
paths of a tiny model, and two wrong samplers are told apart; its marginals are the oracle's posteriors at working size;
the inputs of the GPU tests reach the regimes those tests are there for; and the planner and the buffer layout of
fsmc_decode_pair_samples, run through tests/pair_samples_driver.cpp, give the literals below."""
import os
import subprocess

import numpy as np
import pytest

import pair_loglik_lists as LL
import pair_sample_lists as SL
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastsmc_amd", "csrc")

UNIFORM_CASES = [(0, 0, 0, 0, 0), (1, 2, 3, 4, 5), (2 ** 64 - 1, 63, 0, 63, 6759), (20261020, 5, 9, 1, 2), (7, 1, 2, 0, 3),
                 (2 ** 32, 4000000000, 1, 64, 2 ** 31)]

PLAN_TABLE = [
    # whole sequences where they fit; the rich case of the GPU test under its limits; the caller's chunk; too small
    ("planSamples S=700 nGroups=2 hard=1099511627776",
     "rc=0 chunk=700 chunkRows=700 maxChunks=1 resident=0 wsSlot=807552 slots=2 waves=1 bytes=25841664"),
    ("planSamples S=700 nGroups=2 hard=2097152",
     "rc=0 chunk=27 chunkRows=27 maxChunks=26 resident=0 wsSlot=61056 slots=2 waves=1 bytes=1953792"),
    ("planSamples S=700 nGroups=2 hard=1048576",
     "rc=0 chunk=27 chunkRows=27 maxChunks=26 resident=0 wsSlot=61056 slots=1 waves=1 bytes=976896"),
    ("planSamples S=700 nGroups=2 hard=614400", 'rc=-4 why="workspace limit too small for the forward rows of one wave"'),
    ("planSamples S=700 nGroups=2 chunkSites=150",
     "rc=0 chunk=150 chunkRows=150 maxChunks=5 resident=0 wsSlot=178560 slots=2 waves=1 bytes=5713920"),
    ("planSamples S=700 nGroups=2 chunkSites=5000",
     "rc=0 chunk=700 chunkRows=700 maxChunks=1 resident=0 wsSlot=807552 slots=2 waves=1 bytes=25841664"),
    # the soft budget halves long sequences only: 6760 sites, 2048 waves wanted, 24 GiB earned
    ("planSamples S=6760 nGroups=100000 hard=200000000000 soft=25769803776",
     "rc=0 chunk=423 chunkRows=423 maxChunks=16 resident=0 wsSlot=505728 slots=2048 waves=1 bytes=16571695104"),
    ("planSamples S=400 nGroups=100000 hard=200000000000 soft=1000000",
     "rc=0 chunk=400 chunkRows=400 maxChunks=1 resident=0 wsSlot=461952 slots=2048 waves=1 bytes=15137243136"),
    # members: a row is ceil(member / 4) KiB; one site
    ("planSamples S=129 member=16 nGroups=3", "rc=0 chunk=129 chunkRows=129 maxChunks=1 resident=0 wsSlot=33280 slots=3 waves=1 bytes=1597440"),
    ("planSamples S=129 member=128 nGroups=3 perCU=4 nCU=1",
     "rc=0 chunk=129 chunkRows=129 maxChunks=1 resident=0 wsSlot=266240 slots=3 waves=1 bytes=12779520"),
    ("planSamples S=1 nGroups=1", "rc=0 chunk=1 chunkRows=1 maxChunks=1 resident=0 wsSlot=2304 slots=1 waves=1 bytes=36864"),
    # the two callers of planReplay side by side at equal inputs (the second line of each pair stands above as well):
    # rows of 256 bytes a float4 group against 1 KiB, a smallest chunk of 2 sqrt(S) against sqrt(S)
    ("planViterbi S=700 nGroups=2 hard=2097152",
     "rc=0 chunk=175 chunkRows=175 maxChunks=4 resident=0 wsSlot=55008 slots=2 waves=1 bytes=1760256"),
    ("planViterbi S=700 nGroups=2 chunkSites=150",
     "rc=0 chunk=150 chunkRows=150 maxChunks=5 resident=0 wsSlot=48960 slots=2 waves=1 bytes=1566720"),
]
LAYOUT_TABLE = [
    ("layout 700 2 70", "groupBytes=89600 pairBytes=1400 rowsBytes=98000"),
    ("layout 65 3 200", "groupBytes=12480 pairBytes=195 rowsBytes=39000"),
    ("layout 65 3 7", "groupBytes=12480 pairBytes=195 rowsBytes=1368"),
    ("layout 1 1 1", "groupBytes=64 pairBytes=1 rowsBytes=4"),
    ("layout 6760 64 64", "groupBytes=27688960 pairBytes=432640 rowsBytes=27688960"),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samples_driver") / "pair_samples_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "pair_samples_driver.cpp")], check=True)

    def run(lines):
        return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                              check=True).stdout.splitlines()

    return run


# ---------------------------------------------------------------- the uniforms

def test_philox_known_answers(driver):
    for counter, key, want in SL.PHILOX_KNOWN:
        got = SL.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
        assert got.dtype == np.uint32 and got.tolist() == list(want)
    lines = driver(["philox " + " ".join(f"{v:x}" for v in c + k) for c, k, _ in SL.PHILOX_KNOWN])
    assert lines == [" ".join(f"{v:08x}" for v in want) for _, _, want in SL.PHILOX_KNOWN]


def test_uniforms_are_exact_and_below_one(driver):
    """u is a 24-bit integer times 2^-24: every value is a float32, the largest 1 - 2^-24; the library's text gives the
    restatement's bits."""
    u = SL.uniforms(3, 1, 2, np.arange(50000), 17)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, np.round(u.astype(np.float64) * 2.0 ** 24))
    assert np.float32(0xFFFFFF) * np.float32(2.0 ** -24) == np.float32(1.0 - 2.0 ** -24) < 1
    assert 0.49 < u.mean() < 0.51
    got = driver([f"uniform {s} {a} {b} {r} {t}" for s, a, b, r, t in UNIFORM_CASES])
    for (s, a, b, r, t), line in zip(UNIFORM_CASES, got):
        want = SL.uniforms(s, a, b, np.array([r]), t)[0]
        assert int(line.split()[0], 16) == int(want.view(np.uint32)), (s, a, b, r, t, line)
    # the four sites of a Philox call take its four words; the next site a new call
    out = SL.philox4x32_10(np.array([5, 9, 1, 2], np.uint64), np.array([7, 0], np.uint64))
    for t in range(20, 24):
        assert SL.uniforms(7, 1, 2, np.array([9]), t)[0] == np.float32(out[t & 3] >> 8) * np.float32(2.0 ** -24)


def test_forward_vectors_are_the_oracles():
    """delta of the restatement is pair_loglik_lists.forward's alpha, bit for bit the oracle's alphaFwd."""
    pm, _, folded, pairs, alpha = SL.problem("S200")
    assert np.array_equal(alpha[:, :, :8], LL.oracle_alpha_fwd(pm, folded, pairs[:8]))
    pm, _, folded, pairs, alpha = SL.problem("K20")
    assert np.array_equal(alpha[:, :, :8], LL.oracle_alpha_fwd(pm, folded, pairs[:8]))


# ---------------------------------------------------------------- the law

@pytest.fixture(scope="module")
def tiny():
    pm, _, folded, pair = SL.tiny_problem()
    assert pm.K == 3 and pm.S == 4
    assert abs(float(pm.col_ratios[1]) - 1) > 0.5  # (the product of column ratios matters)
    post = SL.dense_path_posterior(pm, folded, pair)
    assert post.size == 81 and abs(post.sum() - 1) < 1e-12
    return pm, folded, pair, post


def _statistic(tiny, seed, variant=None):
    pm, folded, pair, post = tiny
    states = SL.sample(pm, folded, [pair], SL.TINY_N, seed, variant)[0]
    stat, cells = SL.pearson(states, post)
    return stat, cells, SL.chi2_quantile_999(cells - 1)


@pytest.mark.parametrize("seed", SL.TINY_SEEDS)
def test_the_law_is_the_joint_posterior(tiny, seed):
    """100 000 paths of the tiny model against its exact path posterior: Pearson's statistic over the cells with
    expectation >= 5 below the 99.9th percentile of chi-squared.  Measured: 62.1, 65.3 and 80.4 over 60 cells (98.3)."""
    stat, cells, bound = _statistic(tiny, seed)
    print(f"seed {seed}: {stat:.1f} over {cells} cells, bound {bound:.1f}")
    assert cells >= 40 and stat < bound


@pytest.mark.parametrize("seed", SL.TINY_SEEDS)
@pytest.mark.parametrize("variant", ["B[i]", "no-cR"])
def test_wrong_samplers_fail_it(tiny, seed, variant):
    """B read at the predecessor, and the product of column ratios left out: both are far outside (measured: 8.4e5 and
    7.1e3)."""
    stat, cells, bound = _statistic(tiny, seed, variant)
    print(f"{variant}, seed {seed}: {stat:.1f} over {cells} cells, bound {bound:.1f}")
    assert stat >= bound


def test_wilson_hilferty_is_close():
    """The approximation that stands in for scipy: within 0.5 per cent of the tabulated percentiles at the degrees of
    freedom the test has (40 cells at the least)."""
    z = 3.090232306167813
    for dof, want in ((40, 73.402), (59, 98.324), (80, 124.839)):
        got = dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3
        assert abs(got - want) < 0.005 * want, (dof, got)
        assert abs(SL.chi2_quantile_999(dof) - want) < 0.005 * want


def test_marginals_at_working_size():
    """K = 69, 200 sites, 4 pairs, 4096 samples each: per site and state the frequency lies within 5 standard deviations
    (+ 2 / N) of the oracle's posterior."""
    pm, _, folded, pairs, alpha = SL.problem("S200")
    pairs = pairs[:SL.MARGINAL_PAIRS]
    N = SL.MARGINAL_N
    states = SL.sample(pm, folded, pairs, N, SL.MARGINAL_SEED, alpha=alpha[:, :, :len(pairs)])
    ob, hb = LL._pair_bits(folded, pairs)
    post = O.decode_batch(pm, ob, hb, 0, pm.S)[0].transpose(2, 1, 0)  # [pairs][K][S], normalised at every site
    assert np.abs(post.astype(np.float64).sum(axis=1) - 1).max() < 1e-5
    worst = 0.0
    for i in range(len(pairs)):
        f = np.stack([(states[i] == k).mean(axis=0) for k in range(pm.K)])  # [K][S]
        p = post[i].astype(np.float64)
        # (an fp32 posterior may exceed 1 by an ulp: no variance below zero)
        slack = 5 * np.sqrt(np.clip(p * (1 - p), 0, None) / N) + 2.0 / N
        worst = max(worst, float((np.abs(f - p) / slack).max()))
        assert (np.abs(f - p) <= slack).all(), (i, float((np.abs(f - p) - slack).max()))
    print(f"largest |f - p| as a share of its bound: {worst:.3f}")


# ---------------------------------------------------------------- what the GPU test's inputs reach

def _moves(states):
    prev, cur = states[..., :-1].astype(int), states[..., 1:].astype(int)
    return prev, cur


def test_regimes_of_the_gpu_inputs():
    rich = SL.case("rich", n=SL.RICH_N)[4]
    S = rich.shape[2]
    prev, cur = _moves(rich)
    below, stay, above = int((prev < cur).sum()), int((prev == cur).sum()), int((prev > cur).sum())
    print(f"rich: predecessors below {below}, equal {stay}, above {above}")
    assert min(below, stay, above) >= 1000  # all three kinds of predecessor, moves in both directions
    changed = (prev != cur).any(axis=(0, 1))  # [S - 1]: some sample changes state between t and t + 1
    planned = [SL.planned(S, 69, 2, limit)[0] for limit in SL.LIMITS_RICH_PLANNED]
    for C in [c for c in SL.CHUNKS_RICH if c] + planned + [64, 4]:  # chunk boundaries, haplotype words, Philox calls
        for b in range(C, S, C):
            assert changed[b - 1], (C, b)
    assert (rich == 0).any() and (rich == 68).any()
    # the 65-site case in the chunks of the GPU test: some sample changes state across every chunk boundary; one length is
    # no multiple of four and the last chunk is ragged in all of them
    prev, cur = _moves(SL.case("S65")[4])
    changed = (prev != cur).any(axis=(0, 1))
    for C in SL.CHUNKS_S65:
        for b in range(C, 65, C):
            assert changed[b - 1], (C, b)
    assert any(C % 4 for C in SL.CHUNKS_S65) and all(65 % C for C in SL.CHUNKS_S65)
    # at the sizes of the model cases states change too, in both directions; the smallest models reach both ends
    for name in ("K2", "K3", "K16", "K20", "K64", "K128", "K50", "K69", "K100"):
        pm, _, _, _, states = SL.case(name, first=70)
        if pm.K <= 3:
            assert (states == 0).any() and (states == pm.K - 1).any(), name
        prev, cur = _moves(states)
        assert (prev < cur).any() and (prev > cur).any() and (prev == cur).any(), name
    # K = 69 is the family's model whose column ratios are not 1: paths come from two and more states below
    pm = SL.problem("K69")[0]
    assert (np.abs(pm.col_ratios[:pm.K - 1] - 1) > 1e-3).any()
    prev, cur = _moves(SL.case("K69", first=70)[4])
    assert (cur - prev >= 2).sum() >= 100


def test_zero_sum_case_has_both_kinds():
    _, _, _, pairs, states, bad = SL.zero_sum_case()
    assert bad.any() and not bad.all() and states.shape[0] == len(pairs)


# ---------------------------------------------------------------- plan and layout

@pytest.mark.parametrize("case,want", PLAN_TABLE + LAYOUT_TABLE)
def test_plan_and_layout_table(driver, case, want):
    assert driver([case]) == [want]


def _fields(line):
    line = line.split(" why=")[0]
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def test_plan_invariants(driver):
    """The slot holds its rows and checkpoints; the chunks cover the sequence; the plan stays inside the budget it was
    given; the restated planner of the GPU test agrees."""
    cases = [f"planSamples S={S} member={m} nGroups={g} hard={hard}" for S in (1, 5, 129, 700, 6760)
             for m in (16, 69, 128) for g in (1, 2, 5000) for hard in (1 << 20, 1 << 24, 1 << 36)]
    for case, line in zip(cases, driver(cases)):
        kv = dict(t.split("=") for t in case.split()[1:])
        S, m, hard = int(kv["S"]), int(kv["member"]), int(kv["hard"])
        f = _fields(line)
        row = (m + 3) // 4 * 1024
        if f["rc"] != 0:
            c_min = max(1, int(np.ceil(np.sqrt(S))))
            assert f["rc"] == -4 and (c_min + -(-S // c_min)) * row > hard, case
            continue
        assert 1 <= f["chunk"] <= S and f["maxChunks"] == -(-S // f["chunk"]), case
        assert f["wsSlot"] * 16 == (f["chunk"] + f["maxChunks"]) * row, case
        assert f["bytes"] == f["wsSlot"] * 16 * f["slots"] <= hard, case
        assert 1 <= f["slots"] <= min(int(kv["nGroups"]), 256 * 8), case
        if int(kv["nGroups"]) <= 2:
            assert (f["chunk"], f["maxChunks"], f["slots"]) == SL.planned(S, m, int(kv["nGroups"]), hard), case


def test_layout_invariants(driver):
    cases = [f"layout {S} {n} {p}" for S in (1, 3, 65, 700) for n in (1, 3, 64) for p in (1, 7, 64, 200)]
    for case, line in zip(cases, driver(cases)):
        S, n, p = (int(v) for v in case.split()[1:])
        f = _fields(line)
        assert f["groupBytes"] == 64 * n * S and f["pairBytes"] == n * S
        assert f["rowsBytes"] % 4 == 0 and p * n * S <= f["rowsBytes"] < p * n * S + 4


def test_headers_are_free_of_the_device_runtime():
    for name in ("fsmc_philox.h", "fsmc_plan.h", "fsmc_pair_layout.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip_runtime" not in text and "hipError" not in text, name
