"""The numpy statement of fsmc_decode_pair_transitions (tests/pair_transition_lists.py) on the CPU: its backward vector
is the oracle's, its values are probabilities, it agrees with the fp64 two-slice posterior on the dense transition
matrices, that yardstick is consistent with the posterior itself, and the inputs of the GPU test reach their regimes."""
import numpy as np
import pytest

import pair_transition_lists as TL
from oracle import oracle as O
from pair_common import posterior_tables
from pair_loglik_lists import _pair_bits, forward

F32 = np.float32
EPS = F32(8 * 2.0 ** -24)  # z, r and the two products are rounded once each: (down + up) / z <= 1 picks up five half-ulps


@pytest.mark.parametrize("name", ["K3", "K20", "K69", "K128", "S2"])
def test_backward_vector_is_the_oracles(name):
    """beta of the statement equals the oracle's beta buffer bit for bit, and delta * beta, summed over the states
    ascending and scaled by 1.0f / sum, times the expected times, equals the oracle's posterior tables: the backward
    order (BL + D * vec) + BU and the first scaling over the model's K are the reference's."""
    pm, _, folded, pairs, alpha = TL.problem(name)
    pairs = pairs[:70]
    alpha = alpha[:, :, :70]
    _, _, beta = TL.transitions(pm, folded, pairs, alpha=alpha)
    want = []
    for b0 in range(0, len(pairs), 64):
        ob, hb = _pair_bits(folded, pairs[b0:b0 + 64])
        want.append(O.decode_batch(pm, ob, hb, 0, pm.S)[1])
    assert np.array_equal(beta, np.concatenate(want, axis=2))
    post = alpha * beta  # [S][K][n]
    s = np.zeros((pm.S, len(pairs)), F32)
    for k in range(pm.K):
        s = s + post[:, k, :]
    post = (post * (F32(1.0) / s)[:, None, :]) * pm.exp_times.astype(F32)[None, :, None]
    assert post.dtype == F32
    rows, _ = posterior_tables(pm, folded, pairs)
    assert np.array_equal(post.transpose(2, 1, 0), rows)


@pytest.mark.parametrize("name", TL.MODEL_CASES + TL.SITE_CASES + ("S65", "rich"))
def test_values_are_probabilities(name):
    _, _, _, _, down, up = TL.case(name)
    assert down.dtype == up.dtype == F32
    assert np.isfinite(down).all() and np.isfinite(up).all()
    assert (down >= 0).all() and (up >= 0).all()
    assert (down + up <= F32(1.0) + EPS).all(), float((down + up).max())
    assert not down[:, 0].any() and not up[:, 0].any()


def test_statement_agrees_with_dense_and_dense_with_itself(capsys):
    """The largest difference between the fp32 statement and the fp64 two-slice posterior, printed and bounded by four
    times the figure measured when the lists were written; and the yardstick itself: the two-slice table of (t-1, t)
    summed over the state of site t is the posterior of site t-1."""
    worst = 0.0
    for name in TL.YARDSTICK:
        pm, _, folded, pairs, down, up = TL.case(name)
        for i in range(TL.YARDSTICK_PAIRS):
            d64, u64, rows, post = TL.dense_transitions(pm, folded, pairs[i])
            assert np.allclose(rows[1:], post[:-1], rtol=0, atol=1e-12), name
            assert (d64 >= 0).all() and (u64 >= 0).all() and (d64 + u64 <= 1 + 1e-12).all()
            diff = max(np.abs(down[i] - d64).max(), np.abs(up[i] - u64).max())
            worst = max(worst, float(diff))
    with capsys.disabled():
        print(f"\nlargest |statement - fp64 yardstick| = {worst:.3e} (bound {TL.YARDSTICK_BOUND:.3e})")
    assert worst <= TL.YARDSTICK_BOUND


def test_inputs_reach_their_regimes():
    S = TL.CASES["rich"][1]
    edges = {C: set(range(C, S, C)) for C in TL.CHUNKS_RICH}  # the first sites of the chunks behind the first
    assert any(1 in e for e in edges.values()), "a chunk edge at t = 1: the row of t - 1 is a checkpoint"
    assert any(S - 1 in e for e in edges.values()), "a chunk edge at S - 1: the first step of the walk reads a checkpoint"
    assert any(not e for e in edges.values()), "one chunk: no second sweep"
    assert any(e and S % C for C, e in edges.items()), "a ragged last chunk"
    # a move that cannot happen has probability exactly 0: upwards out of a top state that holds everything, downwards
    # out of state 0
    _, _, _, _, down, up, het, (lo, hi) = TL.dominant_case()
    assert het[:, 0].any() and het[:, 1].any() and not het[:, 0].all() and not het[:, 1].all()
    assert np.isfinite(down).all() and np.isfinite(up).all()
    assert not up[het[:, 0], lo].any() and not down[het[:, 0], lo + 1].any()  # state 0 holds everything at site lo
    assert (down[het[:, 0], lo] > 0).all() and (up[het[:, 0], lo + 1] > 0).all()
    assert not down[het[:, 1], hi].any() and not up[het[:, 1], hi + 1].any()  # the top state at site hi
    assert (up[het[:, 1], hi] > 0).all() and (down[het[:, 1], hi + 1] > 0).all()
    assert (up[~het[:, 0], lo] > 0).all() and (down[~het[:, 1], hi] > 0).all()
    moving = 0
    for name in TL.MODEL_CASES + ("rich",):
        _, _, _, _, down, up = TL.case(name)
        moving += int(((down[:, 1:] > 0.25) | (up[:, 1:] > 0.25)).sum())
    assert moving > 0, "sites where a change is likely"
    # the bins: a one-site bin, bins of 64 and 65 sites, edges at no multiple of four, the whole sequence
    widths = {k: np.diff(e) for k, e in TL.EDGES.items()}
    assert (widths["single"] == 1).all() and 1 in widths["odd"] and (TL.EDGES["odd"] % 4 != 0).any()
    assert list(widths["w64_65"]) == [64, 65, 64] and list(TL.EDGES["whole"]) == [0, 200]


def test_bin_sums_follow_the_definition():
    """bin_sums() vectorises over pairs; here the definition is followed literally for a few cells, a one-site bin is the
    row's value itself, and the fp64 order is not the fp32 running sum."""
    _, _, _, _, down, up = TL.case("S200")
    single = TL.bin_sums(down, TL.EDGES["single"])
    assert np.array_equal(single, down)
    differs = 0
    for rows in (down, up):
        for key in ("w64_65", "odd", "whole"):
            e = TL.EDGES[key]
            got = TL.bin_sums(rows[:3], e)
            for i in range(3):
                for b in range(len(e) - 1):
                    lo, hi = int(e[b]), int(e[b + 1])
                    a = [np.float64(0.0)] * 64
                    for j in range(64):
                        for t in range(lo + j, hi, 64):
                            a[j] = a[j] + np.float64(rows[i, t])
                    for stride in (32, 16, 8, 4, 2, 1):
                        for j in range(stride):
                            a[j] = a[j] + a[j + stride]
                    assert got[i, b] == F32(a[0]), (key, i, b)
                    run = F32(0.0)
                    for t in range(lo, hi):
                        run = run + rows[i, t]
                    differs += int(run != got[i, b])
    assert differs > 0


# ---------------------------------------------------------------- the layout of the device buffers

def test_layout_invariants(tmp_path):
    """layout::transitions (fsmc_pair_layout.h) on the CPU: both directions' rows start on 16 bytes and hold the slice's
    pairs; edges, the S ones and the cells of both directions follow each other without overlap; a group's share of the
    buffers is what the slice planner divides by."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pair_transitions_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "fastsmc_amd", "csrc"), "-o", exe,
                    os.path.join(root, "tests", "pair_transitions_driver.cpp")], check=True)
    cases = [f"layout {S} {B} {p}" for S in (1, 3, 65, 700) for B in (0, 1, 5, 700) for p in (1, 7, 64, 200)]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True).stdout
    for case, line in zip(cases, out.splitlines()):
        S, B, p = (int(v) for v in case.split()[1:])
        f = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        assert f["rowsPerOut"] % 4 == 0 and p <= f["rowsPerOut"] < p + 4, case
        assert f["rowsBytes"] == 2 * f["rowsPerOut"] * S * 4 and (f["rowsPerOut"] * S * 4) % 16 == 0, case
        assert f["groupBytes"] == 64 * 2 * 4 * (S + B), case
        assert f["outBytes"] == 2 * f["rowsPerOut"] * B * 4, case
        if B:
            assert f["offEdges"] == 0 and f["offWeights"] >= (B + 1) * 4 and f["offWeights"] % 8 == 0, case
            assert f["offBins"] >= f["offWeights"] + S * 4 and f["offBins"] % 8 == 0, case
        assert f["accBytes"] == f["offBins"] + f["outBytes"], case
        if p <= 64:
            assert f["rowsBytes"] + f["outBytes"] <= f["groupBytes"], case
