"""The oracle against the float64 dense forward-backward (tests/dense_reference.py) beyond K = 69: 16, 128, 300, 600
and 1030 states, on the suite's benign generator and on the edge models of tests/edge_models.py (subnormal posteriors,
bitwise-degenerate posteriors).  Every GPU test trusts the oracle bit for bit; this is what the oracle is trusted
against.  Every output is checked: posterior, per-pair mean and MAP, sums over pairs and IBD records."""
import copy

import numpy as np
import pytest

import edge_models as E
from dense_reference import dense_posterior, dense_posterior_sequence
from oracle import oracle as O

# sites of the window checked against the dense chain (its K x K matrices are cached per table row)
SITES = {16: 400, 128: 400, 300: 160, 600: 80, 1030: 40}
N_DENSE_PAIRS = 8
CASES = [(K, name) for name in ("benign", "subnormal-1e-30", "degenerate") for K in SITES]


def _dense_tol(K, name):
    """Relative bound of the per-pair mean and the sums against the dense chain: 1e-5, except for the 1030 equal states
    of the degenerate model.  There the posterior's fp32 normalisation -- a sum of 1030 equal terms, up to ~K * 2^-24
    relative -- is off by 1.5e-5 (7.4e-6 at 600 states; at most 5e-6 in every other case)."""
    return 2e-5 if (name == "degenerate" and K == 1030) else 1e-5


def _truncate(pm, n):
    """The model restricted to its first n sites (a whole-sequence decode of a shorter chromosome)."""
    t = copy.copy(pm)
    t.S = n
    for name in ("step_row", "e1", "e0m1", "e2m0", "gen", "phys", "gap_row_f", "site_row_f", "gap_row_b",
                 "site_row_b", "hom"):
        a = getattr(pm, name)
        if a is not None:
            setattr(t, name, np.ascontiguousarray(a[:n]))
    return t


def _build(K, name):
    if name == "benign":
        return E.benign(K)
    if name == "subnormal-1e-30":
        return E.subnormal(K, 1e-30)
    return E.degenerate(K)


def _ibd_levels(pm, prob):
    """The four threshold levels of the scan (hmm_oracle.c, fo_ibd_scan_pair), as fp32 products."""
    t = np.float32(pm.probability_threshold)
    return np.array([np.float32(1000) * t, np.float32(100) * t, np.float32(10) * t, t], np.float64)


@pytest.mark.parametrize("K,name", CASES)
def test_oracle_matches_float64_at_edges(K, name):
    pm_full, _, folded, pairs = _build(K, name)
    S = SITES[K]
    pm = _truncate(pm_full, S)
    pairs = pairs[:N_DENSE_PAIRS]
    folded = np.ascontiguousarray(folded[:, :S])
    ob = np.stack([folded[a] ^ folded[b] for a, b in pairs])
    hb = np.stack([folded[a] & folded[b] for a, b in pairs])
    post, _ = O.decode_batch(pm, ob, hb, 0, S)
    mean, mp, _ = O.per_pair_output(pm, post, len(pairs))
    sums = np.zeros((S, K), np.float32)
    O.augment_sum_over_pairs(pm, post, len(pairs), ob, hb, sums)
    et = pm.exp_times.astype(np.float64)
    sum64 = np.zeros((S, K))
    near_map = near_ibd = 0
    for v in range(len(pairs)):
        ref = dense_posterior(pm, ob[v], hb[v], 0, S)
        got = post[:, :, v].astype(np.float64)
        sum64 += ref
        # posterior: absolute error, and relative error on the entries that matter
        assert np.max(np.abs(got - ref)) < 2e-5, (v, np.max(np.abs(got - ref)))
        big = ref > 1e-3  # (none for the 1030 equal terms of the degenerate model)
        assert not big.any() or np.max(np.abs(got[big] / ref[big] - 1.0)) < 1e-3
        if name == "degenerate":
            assert np.all(got == got[:, :1]), "exactly uniform over the real states"
        # per-pair posterior mean: the oracle's fp32 accumulation against float64 on its own posterior, and against the
        # dense chain's (_dense_tol)
        own = got @ et
        assert np.max(np.abs(mean[v] / own - 1.0)) <= 1e-5, np.max(np.abs(mean[v] / own - 1.0))
        m64 = ref @ et
        assert np.max(np.abs(mean[v] / m64 - 1.0)) <= _dense_tol(K, name), np.max(np.abs(mean[v] / m64 - 1.0))
        # per-pair MAP: the float64 argmax, except where the float64 top two are closer than 1e-5 relative
        top2 = np.sort(ref, axis=1)[:, -2:]
        close = (top2[:, 1] - top2[:, 0]) < 1e-5 * top2[:, 1]
        if name == "degenerate":
            assert np.all(mp[v] == 0)
        else:
            differ = mp[v] != np.argmax(ref, axis=1)
            assert not np.any(differ & ~close), np.nonzero(differ & ~close)
            near_map += int(np.count_nonzero(differ))
        # IBD records: the oracle's scan on the float64 posterior rounded to fp32 against the fp32 chain's, except
        # segments with a boundary site whose float64 IBD probability is within 1e-4 of a threshold level.  For the
        # degenerate model this excuses everything: every site's IBD probability is state_threshold / K, and so is
        # the probability threshold (the prior mass below the state threshold; the quantile discretisation gives
        # every state 1/K of it), so every site is near it -- that model's records are pinned by the GPU test (bit
        # for bit against the oracle), not here
        r32 = O.ibd_scan_pair(pm, post, v, 0, S, want_mean=False, want_map=False)
        r64 = O.ibd_scan_pair(pm, ref.astype(np.float32)[:, :, None], 0, 0, S, want_mean=False, want_map=False)
        p64 = ref[:, :pm.state_threshold].sum(axis=1)
        near = np.any(np.abs(p64[:, None] - _ibd_levels(pm, p64)[None, :]) < 1e-4, axis=1)
        seg32 = {(int(r["start"]), int(r["end"])) for r in r32}
        seg64 = {(int(r["start"]), int(r["end"])) for r in r64}
        for s0, s1 in seg32 ^ seg64:
            edge = [x for x in (s0 - 1, s0, s1, s1 + 1) if 0 <= x < S]
            assert np.any(near[edge]), (v, s0, s1)
            near_ibd += 1
    # sums over pairs: against float64 on the oracle's own posteriors (1e-5 relative) and on the dense chain's
    # (_dense_tol relative where the sum is > 1e-3; 2e-5 absolute per pair everywhere)
    own = post[:, :, :len(pairs)].astype(np.float64).sum(axis=2)
    pos = own > 0
    assert np.max(np.abs(sums[pos] / own[pos] - 1.0)) <= 1e-5
    big = sum64 > 1e-3
    assert np.max(np.abs(sums[big] / sum64[big] - 1.0)) <= _dense_tol(K, name)
    assert np.max(np.abs(sums - sum64)) < 2e-5 * len(pairs)
    print(f"K={K} {name}: MAP sites excused (float64 top two within 1e-5) {near_map}, IBD segments excused {near_ibd}")


@pytest.mark.parametrize("K", [69, 200])
@pytest.mark.parametrize("name", ["subnormal-1e-30", "degenerate"])
def test_oracle_sequence_mode_matches_float64_at_edges(K, name):
    builder = (lambda: E.subnormal(K, 1e-30, seq=True)) if name != "degenerate" else (lambda: E.degenerate(K, seq=True))
    pm_full, _, folded, pairs = builder()
    S = 120
    pm = _truncate(pm_full, S)
    folded = np.ascontiguousarray(folded[:, :S])
    pairs = pairs[:4]
    ob = np.stack([folded[a] ^ folded[b] for a, b in pairs])
    hb = np.stack([folded[a] & folded[b] for a, b in pairs])
    post, _ = O.decode_batch(pm, ob, hb, 0, S)
    for v in range(len(pairs)):
        ref = dense_posterior_sequence(pm, ob[v], hb[v], 0, S)
        got = post[:, :, v].astype(np.float64)
        assert np.max(np.abs(got - ref)) < 2e-5
        big = ref > 1e-3
        assert np.max(np.abs(got[big] / ref[big] - 1.0)) < 1e-3
        if name == "degenerate":
            assert np.all(got == got[:, :1]), "exactly uniform over the real states"


def _dense_T_by_loops(m, row):
    """dense_T as first written (tests/test_oracle_dense.py before the move): every column of the upper part a scalar
    product of the one to its left, and the row-ratio form checked row by row."""
    K = m.K
    D, B, U, RR, cR = (x.astype(np.float64) for x in (m.D[row], m.B[row], m.U[row], m.RR[row], m.col_ratios))
    T = np.zeros((K, K))
    for i in range(K):
        T[i, i] = D[i]
        T[i, :i] = B[:i]
    for i in range(K - 2, -1, -1):
        T[i, i + 1] = U[i]
        for j in range(i + 2, K):
            T[i, j] = T[i, j - 1] * cR[j - 1]
    for i in range(K - 2):
        np.testing.assert_allclose(T[i, i + 2:], RR[i] * T[i + 1, i + 2:], rtol=2e-5, atol=1e-30)
    return T


@pytest.mark.parametrize("K", [16, 69, 128])
def test_dense_transition_matrix_is_the_loop_form(K):
    """dense_T builds each row's upper part with np.cumprod (a sequential running product: 1030 states stay cheap);
    the matrix must be the loop form's, bit for bit, on every row the model uses."""
    from dense_reference import dense_T

    pm = E.benign(K)[0]
    for row in np.unique(pm.step_row[1:]):
        np.testing.assert_array_equal(dense_T(pm, int(row)), _dense_T_by_loops(pm, int(row)))
