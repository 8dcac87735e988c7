"""Structural check of the oracle against an independent statement of the same HMM: build the dense K x K
transition matrix from (D, B, U, rowRatios, columnRatios) (Transition.java:152-209) and run a
textbook float64 forward-backward.  The O(K) recurrences of the oracle must give the same posterior."""
import numpy as np

from dense_reference import dense_posterior, dense_posterior_sequence
from oracle import oracle as O


def test_oracle_matches_dense_float64(small_problem):
    m = small_problem["model"]
    folded = small_problem["folded"]
    pairs = [(0, 1), (3, 10), (5, 62), (20, 21)]
    for frm, to in ((0, m.S), (100, 400)):
        ob = np.stack([(folded[a] ^ folded[b])[frm:to] for a, b in pairs])
        hb = np.stack([(folded[a] & folded[b])[frm:to] for a, b in pairs])
        post, _ = O.decode_batch(m, ob, hb, frm, to)
        for v in range(len(pairs)):
            ref = dense_posterior(m, ob[v], hb[v], frm, to)
            got = post[frm:to, :, v].astype(np.float64)
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-5)
            assert np.max(np.abs(got - ref)) < 2e-5
            big = ref > 1e-3
            assert np.max(np.abs(got[big] / ref[big] - 1.0)) < 1e-3


def test_lanes_are_independent(small_problem):
    """A pair's result must not depend on batch composition or batch size (lane = pair)."""
    m = small_problem["model"]
    folded = small_problem["folded"]
    pairs = [(0, 1), (3, 10), (5, 62), (20, 21), (7, 9), (11, 40), (2, 33), (8, 50)]
    ob = np.stack([folded[a] ^ folded[b] for a, b in pairs])
    hb = np.stack([folded[a] & folded[b] for a, b in pairs])
    post8, _ = O.decode_batch(m, ob, hb, 0, m.S)
    post4, _ = O.decode_batch(m, ob[4:], hb[4:], 0, m.S)
    np.testing.assert_array_equal(post8[:, :, 4:], post4)


def test_oracle_sequence_mode_matches_dense_float64(seq_problem):
    m = seq_problem["model"]
    assert m.sequence and len(np.unique(m.gap_row_f)) > 10
    folded = seq_problem["folded"]
    pairs = [(0, 1), (3, 10), (5, 30), (20, 21)]
    for frm, to in ((0, m.S), (37, 211), (5, 6)):
        ob = np.stack([(folded[a] ^ folded[b])[frm:to] for a, b in pairs])
        hb = np.stack([(folded[a] & folded[b])[frm:to] for a, b in pairs])
        post, _ = O.decode_batch(m, ob, hb, frm, to)
        for v in range(len(pairs)):
            ref = dense_posterior_sequence(m, ob[v], hb[v], frm, to)
            got = post[frm:to, :, v].astype(np.float64)
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-5)
            assert np.max(np.abs(got - ref)) < 2e-5
            big = ref > 1e-3
            assert np.max(np.abs(got[big] / ref[big] - 1.0)) < 1e-3
