"""The numpy statement of fsmc_decode_pair_cdf (per pair and site: tail probabilities at state cuts and quantile states
of the posterior) for its tests.  Nothing here calls the code under test.

For pair i and site t, post[k] is the oracle's normalised fp32 posterior over the model's K states.  In fp32 and in
ascending k only:
  cdf[0] = float32(0) + post[0];  cdf[k] = cdf[k-1] + post[k]
  tail for a cut c, 1 <= c <= K:   cdf[c-1], float32
  quantile state for q, 0 < q <= 1: the smallest k with cdf[k] >= float32(q), int32; K-1 if no state reaches q.
`reduce` below is an explicit loop over k, vectorised over sites and pairs: numpy's float32 `+` on arrays is one IEEE
round-to-nearest add an element, so the order of the additions is the one written here (np.cumsum / np.sum are not used:
their order is numpy's business).

The pair list is PAIRS_192 of tests/pair_minima_lists.py on conftest's small problem (64 haplotypes x 640 sites, K = 69,
three full groups), decoded batch by batch of 64 as the work list's groups are.  The standard outputs are
CUTS = [1, state threshold, 25, 69] and QS = [0.025, 0.5, 0.975, 1.0].  tests/test_pair_cdf_lists.py proves on the CPU
what these reach on the oracle's posteriors."""
import numpy as np

from oracle import oracle as O
from pair_minima_lists import PAIRS_192, rows_192  # noqa: F401  (re-exported for the tests)

QS = [0.025, 0.5, 0.975, 1.0]


def cuts(pm):
    """The standard state cuts of a 69-state model: the first state alone, the IBD scan's threshold, 25, all states."""
    return [1, int(pm.state_threshold), 25, 69]


def oracle_posteriors(pm, folded, pairs):
    """[(post [S][K][64] float32, pairs of the batch)]: the oracle's posterior of `pairs`, batch by batch of 64."""
    out = []
    for b0 in range(0, len(pairs), 64):
        chunk = pairs[b0:b0 + 64]
        ob = np.stack([folded[a] ^ folded[b] for a, b in chunk])
        hb = np.stack([folded[a] & folded[b] for a, b in chunk])
        post, _ = O.decode_batch(pm, ob, hb, 0, pm.S)
        out.append((post, len(chunk)))
    return out


def reduce(post, n, cut_list, q_list):
    """(tail [len(cut_list)][n][S] float32, qstate [len(q_list)][n][S] int32) of the first n lanes of post [S][K][B]."""
    post = np.asarray(post)
    assert post.dtype == np.float32 and post.ndim == 3
    S, K, B = post.shape
    assert all(1 <= int(c) <= K for c in cut_list)
    qs = [np.float32(q) for q in q_list]
    tail = np.zeros((len(cut_list), S, B), np.float32)
    qstate = np.full((len(qs), S, B), K - 1, np.int32)  # (K-1 where no state reaches q)
    found = np.zeros((len(qs), S, B), bool)
    cdf = np.zeros((S, B), np.float32)
    for k in range(K):  # ascending k: one fp32 add a state
        cdf = cdf + post[:, k, :]
        assert cdf.dtype == np.float32
        for j, c in enumerate(cut_list):
            if int(c) - 1 == k:
                tail[j] = cdf
        for j, q in enumerate(qs):
            hit = (cdf >= q) & ~found[j]  # the first k only
            qstate[j][hit] = k
            found[j] |= hit
    return (np.ascontiguousarray(tail[:, :, :n].transpose(0, 2, 1)),
            np.ascontiguousarray(qstate[:, :, :n].transpose(0, 2, 1)))


def expected(pm, folded, pairs, cut_list, q_list):
    """reduce() over the oracle's posteriors of `pairs`: (tail [n_c][n][S], qstate [n_q][n][S])."""
    parts = [reduce(post, n, cut_list, q_list) for post, n in oracle_posteriors(pm, folded, pairs)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


_cache = {}


def posteriors_192(small_problem):
    """The oracle's posteriors of PAIRS_192, computed once a process and handed out read-only."""
    if "post" not in _cache:
        batches = oracle_posteriors(small_problem["model"], small_problem["folded"], PAIRS_192)
        for post, _ in batches:
            post.setflags(write=False)
        _cache["post"] = batches
    return _cache["post"]


def expected_192(small_problem, cut_list=None, q_list=None):
    """reduce() of posteriors_192 for the given cuts and quantiles (the standard sets by default), computed once a
    process for each set and handed out read-only."""
    pm = small_problem["model"]
    cut_list = cuts(pm) if cut_list is None else [int(c) for c in cut_list]
    q_list = QS if q_list is None else [float(np.float32(q)) for q in q_list]
    key = (tuple(cut_list), tuple(q_list))
    if key not in _cache:
        parts = [reduce(post, n, cut_list, q_list) for post, n in posteriors_192(small_problem)]
        tail = np.concatenate([p[0] for p in parts], axis=1)
        qstate = np.concatenate([p[1] for p in parts], axis=1)
        tail.setflags(write=False)
        qstate.setflags(write=False)
        _cache[key] = (tail, qstate)
    return _cache[key]
