"""Models at the numeric edges of the decode: subnormal and exactly-zero posteriors, bitwise ties between states,
an IBD probability exactly equal to the scan's threshold, and pairs of identical or complementary haplotypes.

Each builder starts from a seeded synthetic problem (``synth`` + ``O.prepare_model``), edits the PreparedModel's
arrays (``Context.create_model`` takes any tables) and returns ``(pm, bits, folded, pairs)``.  Each one asserts on
the oracle's own output that its regime is reached, so that a later change to a generator cannot quietly turn an
edge test into a benign one; ``regime`` counts what the oracle produces.

Plain helper module imported by the tests (tests/test_gpu_numeric_edges.py, tests/test_oracle_dense_edges.py)."""
from __future__ import annotations

import numpy as np

from conftest import wave_group_member
from fastsmc_amd import synth
from oracle import oracle as O

N_PAIRS = 96
S_ARRAY = 400
S_SEQ = 300


def _haps(S, seq, seed, cm_per_mb=25.0):
    if seq:  # (conftest.seq_problem's generator: dense sites of varying spacing)
        return synth.make_haps(64, S, seed=seed, cm_per_mb=1.2, bp_per_site=2500, switch_per_cm=2.0)
    return synth.make_haps(64, S, seed=seed, cm_per_mb=cm_per_mb, switch_per_cm=0.6)


def _prepare(K, haps, seq, time=200):
    tables = synth.make_model_tables(K)
    bits, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, 64, time=time, decoding_sequence=seq)
    return pm, bits, folded


def benign(K, seq=False, S=None, seed=None, cm_per_mb=25.0):
    """The suite's ordinary generator: the reference point of the edge builders."""
    S = S or (S_SEQ if seq else S_ARRAY)
    pm, bits, folded = _prepare(K, _haps(S, seq, seed or (K + 7), cm_per_mb), seq)
    return pm, bits, folded, O.enumerate_all_pairs(32)[:N_PAIRS]


def oracle_posteriors(pm, folded, pairs, batch=64):
    """The oracle's posterior [S][K][B] of each batch of ``batch`` pairs (whole windows), with the batch's bits."""
    out = []
    for b0 in range(0, len(pairs), batch):
        sub = pairs[b0:b0 + batch]
        ob = np.stack([folded[a] ^ folded[b] for a, b in sub])
        hb = np.stack([folded[a] & folded[b] for a, b in sub])
        post, _ = O.decode_batch(pm, ob, hb, 0, pm.S)
        out.append((post, ob, hb))
    return out


def regime(pm, folded, pairs):
    """Counts over the oracle's posteriors of every pair: subnormal, exact zero, smallest positive, and sites at which
    two or more real states share the largest posterior bitwise (the per-pair MAP then has a tie to break)."""
    sub = zero = ties = 0
    smallest = np.inf
    for post, _, _ in oracle_posteriors(pm, folded, pairs):
        tiny = np.finfo(np.float32).tiny
        sub += int(np.count_nonzero((post > 0) & (post < tiny)))
        zero += int(np.count_nonzero(post == 0))
        pos = post[post > 0]
        if pos.size:
            smallest = min(smallest, float(pos.min()))
        top = post.max(axis=1, keepdims=True)
        ties += int(np.count_nonzero((post == top).sum(axis=1) > 1))
    return dict(subnormal=sub, zero=zero, smallest=smallest, tied_sites=ties)


def block_of(K):
    """States 0..7 (0..K/4-1 for fewer than 32 states) and eight states round a block boundary of the kernel that runs
    K: the wave boundary of a wave-group member (states kh-4 .. kh+3 for kh states a wave), a 16-state operand block /
    32-state boundary below 129 states (moved down so as to stay inside the model), state 64 for the any-K kernel."""
    if 128 < K <= 1024:
        c = wave_group_member(K)[1]
    elif K > 1024:
        c = 64
    else:
        c = min(32, K - 4)
    return np.unique(np.concatenate([np.arange(min(8, K // 4)), np.arange(c - 4, c + 4)]))


def subnormal(K, scale, seq=False):
    """Emissions of the states ``block_of(K)`` scaled by ``scale`` (1e-30: subnormal posteriors; 1e-38: subnormal table
    entries and exact-zero posteriors); in sequence mode the homozygous rows too.  The array-mode map is 10 cM/Mb,
    2 cM/Mb below 32 states: with the coarse states of a small model the suite's 25 cM/Mb mix too much to reach 1 000
    subnormals (794 at 33 states; 410 at 16 states and 10 cM/Mb)."""
    assert scale in (1e-30, 1e-38)
    pm, bits, folded, pairs = benign(K, seq, cm_per_mb=10.0 if K >= 32 else 2.0)
    blk = block_of(K)
    s = np.float32(scale)
    for name in ("e1", "e0m1", "e2m0") + (("hom",) if seq else ()):
        a = getattr(pm, name)
        a[:, blk] = a[:, blk] * s
    tiny = np.finfo(np.float32).tiny
    if scale == 1e-38:
        e = np.abs(pm.e1[:, blk])
        assert np.count_nonzero((e > 0) & (e < tiny)) > 100, "the table entries are subnormal"
    st = regime(pm, folded, pairs)
    assert st["subnormal"] > 1000, st
    if scale == 1e-38:
        assert st["zero"] > 1000, st
    return pm, bits, folded, pairs


def zero_states(K):
    """A few real states whose emission is exactly 0 at every site: the last two before the padding of a padded
    member, one low state and one in the middle.  Their posteriors are exactly +0, no other state's is."""
    pm, bits, folded, pairs = benign(K)
    dead = np.unique([1, K // 2, K - 2, K - 1])
    for name in ("e1", "e0m1", "e2m0"):
        getattr(pm, name)[:, dead] = 0.0
    live = np.setdiff1d(np.arange(K), dead)
    for post, _, _ in oracle_posteriors(pm, folded, pairs):
        d = post[:, dead]
        assert np.all(d == 0) and not np.any(np.signbit(d)), "dead states: exactly +0"
        assert np.all(post[:, live] > 0), "every other state has a positive posterior"
    return pm, bits, folded, pairs


def degenerate(K, seq=False):
    """Every posterior of a site bitwise equal: uniform prior, every state's emissions those of state 0, and every step
    on an appended identity row (D = 1, B = U = 0, RR = 1 below the last state: the key-0 row of synth's tables).
    ``prepare_model`` compacts the table to the rows the sites use, hence the explicit append."""
    pm, bits, folded, pairs = benign(K, seq)
    pm.pi = np.full(K, np.float32(1.0) / np.float32(K), np.float32)
    for name in ("e1", "e0m1", "e2m0") + (("hom",) if seq else ()):
        a = getattr(pm, name)
        a[:] = a[:, :1]
    rr = np.zeros(K, np.float32)
    rr[:K - 1] = 1.0
    for name, row in (("D", np.ones(K, np.float32)), ("B", np.zeros(K, np.float32)), ("U", np.zeros(K, np.float32)),
                      ("RR", rr)):
        setattr(pm, name, np.ascontiguousarray(np.vstack([getattr(pm, name), row[None, :]]), np.float32))
    ident = pm.D.shape[0] - 1
    pm.step_row = np.full(pm.S, ident, np.int32)
    if seq:
        for name in ("gap_row_f", "site_row_f", "gap_row_b", "site_row_b"):
            setattr(pm, name, np.full(pm.S, ident, np.int32))
    for post, _, _ in oracle_posteriors(pm, folded, pairs):
        assert np.all(post == post[:, :1]), "posteriors of a site equal across states"
        _, mp, _ = O.per_pair_output(pm, post, post.shape[2])
        assert np.all(mp == 0)
    recs = O.decode_pairs_ibd(pm, folded, pairs, batch_size=64)
    assert recs.size > 0 and np.all(recs["map"] == pm.exp_times[0])
    return pm, bits, folded, pairs


def ibd_probability(pm, post, v):
    """The scan's per-site IBD probability of lane v: the posteriors of the states below the state threshold, summed
    in ascending state order in fp32 (hmm_oracle.c, fo_ibd_scan_pair)."""
    acc = np.zeros(pm.S, np.float32)
    for k in range(pm.state_threshold):
        acc = (acc + post[:, k, v]).astype(np.float32)
    return acc


def threshold_equal(K):
    """The probability threshold set to the exact IBD probability of one site inside a segment (the segment's weakest
    interior site of the pair with the longest segment): the scan meets ``sum >= threshold`` with equality there.
    Asserted: the records differ from those of the next float above the threshold, at which that site falls out --
    a scan that took ``>`` for ``>=`` would produce those."""
    pm, bits, folded, pairs = benign(K)
    (post, _, _), = oracle_posteriors(pm, folded, pairs[:64])
    best = None
    for v in range(64):
        for r in O.ibd_scan_pair(pm, post, v, 0, pm.S, want_mean=False, want_map=False):
            if r["end"] - r["start"] >= 4 and (best is None or r["end"] - r["start"] > best[2] - best[1]):
                best = (v, int(r["start"]), int(r["end"]))
    assert best is not None, "a segment of at least five sites"
    v, s0, s1 = best
    prob = ibd_probability(pm, post, v)
    site = s0 + 1 + int(np.argmin(prob[s0 + 1:s1]))
    thr = np.float32(prob[site])
    assert thr > 0

    def records(t):
        pm.probability_threshold = np.float32(t)
        return O.decode_pairs_ibd(pm, folded, pairs, batch_size=64)

    above = records(np.nextafter(thr, np.float32(np.inf)))
    at = records(thr)  # (last: the model keeps this threshold)
    assert at.tobytes() != above.tobytes(), "the equality branch decides a record"
    return pm, bits, folded, pairs


def identical_and_complement_pairs(K):
    """Exact copies (one IBD segment over the whole window) and exact complements (no segment) among ordinary pairs of
    the same groups: haplotype 3 is a copy of 2, 9 of 4 and 40 of 11; 7 is the complement of 6 and 13 of 0."""
    haps = _haps(S_ARRAY, False, K + 7)
    copies = ((2, 3), (4, 9), (11, 40))
    compl = ((6, 7), (0, 13))
    for a, b in copies:
        haps.alleles[b] = haps.alleles[a]
    for a, b in compl:
        haps.alleles[b] = 1 - haps.alleles[a]
    pm, bits, folded = _prepare(K, haps, False)
    pairs = O.enumerate_all_pairs(32)[:N_PAIRS]
    # (2, 3), (4, 9), (6, 7) sit in the first group of 64 pairs, (0, 13) and (11, 40) in the second
    pairs[75] = (11, 40)
    recs = O.decode_pairs_ibd(pm, folded, pairs, batch_size=64)
    for a, b in copies:
        i = pairs.index((a, b))
        r = recs[recs["pair"] == i]
        assert r.size == 1 and r["start"][0] == 0 and r["end"][0] == pm.S - 1, (a, b, r)
    for a, b in compl:
        assert np.count_nonzero(recs["pair"] == pairs.index((a, b))) == 0, (a, b)
    assert np.count_nonzero(~np.isin(recs["pair"], [pairs.index(p) for p in copies + compl])) > 0
    return pm, bits, folded, pairs
