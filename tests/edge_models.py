"""Models at the numeric edges of the decode: subnormal and exactly-zero posteriors, bitwise ties between states,
an IBD probability exactly equal to the scan's threshold, and pairs of identical or complementary haplotypes.

Each builder starts from a seeded synthetic problem (``synth`` + ``O.prepare_model``), edits the PreparedModel's
arrays (``Context.create_model`` takes any tables) and returns ``(pm, bits, folded, pairs)``.  Each one asserts on
the oracle's own output that its regime is reached, so that a later change to a generator cannot quietly turn an
edge test into a benign one; ``regime`` counts what the oracle produces.

``dyadic_ties`` is the model of the Viterbi tie rules: its regime is asserted on the numpy restatement of the
max-product sweep (tests/pair_viterbi_lists.py), since the oracle has no Viterbi.

``degenerate_with_dead_states`` is the model of the quantile states' plateau rule (fsmc_decode_pair_cdf: the smallest k
with cdf[k] >= q): equal posteriors put the running sum on the same value at thousands of cells, the exact zeros keep
it there for a state.  tests/pair_edge_lists.py puts it and the subnormal, zero-state and degenerate builders through
the five posterior-reducing decodePairs entry points.

Plain helper module imported by the tests (tests/test_gpu_numeric_edges.py, tests/test_oracle_dense_edges.py,
tests/pair_viterbi_lists.py, tests/pair_loglik_lists.py, tests/pair_edge_lists.py)."""
from __future__ import annotations

import functools

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


def degenerate_with_dead_states(K, seq=False):
    """``degenerate`` with the emissions of zero_states' states (1, K/2, K-2, K-1) exactly 0 at every site, in sequence
    mode the homozygous row too: the running sum of a site's posterior over the states stands still on each of them,
    at a value that thousands of cells share bitwise.  Dead states have posterior exactly +0, the live ones are bitwise
    equal at every site, and the per-pair MAP is state 0 everywhere."""
    pm, bits, folded, pairs = degenerate(K, seq)
    dead = np.unique([1, K // 2, K - 2, K - 1])
    for name in ("e1", "e0m1", "e2m0") + (("hom",) if seq else ()):
        getattr(pm, name)[:, dead] = 0.0
    live = np.setdiff1d(np.arange(K), dead)
    for post, _, _ in oracle_posteriors(pm, folded, pairs):
        d = post[:, dead]
        assert np.all(d == 0) and not np.any(np.signbit(d)), "dead states: exactly +0"
        assert np.all(post[:, live] > 0) and np.all(post[:, live] == post[:, :1]), "live states: equal and positive"
        _, mp, _ = O.per_pair_output(pm, post, post.shape[2])
        assert np.all(mp == 0)
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


def _blocks(rng, K, values, n_blocks):
    """[K] float32, constant over n_blocks runs of states (fewer where K is smaller) with random edges."""
    edges = np.sort(rng.choice(np.arange(1, K), min(n_blocks - 1, K - 1), replace=False))
    out = np.empty(K, np.float32)
    lo = 0
    for hi in list(edges) + [K]:
        out[lo:hi] = rng.choice(values)
        lo = hi
    return out


TIE_MINIMUM = 1000  # equal operands at each of the step's comparisons (dyadic_ties)


def dyadic_ties(K, S=129, seed=1, dead_top=False, regime=None):
    """Bitwise ties at every comparison of the max-product sweep (csrc/fsmc_pair_viterbi.h): every number of the model is
    a power of two (or 0) and constant over blocks of states -- pi = 2^-7; per site e1 in {1/4, 1/2, 1}, e0m1 in {0, 1/4,
    1/2}, e2m0 in {0, 1/4} over about five blocks whose edges are drawn afresh for every site (no multiple of 4 or 16 is
    preferred), where e0m1 and e2m0 keep a drawn value only where the class's emission (e1, e1 + e0m1, e1 + e0m1 + e2m0)
    stays a power of two and are 0 elsewhere; per table row D, B, U in {1/8, 1/4, 1/2} and the column ratios in {1/2, 1}
    over three blocks; RR[i] = U[i] cR[i+1] / U[i+1], exact for these values, so that the row-ratio form describes the
    same matrix (dense_reference.dense_T asserts it); the last column of B, U, RR and the column ratios stays 0 as in
    every model.  States of a block carry bitwise-equal values, products with powers of two are exact, and equal values
    through equal operations stay equal after the 1 / sum scaling: the ties survive every site.  And since the scaling
    factor is common to the states of a pair and commutes with a power of two, two states of a site either tie exactly or
    differ by a factor of two at least, in fp32 and in fp64 alike: the restatement's path is the dense fp64 Viterbi's for
    every pair.  (With emissions like 3/4 a product is rounded, two paths that take the same factors in another order
    differ in the last bit, differently in the two precisions, and a third of the sampled paths differed from the dense
    ones at equal probability.)  With ``dead_top`` the emissions of states K-2 and K-1 are exactly 0 at every site: their
    values are +0 like those of the ghost states a padded member has above them.

    70 pairs of 64 haplotypes.  Asserted on the restatement: at least TIE_MINIMUM bitwise-equal operands at each of the
    step's comparisons that pair_viterbi_lists.tie_rules(K) names; at the final argmax, which compares K - 1 times a pair
    and at one site only (TIE_MINIMUM is out of reach there: 140 comparisons in all at three states), at least one equal
    operand a pair on average; none at a comparison tie_rules(K) does not name.  How many ties a seed gives at the final
    argmax depends on the last site alone and varies widely, so a seed that misses fails here and not quietly in a
    test.  ``regime``: a dict that receives the restatement's output ("viterbi") and its counter ("counts")."""
    import pair_viterbi_lists as VL

    pm, bits, folded = _prepare(K, _haps(S, False, 100 + K + S), False)
    rng = np.random.default_rng(seed)
    pm.pi = np.full(K, np.float32(2.0 ** -7), np.float32)
    for pos in range(S):
        e1 = _blocks(rng, K, [0.25, 0.5, 1.0], 5)
        e0m1 = _blocks(rng, K, [0.0, 0.25, 0.5], 5)
        e2m0 = _blocks(rng, K, [0.0, 0.25], 5)
        # (each class's emission a power of two: e1, e1 + e0m1, e1 + e0m1 + e2m0)
        e0m1 = np.where(e0m1 == e1, e0m1, np.float32(0.0))
        e2m0 = np.where(e2m0 == e1 + e0m1, e2m0, np.float32(0.0))
        pm.e1[pos], pm.e0m1[pos], pm.e2m0[pos] = e1, e0m1, e2m0
    for r in range(pm.D.shape[0]):
        for tab in (pm.D, pm.B, pm.U):
            tab[r] = _blocks(rng, K, [0.125, 0.25, 0.5], 3)
    pm.col_ratios[:] = _blocks(rng, K, [0.5, 1.0], 3)
    pm.RR[:] = 0.0
    pm.RR[:, :K - 2] = pm.U[:, :K - 2] * pm.col_ratios[None, 1:K - 1] / pm.U[:, 1:K - 1]
    pm.B[:, K - 1] = pm.U[:, K - 1] = pm.col_ratios[K - 1] = 0.0
    if dead_top:
        for name in ("e1", "e0m1", "e2m0"):
            getattr(pm, name)[:, K - 2:] = 0.0
    pairs = O.enumerate_all_pairs(32)[37:37 + 70]
    counts = VL.new_counts()
    out = VL.viterbi(pm, folded, pairs, counts=counts)
    mant, _ = VL.expected(out[1], out[2])
    assert ((mant >= 0.5) & (mant < 1)).all(), "every pair has a finite, non-zero probability"
    for name in VL.CONTRACT:
        if name not in VL.tie_rules(K):
            assert counts[name] == 0, (K, S, seed, dead_top, name, counts)
        else:
            assert counts[name] >= (len(pairs) if name == "last" else TIE_MINIMUM), (K, S, seed, dead_top, name, counts)
    if regime is not None:
        regime.update(viterbi=out, counts=counts)
    return pm, bits, folded, pairs


# ---------------------------------------------------------------- the edge models of the two pair sweeps

# fsmc_decode_pair_loglik and fsmc_decode_pair_viterbi (forward_kernel, viterbi_kernel) at the edges above: every builder
# whose edge is in the model or the haplotypes (threshold_equal's is in the scan, which the sweeps do not run), at an exact
# member (69) and two padded ones (33 -> 48, 105 -> 112), 96 pairs = a full group and a half-full one; in sequence mode, which
# only the forward kernel has, the two builders that have it, at 69 states.
SWEEP_BUILDERS = {
    "subnormal-1e-30": lambda K, seq: subnormal(K, 1e-30, seq),
    "subnormal-1e-38": lambda K, seq: subnormal(K, 1e-38, seq),
    "zero-states": lambda K, seq: zero_states(K),
    "degenerate": lambda K, seq: degenerate(K, seq),
    "identical-complement": lambda K, seq: identical_and_complement_pairs(K),
}
SWEEP_CASES = [(name, K, False) for K in (69, 33, 105) for name in SWEEP_BUILDERS]
SWEEP_SEQ_CASES = [("subnormal-1e-30", 69, True), ("degenerate", 69, True)]


def sweep_id(case):
    return f"{case[0]}-K{case[1]}{'-seq' if case[2] else ''}"


@functools.lru_cache(maxsize=None)
def sweep_model(name, K, seq=False):
    """(pm, bits, folded, pairs) of a builder, built once a process and shared by the tests of both sweeps: read-only."""
    assert (name, K, seq) in SWEEP_CASES + SWEEP_SEQ_CASES
    return SWEEP_BUILDERS[name](K, seq)
