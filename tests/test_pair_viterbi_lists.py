"""What tests/pair_viterbi_lists.py claims, shown on the CPU: the paths of its float32 restatement of the contract are
those of a textbook fp64 Viterbi on the dense transition matrices (or as probable, to rounding), the reported
log-probabilities are the dense ones to fp32 rounding, and the inputs reach the regimes the GPU tests are there for:
among them the tie cases, on which each of the contract's five comparisons, flipped alone, changes a path, and the edge
models, on which every pair keeps a finite, non-zero probability."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
import pair_viterbi_lists as VL
from conftest import expected_member

# Over the sampled pairs of every case, measured on the CPU (both relative to the dense optimum's log-probability):
#   the fp64 joint log-probability of the restatement's path against the dense Viterbi optimum: at most 1.97e-15 (the
#     rich case; every one of the 242 sampled paths is the dense one, what is left is the order of the fp64 additions)
#   the reported log-probability, log(mant) + expo ln 2, against the dense optimum: at most 4.19e-8 (the 20-state case;
#     1.1e-8 on S200, 4.4e-9 on the rich case): fp32 rounding of the sums, relative to log-probabilities of -0.7 ... -330
#   the tie cases (edge_models.dyadic_ties), measured the same way: every one of their 101 sampled paths is the dense one
#     (every number of the model is a power of two, so two states either tie exactly or differ by a factor of two, in
#     fp32 and in fp64 alike), the path's log-probability to 2.26e-15 (the 300-site case), the reported one to 8.3e-9:
#     both inside the bounds below, which stay as they were
# Nothing derives a tighter bound, so four times the measured values are allowed.
MEASURED_PATH_DIFFERENCE = 1.97e-15
MEASURED_REPORTED_DIFFERENCE = 4.19e-8
PATH_BOUND = 4 * MEASURED_PATH_DIFFERENCE
REPORTED_BOUND = 4 * MEASURED_REPORTED_DIFFERENCE


def _sample(name):
    """The pairs of a case that are compared with the dense Viterbi (a dense run costs K^2 a site)."""
    K, S, n = (VL.TIE_CASES[name][:2] + (VL.TIE_PAIRS,)) if name in VL.TIE_CASES else VL.CASES[name]
    return range(0, n, 7 if S >= 300 else 5 if K < 100 else 10)


_compared = {}


def _compare(name):
    """(sampled, paths that differ, worst relative difference of the path's log-probability, of the reported one), once."""
    if name not in _compared:
        pm, _, folded, pairs, states, sums, last = VL.case(name)
        lp = VL.log_probability(*VL.expected(sums, last))
        worst_path = worst_reported = 0.0
        differ = 0
        for i in _sample(name):
            path, dense_lp = VL.dense_viterbi(pm, folded, pairs[i])
            own = VL.dense_path_log_probability(pm, folded, pairs[i], states[i].astype(np.int64))
            differ += not np.array_equal(path, states[i])
            worst_path = max(worst_path, abs(own - dense_lp) / abs(dense_lp))
            worst_reported = max(worst_reported, abs(lp[i] - dense_lp) / abs(dense_lp))
        _compared[name] = (len(_sample(name)), differ, worst_path, worst_reported)
    return _compared[name]


@pytest.mark.parametrize("name", list(VL.CASES) + list(VL.TIE_CASES))
def test_paths_and_probabilities_against_the_dense_viterbi(name):
    pm, _, _, pairs, states, sums, last = VL.case(name)
    assert states.dtype == np.uint8 and states.shape == (len(pairs), pm.S) and (states < pm.K).all()
    mant, _ = VL.expected(sums, last)
    assert ((mant >= 0.5) & (mant < 1)).all()
    n, differ, worst_path, worst_reported = _compare(name)
    print(f"{name}: {n} sampled, {differ} paths differ from the dense one; relative difference of the path's "
          f"log-probability {worst_path:.3e}, of the reported one {worst_reported:.3e}")
    assert worst_path <= PATH_BOUND, (name, worst_path)
    assert worst_reported <= REPORTED_BOUND, (name, worst_reported)


def test_at_most_five_per_cent_of_sampled_paths_differ():
    """Near-ties may resolve differently in fp32 and fp64; over all cases together."""
    done = [_compare(name) for name in list(VL.CASES) + list(VL.TIE_CASES)]
    sampled, differ = sum(d[0] for d in done), sum(d[1] for d in done)
    print(f"{differ} of {sampled} sampled paths differ from the dense Viterbi's")
    assert differ <= 0.05 * sampled, (differ, sampled)


def test_at_most_five_per_cent_of_sampled_tie_paths_differ():
    """The same cap on the tie cases alone: np.argmax takes the first maximum, which is the contract's rule, so a tie is
    no reason for the dense path to differ."""
    done = [_compare(name) for name in VL.TIE_CASES]
    sampled, differ = sum(d[0] for d in done), sum(d[1] for d in done)
    print(f"{differ} of {sampled} sampled paths of the tie cases differ from the dense Viterbi's")
    assert differ <= 0.05 * sampled, (differ, sampled)


def test_on_the_cohort():
    pm, _, folded, _ = VL.cohort_problem()
    pairs = VL.cohort_pairs()[0]
    states, sums, last = VL.cohort_viterbi()
    assert states.shape == (200, 700)
    assert np.array_equal(sums > 0, np.ones_like(sums, bool))
    lp = VL.log_probability(*VL.expected(sums, last))
    for i in range(0, 200, 40):
        path, dense_lp = VL.dense_viterbi(pm, folded, pairs[i])
        own = VL.dense_path_log_probability(pm, folded, pairs[i], states[i].astype(np.int64))
        assert abs(own - dense_lp) <= PATH_BOUND * abs(dense_lp) and abs(lp[i] - dense_lp) <= REPORTED_BOUND * abs(dense_lp)
    # below the data likelihood: one path against the sum over all of them
    ll = LL.log_likelihood(*LL.expected(LL.cohort_sums())[:2])
    assert (lp <= ll).all()


def _predecessor_kinds(states):
    """On final paths, at states k >= 1: came from below (i < k), stayed (i = k), came from above (i > k)."""
    prev, cur = states[:, :-1].astype(int), states[:, 1:].astype(int)
    at = cur >= 1
    return int(((prev < cur) & at).sum()), int(((prev == cur) & at).sum()), int(((prev > cur) & at).sum())


@pytest.mark.parametrize("name", VL.RICH)
def test_rich_cases_move(name):
    """A kernel whose back-pointer was always `stay` passes where paths never move: here they do."""
    _, _, _, pairs, states, _, _ = VL.case(name)
    runs = np.array([len(VL.state_runs(r)[0]) for r in states])
    move = np.diff(states.astype(int), axis=1)
    up, down = int((move > 0).sum()), int((move < 0).sum())
    below, stay, above = _predecessor_kinds(states)
    print(f"{name}: runs a pair min {runs.min()} median {np.median(runs)} max {runs.max()}, {int((runs >= 4).sum())} of "
          f"{len(pairs)} pairs with >= 4 runs, {up} upward and {down} downward moves; predecessors at k >= 1: {below} "
          f"below, {stay} equal, {above} above")
    assert (runs >= 4).sum() * 2 >= len(pairs)
    assert up > 0 and down > 0
    assert below > 0 and stay > 0 and above > 0


def test_rich_case_moves_across_chunk_boundaries():
    """For every chunk length the GPU test runs the rich case with -- the ones it sets and the ones the planner picks
    under its workspace limits -- some pair changes state from the last site of a chunk to the first of the next (the
    traceback's hand-over between chunks), and some pair across a multiple of 64 (a new word of haplotype bits, a new
    register of table rows)."""
    _, _, _, _, states, _, _ = VL.case("rich")
    S = states.shape[1]
    changes = states[:, 1:] != states[:, :-1]  # [pair][t - 1]: between site t - 1 and t
    planned = [VL.planned(S, 69, 2, limit) for limit in VL.LIMITS_RICH]
    assert planned == [(53, 14, 2), (88, 8, 1)], planned  # (what the GPU test asserts of fsmc_ctx_last_plan)
    for C in VL.CHUNKS_RICH + tuple(c for c, _, _ in planned):
        if C in (0, S):
            continue
        at = np.arange(C, S, C)
        assert changes[:, at - 1].any(), C
    assert changes[:, np.arange(64, S, 64) - 1].any()
    assert any(C and S % C for C in VL.CHUNKS_RICH) and S in VL.CHUNKS_RICH and 0 in VL.CHUNKS_RICH


def test_s65_case_in_chunks():
    """The 65-site case in the chunks of the GPU test.  Its most probable paths move between five pairs of sites only
    (into t = 4, 51, 52, 56 and 62), so no chunk length puts a move on EVERY boundary -- none of 2, 3, 4, 5, 7 and 64 does;
    what holds, and is asserted: the chunks of 2, 3, 4 and 7 sites each have a boundary that some path moves across (the
    traceback's hand-over with a change of state), one of the lengths is no multiple of four, and the last chunk is ragged
    in every one.  What this case adds on the GPU is the rows' phases (65 bytes a row), not moving paths; those are the
    rich case's above."""
    _, _, _, _, states, _, _ = VL.case("S65")
    S = states.shape[1]
    moved = np.flatnonzero((states[:, 1:] != states[:, :-1]).any(axis=0)) + 1
    assert moved.tolist() == [4, 51, 52, 56, 62], moved
    for C in VL.CHUNKS_S65:
        if C != 64:
            assert set(range(C, S, C)) & set(moved.tolist()), C
    assert any(C % 4 for C in VL.CHUNKS_S65) and all(S % C for C in VL.CHUNKS_S65)


def test_small_models_move_too():
    for name, lo in (("K2", 1), ("K3", 2)):
        _, _, _, _, states, _, _ = VL.case(name)
        runs = np.array([len(VL.state_runs(r)[0]) for r in states])
        print(f"{name}: {runs.min()} - {runs.max()} runs a pair")
        assert runs.max() >= 4 and runs.min() >= lo


def test_zero_sum_problem():
    """The affected pairs have mantissa 0 / NaN, the others are finite, and every state lies in [0, K)."""
    pm, _, _, pairs, states, sums, last = VL.zero_sum_viterbi()
    mant, expo = VL.expected(sums, last)
    bad = (mant == 0) | ~np.isfinite(mant)
    hit = (sums == 0).any(axis=1)
    assert np.array_equal(bad, hit) and 2 <= bad.sum() <= len(pairs) - 2
    assert ((mant[~bad] >= 0.5) & (mant[~bad] < 1)).all()
    assert (states < pm.K).all()
    # lanes are independent: the pairs that are not hit, decoded without the others, give the same rows
    again = VL.viterbi(pm, VL.zero_sum_viterbi()[2], [pairs[i] for i in np.flatnonzero(~bad)])
    assert np.array_equal(again[0], states[~bad]) and np.array_equal(again[1], sums[~bad])


@pytest.mark.parametrize("name", list(VL.CASES) + list(VL.TIE_CASES))
def test_viterbi_probability_is_at_most_the_likelihood(name):
    pm, _, folded, pairs, _, sums, last = VL.case(name)
    lp = VL.log_probability(*VL.expected(sums, last))
    if name in VL.RICH or name in VL.TIE_CASES:
        fsums, _ = LL.forward(pm, folded, pairs)
    else:
        fsums = LL.case(name)[4]
    ll = LL.log_likelihood(*LL.expected(fsums)[:2])
    assert (lp <= ll).all() and (lp < ll).any()


# ---------------------------------------------------------------- the tie rules

def _one_rule_flipped(flipped, lanes):
    """The contract's rules, with the comparison `flipped[j]` (`>=` for `>` or the reverse) in lanes [j * lanes, (j + 1)
    * lanes) only: every mutant of a case in one run of the restatement, lanes being independent."""
    rules = {}
    for name, cmp in VL.CONTRACT.items():
        mask = np.repeat([f == name for f in flipped], lanes)

        def rule(a, b, cmp=cmp, mask=mask):
            return np.where(mask, VL.FLIPPED[cmp](a, b), cmp(a, b))

        rules[name] = rule
    return rules


@pytest.mark.parametrize("name", list(VL.TIE_CASES))
def test_every_tie_rule_decides_a_path(name):
    """The mutants: the restatement with one comparison flipped gives other states for at least one pair, for every
    comparison that can tie at this K -- so a kernel that broke that tie the other way would not pass on this input.  The
    comparisons that cannot tie (tie_rules: K = 2 has no suffix, carry or last tie, K = 3 no last tie) met no equal operands,
    and flipping them changes nothing: stated, not skipped."""
    pm, _, folded, pairs, states, sums, last = VL.case(name)
    counts = VL.tie_counts(name)
    can_tie = VL.tie_rules(pm.K)
    n = len(pairs)
    flipped = list(VL.CONTRACT)
    out = VL.viterbi(pm, folded, list(pairs) * len(flipped), _one_rule_flipped(flipped, n))
    changed = {f: int((out[0][j * n:(j + 1) * n] != states).any(axis=1).sum()) for j, f in enumerate(flipped)}
    print(f"{name}: equal operands {({f: counts[f] for f in flipped})}; pairs whose path changes under a single flip "
          f"{changed}; {len({r.tobytes() for r in states})} distinct paths")
    for f in flipped:
        if f in can_tie:
            assert counts[f] > 0 and changed[f] >= 1, (name, f, counts, changed)
        else:
            assert counts[f] == 0 and changed[f] == 0, (name, f, counts, changed)
    # (the unflipped lanes of such a run are the restatement's own: the lane trick changes nothing)
    again = VL.viterbi(pm, folded, list(pairs) * 2, _one_rule_flipped(["suffix", None], n))
    assert all(np.array_equal(a[n:], b) for a, b in zip(again, (states, sums, last)))


def test_flipped_rules_are_the_other_comparison():
    a, b = np.array([1, 2, 2], np.float32), np.array([2, 2, 1], np.float32)
    for cmp, other in VL.FLIPPED.items():
        assert (cmp(a, b) != other(a, b)).tolist() == [False, True, False]
    assert [VL.CONTRACT[f](b, b).all() for f in ("suffix", "carry", "diag", "lower", "last")] == [True, True, False, False, False]


@pytest.mark.parametrize("name", [n for n, c in VL.TIE_CASES.items() if c[3]])
def test_dead_top_walks_beside_the_ghosts(name):
    """The padded members whose two top states are at +0 like the ghosts above them: no path leaves the model, and some
    path visits the live states just below (>= K - 4), so the top of the model is walked next to the ties with the ghosts."""
    pm, _, _, _, states, _, _ = VL.case(name)
    K = pm.K
    assert K < expected_member(K)  # (a padded member)
    assert (states < K).all()
    top = int(states.max())
    print(f"{name}: highest state visited {top} of {K}; {int((states >= K - 4).any(axis=1).sum())} pairs visit a state >= K - 4")
    assert top >= K - 4


def test_tie_case_moves_across_chunk_boundaries():
    """For every chunk length the GPU test gives the 300-site tie case (16 and 150 sites, and the planner's under the
    workspace limit) some pair changes state from the last site of a chunk to the first of the next, as the rich case
    does: the traceback hands over between chunks while paths move through ties."""
    _, _, _, _, states, _, _ = VL.case(VL.TIE_CHUNKED)
    S = states.shape[1]
    changes = states[:, 1:] != states[:, :-1]
    planned = VL.planned(S, 69, 2, VL.LIMIT_TIES)
    assert planned == (75, 4, 2), planned  # (what the GPU test asserts of fsmc_ctx_last_plan)
    for C in (16, 150, planned[0]):
        assert changes[:, np.arange(C, S, C) - 1].any(), C
    assert any(C and S % C for C in VL.CHUNKS_TIES) and 0 in VL.CHUNKS_TIES


# ---------------------------------------------------------------- the numeric edges (tests/edge_models.py)

@pytest.mark.parametrize("case", E.SWEEP_CASES + E.SWEEP_SEQ_CASES, ids=E.sweep_id)
def test_edge_models_leave_every_pair_a_probability(case):
    """On every edge model the GPU tests of the two sweeps run, both restatements give every one of the 96 pairs a finite,
    non-zero mantissa (no zero scaling sum anywhere): the GPU tests compare every pair bit for bit and exempt none.  The
    Viterbi restatement has no sequence mode (the kernel refuses it)."""
    name, K, seq = case
    pm, _, _, pairs, fsums = LL.edge_case(name, K, seq)
    assert len(pairs) == 96 and pm.K == K and bool(pm.sequence) == seq
    fm, _, _, _ = LL.expected(fsums)
    assert np.isfinite(fsums).all() and (fsums > 0).all() and ((fm >= 0.5) & (fm < 1)).all()
    if seq:
        print(f"{E.sweep_id(case)}: smallest forward sum {fsums.min():.3e}")
        return
    _, _, _, _, states, sums, last, counts = VL.edge_case(name, K)
    mant, _ = VL.expected(sums, last)
    print(f"{E.sweep_id(case)}: smallest forward sum {fsums.min():.3e}, smallest Viterbi sum {sums.min():.3e}, smallest "
          f"last delta {last.min():.3e}; counter {counts}; {len({r.tobytes() for r in states})} distinct paths")
    assert np.isfinite(sums).all() and (sums > 0).all() and np.isfinite(last).all() and (last > 0).all()
    assert ((mant >= 0.5) & (mant < 1)).all()
    assert (states < K).all()
    if name == "subnormal-1e-38":  # the max-product vectors themselves carry subnormals, not only the tables
        assert counts["subnormal"] > 100, counts


def test_state_runs():
    starts, ends, states = VL.state_runs(np.array([3, 3, 5, 5, 5, 2], np.uint8))
    assert starts.tolist() == [0, 2, 5] and ends.tolist() == [2, 5, 6] and states.tolist() == [3, 5, 2]
