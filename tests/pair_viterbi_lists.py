"""Inputs and the numpy statement of fsmc_decode_pair_viterbi (per pair: the most probable joint state sequence under the
model and its probability as mantissa and exponent) for its tests.  Nothing here calls the code under test.

The statement is the contract of include/fastsmc_hip.h in float32, one numpy operation per IEEE operation and one numpy
comparison per comparison, vectorised over the pairs (lanes are independent):
  viterbi(pm, folded, pairs) -> (states [n][S] uint8, sums [n][S] float32, last [n] float32)
    site 0: v = pi * em0.  Site t >= 1, from the scaled vector p of site t-1: the suffix maximum from the top with `>=`
    (the smaller index wins a tie), MU / uI = the running maximum of U[k-1] * p[k-1] and cR[k-1] * MU with `>=` for the
    carried value, best = MU, then d = D[k] * p[k] with `>`, then l = B[k] * mC[k+1] with `>`; v[k] = em[k] * best,
    psi[t][k] = the index best came from.  Every site: the sum over k ascending from 0.f, delta = v * (1.0f / sum)
    (pair_loglik_lists._sum_and_scale).  x[S-1] = the first maximum of the last delta, x[t-1] = psi[t][x[t]];
    `last` = delta[S-1][x[S-1]].
  expected(sums, last) -> (mant [n] float64, expo [n] int32): pair_loglik_lists.chain over the sums, then once more with
    `last`.
The emission rows are pair_loglik_lists.forward's: (e1 + e0m1 * z) + e2m0 * t.
_next_delta and viterbi take the five comparisons as `rules` (CONTRACT by default) and an optional counter of bitwise-equal
operands, so that a test can show on the CPU which ties an input contains and that each one decides a path.

The yardstick is a textbook Viterbi in float64 on the dense transition matrices of tests/dense_reference.py
(dense_viterbi), and the joint log-probability of any path on the same matrices (dense_path_log_probability)."""
import operator

import numpy as np

from fastsmc_amd import synth
from oracle import oracle as O
from pair_loglik_lists import (ALL_PAIRS, CASES as LL_CASES, PAIR_COUNTS, _pair_bits, _problem, _sum_and_scale,  # noqa: F401
                               case as ll_case, chain, cohort_problem, zero_sum_problem)
from pair_common import cohort_pairs

F32 = np.float32


# The five comparisons of the contract (the header of csrc/fsmc_pair_viterbi.h): with these, the smaller predecessor index
# wins every tie.  `rules` below maps each name to the comparison that takes its place (a function of two float32
# arrays, first operand as the contract writes it); tests/test_pair_viterbi_lists.py flips one at a time to show that an
# input tells the two apart.
CONTRACT = {"suffix": operator.ge, "carry": operator.ge, "diag": operator.gt, "lower": operator.gt, "last": operator.gt}
FLIPPED = {operator.ge: operator.gt, operator.gt: operator.ge}
TINY = np.finfo(F32).tiny


def new_counts():
    """A counter for _next_delta / viterbi: per comparison, how often its two operands were bitwise equal (the suffix
    comparison at k = 0 decides nothing that is read and is not counted), and under "subnormal" how many values of the
    vectors v and delta were subnormal."""
    return dict.fromkeys(tuple(CONTRACT) + ("subnormal",), 0)


def _equal(counts, name, a, b):
    if counts is not None:
        counts[name] += int(np.count_nonzero(a == b))


def _next_delta(pm, row, prev, em, rules=CONTRACT, counts=None):
    """One max-product step: prev, em [n][K] float32 -> (v [n][K] float32, psi [n][K] uint8)."""
    K = pm.K
    D, B, U, cR = pm.D[row], pm.B[row], pm.U[row], pm.col_ratios
    n = prev.shape[0]
    mC = np.empty_like(prev)
    cI = np.empty((n, K), np.int32)
    mC[:, K - 1] = prev[:, K - 1]
    cI[:, K - 1] = K - 1
    for k in range(K - 2, -1, -1):
        if k >= 1:
            _equal(counts, "suffix", prev[:, k], mC[:, k + 1])
        ge = rules["suffix"](prev[:, k], mC[:, k + 1])
        mC[:, k] = np.where(ge, prev[:, k], mC[:, k + 1])
        cI[:, k] = np.where(ge, k, cI[:, k + 1])
    v = np.empty_like(prev)
    psi = np.empty((n, K), np.uint8)
    MU = np.zeros(n, F32)
    uI = np.zeros(n, np.int32)
    for k in range(K):
        d = D[k] * prev[:, k]
        if k >= 1:
            cand = U[k - 1] * prev[:, k - 1]
            car = cR[k - 1] * MU
            _equal(counts, "carry", car, cand)
            ge = rules["carry"](car, cand)
            MU = np.where(ge, car, cand)
            uI = np.where(ge, uI, k - 1)
            _equal(counts, "diag", d, MU)
            gd = rules["diag"](d, MU)
            best = np.where(gd, d, MU)
            arg = np.where(gd, k, uI)
        else:
            best = d
            arg = np.zeros(n, np.int32)
        if k < K - 1:
            l = B[k] * mC[:, k + 1]
            _equal(counts, "lower", l, best)
            gl = rules["lower"](l, best)
            best = np.where(gl, l, best)
            arg = np.where(gl, cI[:, k + 1], arg)
        assert best.dtype == F32 and MU.dtype == F32
        v[:, k] = em[:, k] * best
        psi[:, k] = arg
    return v, psi


def viterbi(pm, folded, pairs, rules=CONTRACT, counts=None):
    """(states [n][S] uint8, sums [n][S] float32, last [n] float32) of `pairs` over the whole sequence, array mode.
    `rules`: the comparisons, the contract's by default; `counts`: a new_counts() to fill, or None."""
    assert not pm.sequence and pm.K <= 128
    ob, hb = _pair_bits(folded, pairs)
    n, S, K = len(pairs), pm.S, pm.K
    z = np.where(ob != 0, F32(0.0), F32(1.0)).astype(F32)  # isZero
    t = np.where(hb != 0, F32(1.0), F32(0.0)).astype(F32)  # isTwo

    def emission(pos):
        return (pm.e1[pos][None, :] + pm.e0m1[pos][None, :] * z[:, pos, None]) + pm.e2m0[pos][None, :] * t[:, pos, None]

    def subnormal(*vectors):
        if counts is not None:
            counts["subnormal"] += sum(int(np.count_nonzero((a > 0) & (a < TINY))) for a in vectors)

    sums = np.empty((n, S), F32)
    psi = np.zeros((S, n, K), np.uint8)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = pm.pi[None, :] * emission(0)
        sums[:, 0], delta = _sum_and_scale(v)
        subnormal(v, delta)
        for pos in range(1, S):
            v, psi[pos] = _next_delta(pm, int(pm.step_row[pos]), delta, emission(pos), rules, counts)
            sums[:, pos], delta = _sum_and_scale(v)
            subnormal(v, delta)
        best = delta[:, 0].copy()
        x = np.zeros(n, np.int64)
        for k in range(1, K):
            _equal(counts, "last", delta[:, k], best)
            gt = rules["last"](delta[:, k], best)
            best = np.where(gt, delta[:, k], best)
            x = np.where(gt, k, x)
    assert best.dtype == F32
    states = np.empty((n, S), np.uint8)
    rows = np.arange(n)
    for pos in range(S - 1, -1, -1):
        states[:, pos] = x
        if pos:
            x = psi[pos][rows, x].astype(np.int64)
    return states, sums, best


def expected(sums, last):
    """(mant float64 [n], expo int32 [n]): the chain over the sums and then `last`."""
    return chain(np.concatenate([sums, last[:, None]], axis=1).astype(F32), 0, sums.shape[1] + 1)


def log_probability(mant, expo):
    with np.errstate(divide="ignore"):
        return np.log(mant) + expo.astype(np.float64) * np.log(2.0)


def state_runs(row):
    """(starts, ends, states) of the runs of one row: the statement of fastsmc_amd.api.state_runs."""
    row = np.asarray(row)
    cut = np.flatnonzero(row[1:] != row[:-1]) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [row.size]])
    return starts, ends, row[starts]


# ---------------------------------------------------------------- the fp64 yardstick

def _dense(pm, folded, pair):
    import dense_reference as DR

    x = folded[pair[0]] ^ folded[pair[1]]
    t = folded[pair[0]] & folded[pair[1]]
    Ts = {}

    def T(pos):
        row = int(pm.step_row[pos])
        return Ts.setdefault(row, DR.dense_T(pm, row))

    def em(pos):
        return DR.emission(pm, pos, x[pos], t[pos])

    return T, em


def dense_viterbi(pm, folded, pair):
    """(path [S], log P(path, observations)) by a textbook Viterbi in float64 on the dense matrices: delta'[k] = em[k] *
    max_i delta[i] * T[i][k] (the first maximum), renormalised at every site."""
    T, em = _dense(pm, folded, pair)
    S, K = pm.S, pm.K
    d = pm.pi.astype(np.float64) * em(0)
    lp = np.log(d.sum())
    d = d / d.sum()
    psi = np.zeros((S, K), np.int64)
    for pos in range(1, S):
        cand = d[:, None] * T(pos)  # [from][to]
        psi[pos] = np.argmax(cand, axis=0)
        d = em(pos) * cand.max(axis=0)
        lp += np.log(d.sum())
        d = d / d.sum()
    x = int(np.argmax(d))
    lp += np.log(d[x])
    path = np.empty(S, np.int64)
    for pos in range(S - 1, -1, -1):
        path[pos] = x
        if pos:
            x = int(psi[pos][x])
    return path, lp


def dense_path_log_probability(pm, folded, pair, path):
    """log P(path, observations of the pair) in float64 on the dense matrices."""
    T, em = _dense(pm, folded, pair)
    with np.errstate(divide="ignore"):
        lp = np.log(pm.pi.astype(np.float64)[path[0]]) + np.log(em(0)[path[0]])
        for pos in range(1, pm.S):
            lp += np.log(T(pos)[path[pos - 1], path[pos]]) + np.log(em(pos)[path[pos]])
    return lp


# ---------------------------------------------------------------- the inputs

def _rich_problem(K, S):
    """A map dense in recombination (1000 cM / Mb): paths that move, up and down, every few dozen sites."""
    n_hap = 64
    tables = synth.make_model_tables(K)
    haps = synth.make_haps(n_hap, S, seed=23, cm_per_mb=1000.0, switch_per_cm=0.6)
    bits, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, n_hap, time=200)
    return pm, bits, folded


# the array-mode cases of pair_loglik_lists (models K = 2 ... 128 at 129 sites; 1 ... 200 sites at K = 69; 200 pairs at
# 65 sites) and the two rich ones: name -> (K, S, pairs)
CASES = {name: (K, S, n) for name, (K, S, n, seq, _) in LL_CASES.items() if not seq}
CASES["rich"] = (69, 700, 70)
CASES["dense40"] = (40, 300, 70)
RICH = ("rich", "dense40")
CHUNKS_RICH = (16, 64, 150, 700, 0)  # chunk lengths of the GPU test on the rich case: 150 does not divide 700, 0 = automatic
# ... and on the 65-site case, whose 200 rows each start at another phase of the output's groups of four sites and share
# groups with their neighbours: a chunk that ends at t = 1 (2), edges inside a group (2, 3, 7) and on group boundaries of
# the aligned rows (4, 64), a last chunk shorter than the others in every one
CHUNKS_S65 = (2, 3, 4, 7, 64)

LIMITS_RICH = (1 << 20, 600 << 10)  # workspace limits of the GPU test on the rich case (two groups: two waves wanted)


def planned(S, member, waves_wanted, limit):
    """(chunk sites, chunks, waves) of fsmc_decode_pair_viterbi under a workspace limit, as its planner states them: a
    wave's slot is chunk rows of back-pointers (ceil(member / 4) x 256 bytes a site) and a checkpoint (x 1024 bytes) a
    chunk; the waves are what the limit holds of the smallest slot (about 2 sqrt(S) sites a chunk); the chunk is the whole
    sequence halved (rounding up, never below that smallest chunk) until the waves' slots fit the limit."""
    k4 = (member + 3) // 4

    def slot(c):
        return c * k4 * 256 + -(-S // c) * k4 * 1024

    c_min = min(S, max(1, int(np.ceil(2.0 * np.sqrt(S)))))
    waves = min(waves_wanted, limit // slot(c_min))
    assert waves >= 1
    c = S
    while c > c_min and waves * slot(c) > limit:
        c = max(c_min, (c + 1) // 2)
    return c, -(-S // c), waves


# the tie cases (edge_models.dyadic_ties: states in blocks of bitwise-equal values, so that every comparison of the
# contract meets equal operands): name -> (K, S, seed, dead_top); 70 pairs each.  69 is an exact member, 33 and 105 are
# padded (to 48 and 112: ghost states at +0 above the model, which `dead` real states tie with), 128 the top of the family,
# 3 and 2 the smallest; 300 sites for the chunked runs.  The seeds are ones at which the builder's own assertion holds and
# every comparison decides a path (tests/test_pair_viterbi_lists.py): with every seed tried the step's four do at 33 states
# and more; the final argmax's ties depend on the last site alone, and at two and three states about half the seeds have
# none.
TIE_CASES = {
    "ties-K69": (69, 129, 2, False),
    "ties-K33": (33, 129, 4, False),
    "ties-K105": (105, 129, 3, False),
    "ties-K128": (128, 129, 2, False),
    "ties-K3": (3, 129, 8, False),
    "ties-K2": (2, 129, 7, False),
    "ties-K33-dead": (33, 129, 4, True),
    "ties-K105-dead": (105, 129, 3, True),
    "ties-K69-S300": (69, 300, 3, False),
}
TIE_PAIRS = 70
TIE_CHUNKED = "ties-K69-S300"
CHUNKS_TIES = (16, 150, 0)  # chunk lengths of the GPU test on the 300-site tie case: 16 does not divide 300, 0 = automatic
LIMIT_TIES = 1 << 20  # its workspace limit (two groups: two waves wanted)


def tie_rules(K):
    """The comparisons that can meet equal operands in a model of K states: all five, but for two states.  There no
    suffix comparison is read (they are at k >= 1 and below K - 1), and the one carried MU is cR[0] * 0.f = +0 against
    U[0] * p[0] > 0."""
    return ("diag", "lower", "last") if K == 2 else tuple(CONTRACT)


_cache = {}
_counts = {}


def tie_counts(name):
    """The counter of the restatement's run on a tie case (new_counts())."""
    case(name)
    return _counts[name]


def case(name):
    """(pm, bits, folded, pairs, states, sums, last) of a case; the restatement runs once a process and is read-only."""
    if name not in _cache and name in TIE_CASES:
        import edge_models as E

        K, S, seed, dead_top = TIE_CASES[name]
        regime = {}
        pm, bits, folded, pairs = E.dyadic_ties(K, S, seed, dead_top, regime)
        assert len(pairs) == TIE_PAIRS
        out, _counts[name] = regime["viterbi"], regime["counts"]
        for a in out:
            a.setflags(write=False)
        _cache[name] = (pm, bits, folded, pairs) + out
    if name not in _cache:
        K, S, n = CASES[name]
        if name in RICH:
            pm, bits, folded = _rich_problem(K, S)
            pairs = ALL_PAIRS[37:37 + n]
        else:
            pm, bits, folded, pairs, _, _ = ll_case(name)
        out = viterbi(pm, folded, pairs)
        for a in out:
            a.setflags(write=False)
        _cache[name] = (pm, bits, folded, pairs) + out
    return _cache[name]


def cohort_viterbi():
    """viterbi() of pair_common.cohort_pairs() on the 700-site cohort, once a process."""
    if "cohort" not in _cache:
        pm, _, folded, _ = cohort_problem()
        out = viterbi(pm, folded, cohort_pairs()[0])
        for a in out:
            a.setflags(write=False)
        _cache["cohort"] = out
    return _cache["cohort"]


def zero_sum_viterbi():
    """(pm, bits, folded, pairs, states, sums, last) of pair_loglik_lists.zero_sum_problem()."""
    if "zero" not in _cache:
        pm, bits, folded, pairs, _, _ = zero_sum_problem()
        _cache["zero"] = (pm, bits, folded, pairs) + viterbi(pm, folded, pairs)
    return _cache["zero"]


def edge_case(name, K):
    """(pm, bits, folded, pairs, states, sums, last, counts) of edge_models.sweep_model(name, K): the restatement on a
    model at a numeric edge with its counter (new_counts()), once a process and read-only."""
    key = ("edge", name, K)
    if key not in _cache:
        import edge_models as E

        pm, bits, folded, pairs = E.sweep_model(name, K, False)
        counts = new_counts()
        out = viterbi(pm, folded, pairs, counts=counts)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs) + out + (counts,)
    return _cache[key]
