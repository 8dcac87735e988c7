"""Inputs and the numpy statement of fsmc_decode_pair_transitions (per pair and site: the posterior probability that the
state is lower / higher than at the site before) for its tests.  Nothing here calls the code under test.

The statement is the contract of include/fastsmc_hip.h in float32, one numpy operation per IEEE operation, vectorised over
the pairs:
  transitions(pm, folded, pairs) -> (down [n][S], up [n][S], beta [S][K][n]) float32
delta is pair_loglik_lists.forward's alpha (tests/test_pair_loglik_lists.py shows that it is np.array_equal to the
oracle's alphaFwd); the backward vector is restated here: b_{S-1} = 1.f * (1.0f / sum), going down vec = b * e, BU
descending, BL ascending, the three sums over k ascending, b' = (BL + D * vec) + BU, then the sum over k ascending and
the scaling.  tests/test_pair_transition_lists.py shows that `beta` is np.array_equal to the oracle's beta buffer and that
delta * beta, normalised, gives the oracle's posterior tables.
  bin_sums(rows [n][S], edges) -> [n][B] float32: the defined fp64 order of bin_tail_length (pair_tail_lists) without
    weights: 64 slots, every 64th site ascending, the tree with strides 32 ... 1, rounded once to float.

The yardstick is the two-slice posterior in float64 on the dense transition matrices of tests/dense_reference.py:
  xi_t(k, j) ~ alpha_{t-1}[k] * T[k, j] * e_t[j] * beta_t[j], normalised, summed below / on / above the diagonal
(dense_transitions: one pair)."""
import numpy as np

from pair_loglik_lists import ALL_PAIRS, _pair_bits, _sum_and_scale, forward, zero_sum_problem  # noqa: F401
from pair_sample_lists import (CASES, LIMITS_RICH_PLANNED, LIMITS_RICH_REFUSED, PAIR_COUNTS, RICH_PAIRS,  # noqa: F401
                               planned, problem)
from pair_tail_lists import _slots_and_tree

F32 = np.float32

# the lane-per-pair members at 129 sites; the site counts at K = 69; the rich 700-site case
MODEL_CASES = ("K2", "K3", "K20", "dense40", "K64", "K69", "K50", "K100", "K128")
SITE_CASES = ("S1", "S2", "S3", "S4", "S5", "S63", "S64", "S65", "S200")
from pair_viterbi_lists import CHUNKS_S65  # noqa: E402,F401  (the chunk lengths of the GPU test on the 65-site case)

CHUNKS_RICH = (1, 2, 27, 699, 700)  # chunk lengths of the GPU test on the rich case: an edge at t = 1 (1), at S - 1 (1, 699)

# the largest |statement - fp64 yardstick| over YARDSTICK (three pairs each), measured on the CPU with the code of this
# file (test_statement_agrees_with_dense prints it); the test asserts four times this: fp32 sums of up to 128 products,
# the margin covers other seeds, not the code under test
YARDSTICK = ("K2", "K3", "K20", "K64", "K69", "K128", "S2", "S5", "rich")
YARDSTICK_PAIRS = 3
MEASURED_MAX_ABS_DIFF = 2.21e-7
YARDSTICK_BOUND = 4 * MEASURED_MAX_ABS_DIFF

# bin edges of the 200-site case: the whole sequence; single sites; 64 and 65 sites; edges at no multiple of four
EDGES = {
    "whole": np.array([0, 200], np.int32),
    "single": np.arange(201, dtype=np.int32),
    "w64_65": np.array([0, 64, 129, 193], np.int32),
    "odd": np.array([3, 10, 11, 77, 199], np.int32),  # (a bin of one site among them; site 0 and the last left out)
}


def transitions(pm, folded, pairs, alpha=None):
    """(down [n][S], up [n][S], beta [S][K][n]) float32 of `pairs` over the whole sequence."""
    assert not pm.sequence and pm.K <= 128
    if alpha is None:
        _, alpha = forward(pm, folded, pairs)
    ob, hb = _pair_bits(folded, pairs)
    n, S, K = len(pairs), pm.S, pm.K
    z = np.where(ob != 0, F32(0.0), F32(1.0)).astype(F32)
    tw = np.where(hb != 0, F32(1.0), F32(0.0)).astype(F32)
    down, up = np.zeros((n, S), F32), np.zeros((n, S), F32)
    beta = np.empty((S, K, n), F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        _, b = _sum_and_scale(np.ones((n, K), F32))
        beta[S - 1] = b.T
        for t in range(S - 1, 0, -1):
            row = int(pm.step_row[t])
            D, B, U, RR = pm.D[row], pm.B[row], pm.U[row], pm.RR[row]
            em = (pm.e1[t][None, :] + pm.e0m1[t][None, :] * z[:, t, None]) + pm.e2m0[t][None, :] * tw[:, t, None]
            vec = b * em
            BU = np.zeros((n, K), F32)
            for k in range(K - 2, -1, -1):
                BU[:, k] = U[k] * vec[:, k + 1] + RR[k] * BU[:, k + 1]
            BL = np.zeros((n, K), F32)
            for k in range(1, K):
                BL[:, k] = BL[:, k - 1] + B[k - 1] * vec[:, k - 1]
            Dv = D[None, :] * vec
            f = alpha[t - 1].T
            d, s, u = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
            for k in range(K):
                d = d + f[:, k] * BL[:, k]
                s = s + f[:, k] * Dv[:, k]
                u = u + f[:, k] * BU[:, k]
            zsum = (d + s) + u
            r = F32(1.0) / zsum
            down[:, t], up[:, t] = d * r, u * r
            assert vec.dtype == BU.dtype == BL.dtype == Dv.dtype == d.dtype == zsum.dtype == r.dtype == F32
            _, b = _sum_and_scale((BL + Dv) + BU)
            beta[t - 1] = b.T
    assert down.dtype == up.dtype == F32
    return down, up, beta


def bin_sums(rows, edges):
    """[n][B] float32: per bin the defined fp64 sum of rows[:, e[b]:e[b+1]]."""
    rows = np.asarray(rows)
    assert rows.dtype == F32 and rows.ndim == 2
    x = rows.astype(np.float64)
    out = np.empty((rows.shape[0], len(edges) - 1), F32)
    with np.errstate(invalid="ignore"):
        for b in range(len(edges) - 1):
            out[:, b] = _slots_and_tree(x, int(edges[b]), int(edges[b + 1])).astype(F32)
    return out


# ---------------------------------------------------------------- the fp64 yardstick

def dense_transitions(pm, folded, pair):
    """(down [S], up [S], xi_rows [S][K], posterior [S][K]) of one pair in float64: the two-slice posterior of (t-1, t)
    summed below / above the diagonal, its sums over j (row t: the posterior of site t-1 as the two-slice table has it),
    and the posterior of the textbook forward-backward."""
    import dense_reference as DR

    S, K = pm.S, pm.K
    x = folded[pair[0]] ^ folded[pair[1]]
    a2 = folded[pair[0]] & folded[pair[1]]
    em = [DR.emission(pm, p, x[p], a2[p]) for p in range(S)]
    Ts = {}

    def T(p):
        return Ts.setdefault(int(pm.step_row[p]), DR.dense_T(pm, int(pm.step_row[p])))

    al, be = np.zeros((S, K)), np.zeros((S, K))
    a = pm.pi.astype(np.float64) * em[0]
    al[0] = a / a.sum()
    for p in range(1, S):
        a = em[p] * (al[p - 1] @ T(p))
        al[p] = a / a.sum()
    be[S - 1] = 1.0 / K
    for p in range(S - 2, -1, -1):
        b = T(p + 1) @ (em[p + 1] * be[p + 1])
        be[p] = b / b.sum()
    post = al * be
    post /= post.sum(axis=1, keepdims=True)
    down, up, rows = np.zeros(S), np.zeros(S), np.zeros((S, K))
    for p in range(1, S):
        xi = al[p - 1][:, None] * T(p) * (em[p] * be[p])[None, :]
        xi /= xi.sum()
        down[p], up[p] = np.tril(xi, -1).sum(), np.triu(xi, 1).sum()
        rows[p] = xi.sum(axis=1)
    return down, up, rows, post


# ---------------------------------------------------------------- the inputs

_cache = {}


def case(name, first=None):
    """(pm, bits, folded, pairs, down, up) of a case of pair_sample_lists (its first `first` pairs), read-only, once a
    process."""
    key = ("case", name, first)
    if key not in _cache:
        pm, bits, folded, pairs, alpha = problem(name)
        m = len(pairs) if first is None else first
        down, up, _ = transitions(pm, folded, pairs[:m], alpha=alpha[:, :, :m])
        down.setflags(write=False)
        up.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs[:m], down, up)
    return _cache[key]


def edge_case(name, K):
    """(pm, bits, folded, pairs, down, up) of edge_models.sweep_model(name, K): the restatement on a model at a numeric
    edge (subnormal entries, states at exactly +0, every state equal, identical and complementary haplotypes), once a
    process and read-only."""
    key = ("edge", name, K)
    if key not in _cache:
        import edge_models as E

        pm, bits, folded, pairs = E.sweep_model(name, K, False)
        down, up, _ = transitions(pm, folded, pairs)
        down.setflags(write=False)
        up.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs, down, up)
    return _cache[key]


DOMINANT_RANGES = ((30, 60), (70, 110))  # the site of each range most pairs are heterozygous at: state 0 holds
# everything at the first, state K - 1 at the second


def dominant_case():
    """The K20 problem with the heterozygous emission of every state but state 0 set to zero at one site and of every state
    but the top one at another (DOMINANT_RANGES) (the homozygous rows keep their values to within an ulp): a pair heterozygous there has
    all its mass in one state, so p_up[lo] = p_down[lo + 1] = 0.f and p_down[hi] = p_up[hi + 1] = 0.f exactly.  (pm, bits,
    folded, pairs, down, up, het [pairs][2] bool, (lo, hi))."""
    if "dominant" not in _cache:
        import copy

        pm, bits, folded, pairs, _ = problem("K20")
        pm = copy.deepcopy(pm)
        x = np.stack([folded[a] ^ folded[b] for a, b in pairs])
        sites = tuple(r0 + int(np.argmax(x[:, r0:r1].sum(axis=0))) for r0, r1 in DOMINANT_RANGES)
        for site, keep in zip(sites, (0, pm.K - 1)):
            gone = np.arange(pm.K) != keep
            pm.e0m1[site][gone] = pm.e0m1[site][gone] + pm.e1[site][gone]
            pm.e1[site][gone] = 0.0
        het = x[:, sites] != 0
        down, up, _ = transitions(pm, folded, pairs)
        _cache["dominant"] = (pm, bits, folded, pairs, down, up, het, sites)
    return _cache["dominant"]


def cohort_transitions():
    """(down, up) of pair_common.cohort_pairs() on the 700-site cohort, once a process."""
    if "cohort" not in _cache:
        from pair_common import cohort_pairs
        from pair_loglik_lists import cohort_problem

        pm, _, folded, _ = cohort_problem()
        down, up, _ = transitions(pm, folded, cohort_pairs()[0])
        _cache["cohort"] = (down, up)
    return _cache["cohort"]


def zero_sum_case():
    """(pm, bits, folded, pairs, down, up, bad [pairs] bool) of pair_loglik_lists.zero_sum_problem(): `bad` marks the
    pairs with a zero or NaN scaling sum somewhere."""
    if "zero" not in _cache:
        pm, bits, folded, pairs, sums, _ = zero_sum_problem()
        with np.errstate(invalid="ignore"):
            bad = ~((sums > 0) & np.isfinite(sums)).all(axis=1)
        down, up, _ = transitions(pm, folded, pairs)
        _cache["zero"] = (pm, bits, folded, pairs, down, up, bad)
    return _cache["zero"]
