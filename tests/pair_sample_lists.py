"""Inputs and the numpy statement of fsmc_decode_pair_samples (per pair: state sequences drawn from the joint posterior
over sequences, forward filtering with backward sampling) for its tests.  Nothing here calls the code under test.

The statement is the contract of include/fastsmc_hip.h in float32, one numpy operation per IEEE operation and one numpy
comparison per comparison, vectorised over the pairs and their samples (samples are independent given the forward vectors):
  philox4x32_10(counter [..., 4] uint32, key [..., 2] uint32) -> [..., 4] uint32, in integer arithmetic
  uniforms(seed, hap_a, hap_b, rs, t) -> float32 [len(rs)]: key = (seed & 0xffffffff, seed >> 32), counter = (t >> 2, r,
    hap_a, hap_b), u = float32(out[t & 3] >> 8) * 2^-24
  pick(w [..., K], u [...]) -> states [...]: c = the running sum over i ascending from 0.f, x = u * c[K-1],
    min(K-1, #{i : c[i] <= x})
  weights(pm, row, delta_t [P][K], j [P][n]) -> w [P][n][K]: B[j] * delta[i] above j, D[j] * delta[j] at j, (U[i] * delta[i]) * g
    below, g = 1.f at i = j-1 and g = g * cR[i+1] for i = j-2 .. 0
  sample(pm, folded, pairs, n or rs, seed) -> states [pairs][n][S] uint8
delta is pair_loglik_lists.forward's alpha: tests/test_pair_loglik_lists.py shows that it is np.array_equal to the
oracle's alphaFwd.  `variant` swaps the contract for a wrong sampler ("B[i]": the lower-triangle weight read at the
predecessor instead of the successor; "no-cR": the product of column ratios left out), so that a test can show that the
yardstick tells them apart.

The yardstick is the exact joint posterior over paths in float64 on the dense transition matrices of
tests/dense_reference.py (dense_path_posterior: every path of a tiny model)."""
import itertools

import numpy as np

from pair_loglik_lists import (ALL_PAIRS, CASES as LL_CASES, PAIR_COUNTS, _problem, forward,  # noqa: F401
                               case as ll_case, zero_sum_problem)
from pair_viterbi_lists import CASES as V_CASES, CHUNKS_RICH, CHUNKS_S65, _rich_problem  # noqa: F401

F32 = np.float32
U32 = np.uint32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter, key, output (the published known answers of Philox4x32-10)
PHILOX_KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """[..., 4] uint32 counters and [..., 2] uint32 keys (broadcast against each other) -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # (32 x 32 bits: exact in uint64)
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(U32)


def uniforms(seed, hap_a, hap_b, rs, t):
    """u of (seed, (hap_a, hap_b), sample r, site t): hap_a, hap_b and rs broadcast against each other; float32, exact, in
    [0, 1)."""
    hap_a, hap_b, rs = np.broadcast_arrays(np.asarray(hap_a, np.uint64), np.asarray(hap_b, np.uint64),
                                           np.asarray(rs, np.uint64))
    counter = np.empty(rs.shape + (4,), np.uint64)
    counter[..., 0], counter[..., 1], counter[..., 2], counter[..., 3] = t >> 2, rs, hap_a, hap_b
    out = philox4x32_10(counter, np.array([seed & MASK, (seed >> 32) & MASK], np.uint64))
    u = (out[..., t & 3] >> U32(8)).astype(F32) * F32(2.0 ** -24)
    assert u.dtype == F32
    return u


def pick(w, u):
    """w [..., K] float32, u [...] float32 -> states [...] int64."""
    K = w.shape[-1]
    c = np.empty_like(w)
    run = np.zeros(w.shape[:-1], F32)
    for i in range(K):
        run = run + w[..., i]
        c[..., i] = run
    with np.errstate(invalid="ignore", over="ignore"):
        x = u * c[..., K - 1]
        count = (c <= x[..., None]).sum(axis=-1)
    assert c.dtype == F32 and x.dtype == F32
    return np.minimum(K - 1, count).astype(np.int64)


def weights(pm, row, delta, j, variant=None):
    """The weights of the predecessors of the states j [P][n] given delta [P][K] of the site before: [P][n][K] float32."""
    K = pm.K
    D, B, U, cR = pm.D[row], pm.B[row], pm.U[row], pm.col_ratios
    w = np.empty(j.shape + (K,), F32)
    g = np.ones(j.shape, F32)
    Bj, Dj = B[j], D[j]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i in range(K - 1, -1, -1):
            d = delta[:, i, None]
            if i + 1 < K:
                g = np.where(i + 1 < j, g if variant == "no-cR" else g * cR[i + 1], F32(1.0))
            above = (B[i] if variant == "B[i]" else Bj) * d
            at = Dj * d
            below = (U[i] * d) * g
            assert g.dtype == F32 and above.dtype == F32 and at.dtype == F32 and below.dtype == F32
            w[..., i] = np.where(i > j, above, np.where(i == j, at, below))
    return w


def sample(pm, folded, pairs, n, seed, variant=None, alpha=None):
    """states [pairs][n][S] uint8 of the work list `pairs`; n a count (r = 0 .. n-1) or a sequence of r."""
    assert not pm.sequence and pm.K <= 128
    rs = (np.arange(n) if np.isscalar(n) else np.asarray(n))[None, :]
    if alpha is None:
        _, alpha = forward(pm, folded, pairs)
    S, K, P = pm.S, pm.K, len(pairs)
    a = np.array([p[0] for p in pairs], np.uint64)[:, None]
    b = np.array([p[1] for p in pairs], np.uint64)[:, None]
    out = np.empty((P, rs.shape[1], S), np.uint8)
    w = np.broadcast_to(alpha[S - 1].T[:, None, :], (P, rs.shape[1], K))
    j = pick(w, uniforms(seed, a, b, rs, S - 1))
    out[:, :, S - 1] = j
    for t in range(S - 2, -1, -1):
        j = pick(weights(pm, int(pm.step_row[t + 1]), alpha[t].T, j, variant), uniforms(seed, a, b, rs, t))
        out[:, :, t] = j
    return out


# ---------------------------------------------------------------- the fp64 yardstick

def dense_path_posterior(pm, folded, pair):
    """P(path | observations of the pair) for every path of a tiny model, float64 on the dense matrices: an array of
    shape [K] * S."""
    import dense_reference as DR

    S, K = pm.S, pm.K
    x = folded[pair[0]] ^ folded[pair[1]]
    t = folded[pair[0]] & folded[pair[1]]
    joint = np.empty((K,) * S)
    pi = pm.pi.astype(np.float64)
    em = [DR.emission(pm, pos, x[pos], t[pos]) for pos in range(S)]
    T = [None] + [DR.dense_T(pm, int(pm.step_row[pos])) for pos in range(1, S)]
    for path in itertools.product(range(K), repeat=S):
        p = pi[path[0]] * em[0][path[0]]
        for pos in range(1, S):
            p *= T[pos][path[pos - 1], path[pos]] * em[pos][path[pos]]
        joint[path] = p
    return joint / joint.sum()


def chi2_quantile_999(dof):
    """The 99.9th percentile of chi-squared with `dof` degrees of freedom: scipy's where it is installed, otherwise the
    Wilson-Hilferty approximation (z = 3.090232306)."""
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(0.999, dof))
    except ImportError:
        z = 3.090232306167813
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3


def pearson(states, posterior):
    """(statistic, cells) of sampled paths [N][S] against the exact path posterior, over the cells with expectation >= 5."""
    N, S = states.shape
    K = posterior.shape[0]
    idx = np.zeros(N, np.int64)
    for pos in range(S):
        idx = idx * K + states[:, pos]
    counts = np.bincount(idx, minlength=K ** S).astype(np.float64)
    expect = posterior.reshape(-1) * N
    use = expect >= 5
    return float((((counts - expect) ** 2) / np.where(use, expect, 1.0))[use].sum()), int(use.sum())


# ---------------------------------------------------------------- the inputs

TINY_SEEDS = (1, 2, 3)
TINY_N = 100_000


TINY_BOUNDARIES = (0.0, 3000.0, 6000.0, np.inf)  # P(interval) = 0.18, 0.15, 0.67: column ratios 0.82 and 4.5


def tiny_problem():
    """K = 3, S = 4 (81 paths): three uneven intervals, so that the column ratios are not 1 (the quantile grids of
    synth.make_model_tables have equal intervals), on a map of 100 cM / Mb, where a step neither keeps the state nor
    forgets it; the pair of the first 200 with the most heterozygous sites.  (pm, bits, folded, pair)."""
    if "tiny" not in _cache:
        from fastsmc_amd import synth
        from oracle import oracle as O

        tables = synth.make_model_tables(3, boundaries=np.array(TINY_BOUNDARIES))
        haps = synth.make_haps(64, 4, seed=23, cm_per_mb=100.0, switch_per_cm=0.6)
        bits, derived, flipped = synth.fold_and_pack(haps.alleles)
        folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
        pm = O.prepare_model(tables, (haps.cm / 100.0).astype(np.float32), haps.bp, derived, 64, time=200)
        het = np.array([(folded[a] ^ folded[b]).sum() for a, b in ALL_PAIRS[:200]])
        _cache["tiny"] = (pm, bits, folded, ALL_PAIRS[int(np.argmax(het))])
    return _cache["tiny"]


# the array-mode cases of pair_viterbi_lists (models K = 2 ... 128 at 129 sites; 1 ... 200 sites at K = 69; 200 pairs at
# 65 sites; the rich 700-site case) and more site counts at K = 69: name -> (K, S, pairs)
CASES = dict(V_CASES)
for _S in (3, 4, 5):
    CASES[f"S{_S}"] = (69, _S, 70)
N_MODELS = 3           # samples a pair of the model and site cases
SEED_MODELS = 20261020
N_COUNTS = (1, 2, 33, 64)
SEEDS = (0, 1, 2 ** 64 - 1)
RICH_N = 2             # samples a pair of the rich case
RICH_PAIRS = 70        # two groups
# workspace limits of the GPU test on the rich case (two groups: two waves wanted).  A wave's smallest slot there is 53
# rows (27 sites a chunk, 26 checkpoints) of 18 KiB, 954 KiB: two mebibytes hold two of them, one mebibyte one, and 600 KiB
# -- enough for the Viterbi kernel's back-pointers, a quarter the size -- none, like 16 KiB
LIMITS_RICH_PLANNED = (2 << 20, 1 << 20)
LIMITS_RICH_REFUSED = (600 << 10, 16 << 10)
COHORT_N = 2           # samples a pair of the product-path test

MARGINAL_PAIRS = 4
MARGINAL_N = 4096
MARGINAL_SEED = 7


def planned(S, member, waves_wanted, limit):
    """(chunk sites, chunks, waves) of fsmc_decode_pair_samples under a workspace limit, as its planner states them: a
    wave's slot is chunk rows of forward vectors (ceil(member / 4) x 1024 bytes a site) and a checkpoint of the same size a
    chunk; the waves are what the limit holds of the smallest slot (about sqrt(S) sites a chunk); the chunk is the whole
    sequence halved (rounding up, never below that smallest chunk) until the waves' slots fit the limit."""
    row = (member + 3) // 4 * 1024

    def slot(c):
        return (c + -(-S // c)) * row

    c_min = min(S, max(1, int(np.ceil(np.sqrt(S)))))
    waves = min(waves_wanted, limit // slot(c_min))
    assert waves >= 1
    c = S
    while c > c_min and waves * slot(c) > limit:
        c = max(c_min, (c + 1) // 2)
    return c, -(-S // c), waves


_cache = {}


def problem(name):
    """(pm, bits, folded, pairs, alpha [S][K][pairs]) of a case; the forward restatement runs once a process."""
    key = ("problem", name)
    if key not in _cache:
        K, S, n = CASES[name]
        if name in ("rich", "dense40"):
            pm, bits, folded = _rich_problem(K, S)
            pairs = ALL_PAIRS[37:37 + n]
        elif name in LL_CASES:
            pm, bits, folded, pairs, _, _ = ll_case(name)
        else:
            pm, bits, folded = _problem(K, S, seed=100 + K + S)
            pairs = ALL_PAIRS[37:37 + n]
        _, alpha = forward(pm, folded, pairs)
        alpha.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs, alpha)
    return _cache[key]


def case(name, n=N_MODELS, seed=SEED_MODELS, first=None):
    """(pm, bits, folded, pairs, states [pairs][n][S]) of a case (its first `first` pairs), read-only, once a process."""
    key = ("case", name, n, seed, first)
    if key not in _cache:
        pm, bits, folded, pairs, alpha = problem(name)
        m = len(pairs) if first is None else first
        states = sample(pm, folded, pairs[:m], n, seed, alpha=alpha[:, :, :m])
        states.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs[:m], states)
    return _cache[key]


def cohort_samples():
    """sample() of pair_common.cohort_pairs() on the 700-site cohort, COHORT_N samples a pair, once a process."""
    if "cohort" not in _cache:
        from pair_common import cohort_pairs
        from pair_loglik_lists import cohort_problem

        pm, _, folded, _ = cohort_problem()
        out = sample(pm, folded, cohort_pairs()[0], COHORT_N, SEED_MODELS)
        out.setflags(write=False)
        _cache["cohort"] = out
    return _cache["cohort"]


def zero_sum_case(n=N_MODELS, seed=SEED_MODELS):
    """(pm, bits, folded, pairs, states, bad [pairs] bool) of pair_loglik_lists.zero_sum_problem(): `bad` marks the pairs
    with a zero or NaN scaling sum somewhere."""
    if "zero" not in _cache:
        pm, bits, folded, pairs, sums, _ = zero_sum_problem()
        with np.errstate(invalid="ignore"):
            bad = ~((sums > 0) & np.isfinite(sums)).all(axis=1)
        _cache["zero"] = (pm, bits, folded, pairs, sample(pm, folded, pairs, n, seed), bad)
    return _cache["zero"]


def edge_case(name, K, n=N_MODELS, seed=SEED_MODELS):
    """(pm, bits, folded, pairs, states) of edge_models.sweep_model(name, K): the restatement on a model at a numeric
    edge, once a process and read-only."""
    key = ("edge", name, K, n, seed)
    if key not in _cache:
        import edge_models as E

        pm, bits, folded, pairs = E.sweep_model(name, K, False)
        states = sample(pm, folded, pairs, n, seed)
        states.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs, states)
    return _cache[key]
