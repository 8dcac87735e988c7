"""Inputs and the numpy statement of fsmc_decode_pair_loglik (per pair: the likelihood of its observations from the
forward sweep alone, as mantissa and exponent, over the whole sequence and over bins of sites) for its tests.  Nothing
here calls the code under test.

The statement is a float32 restatement of the forward half of the reference's decodeBatch (HMM.cpp:725-784, NO_SSE
order, as oracle/hmm_oracle.c states it) that keeps the per-site scaling sums the reference drops:
  forward(pm, folded, pairs) -> (sums [n][S] float32, alpha [S][K][n] float32)
every numpy operation is one IEEE fp32 operation on float32 arrays, in the reference's order: the emission
(e1 + e0m1 * z) + e2m0 * t, alphaC from the top down, AU = U[k-1] * prev[k-1] + cR[k-1] * AU, term = (AU + D[k] * prev[k])
+ B[k] * alphaC[k+1], the sum over k ascending from 0.f, the scaling by 1.0f / sum.  Sequence mode: the un-normalised
half-step across the gap (emission (h + h * 0) + h * 0), then the site step; `alpha` holds what the reference's buffer
ends up holding (row t < S-1 the half-step result, the last row the scaled vector).  tests/test_pair_loglik_lists.py
proves on the CPU that `alpha` is np.array_equal to the oracle's alphaFwd for every input below and that the
log-likelihoods agree with an fp64 dense forward.

  chain(sums, lo, hi) -> (mant [n] float64, expo [n] int32): m = 1.0, e = 0; for t in [lo, hi) ascending: m = m *
    float64(sum[t]); where m != 0 and isfinite(m): m, de = frexp(m); e += de.  numpy's float64 `*` is one IEEE multiply
    and np.frexp is exact.
  expected(sums, edges) -> (mant, expo, bin_mant [n][B], bin_expo [n][B]): the total over [0, S) and chain(sums, e[b],
    e[b+1]) per bin."""
import numpy as np

from fastsmc_amd import synth
from oracle import oracle as O
from pair_common import N_HAP, SITES, cohort_pairs  # noqa: F401  (the 700-site cohort of the product path)

F32 = np.float32


def _pair_bits(folded, pairs):
    ob = np.stack([folded[a] ^ folded[b] for a, b in pairs]).astype(np.uint8)
    hb = np.stack([folded[a] & folded[b] for a, b in pairs]).astype(np.uint8)
    return ob, hb


def _next_alpha(pm, row, prev, em):
    """getNextAlphaBatched, NO_SSE branch (HMM.cpp:787-830): prev, em [n][K] float32 -> next [n][K] float32."""
    K = pm.K
    D, B, U, cR = pm.D[row], pm.B[row], pm.U[row], pm.col_ratios
    alphaC = np.empty_like(prev)
    alphaC[:, K - 1] = prev[:, K - 1]
    for k in range(K - 2, -1, -1):
        alphaC[:, k] = alphaC[:, k + 1] + prev[:, k]
    nxt = np.empty_like(prev)
    AU = np.zeros(prev.shape[0], F32)
    for k in range(K):
        if k:
            AU = U[k - 1] * prev[:, k - 1] + cR[k - 1] * AU
        term = AU + D[k] * prev[:, k]
        if k < K - 1:
            term = term + B[k] * alphaC[:, k + 1]
        nxt[:, k] = em[:, k] * term
    assert nxt.dtype == F32 and AU.dtype == F32
    return nxt


def _sum_and_scale(vec):
    """calculateScalingBatch + applyScalingBatch: the sum over k ascending from 0.f, then vec * (1.0f / sum)."""
    s = np.zeros(vec.shape[0], F32)
    for k in range(vec.shape[1]):
        s = s + vec[:, k]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scal = F32(1.0) / s
        out = vec * scal[:, None]
    assert s.dtype == F32 and out.dtype == F32
    return s, out


def forward(pm, folded, pairs):
    """(sums [n][S] float32, alpha [S][K][n] float32) of `pairs` over the whole sequence."""
    ob, hb = _pair_bits(folded, pairs)
    n, S, K = len(pairs), pm.S, pm.K
    z = np.where(ob != 0, F32(0.0), F32(1.0)).astype(F32)  # isZero
    t = np.where(hb != 0, F32(1.0), F32(0.0)).astype(F32)  # isTwo
    zero = np.zeros((n, 1), F32)

    def emission(pos):
        return (pm.e1[pos][None, :] + pm.e0m1[pos][None, :] * z[:, pos, None]) + pm.e2m0[pos][None, :] * t[:, pos, None]

    sums = np.empty((n, S), F32)
    alpha = np.empty((S, K, n), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        sums[:, 0], a = _sum_and_scale(pm.pi[None, :] * emission(0))
        alpha[0] = a.T
        for pos in range(1, S):
            if pm.sequence:
                h = pm.hom[pos][None, :]
                a = _next_alpha(pm, int(pm.gap_row_f[pos]), a, (h + h * zero) + h * zero)
                alpha[pos - 1] = a.T
                a = _next_alpha(pm, int(pm.site_row_f[pos]), a, emission(pos))
            else:
                a = _next_alpha(pm, int(pm.step_row[pos]), a, emission(pos))
            sums[:, pos], a = _sum_and_scale(a)
            alpha[pos] = a.T
    return sums, alpha


def oracle_alpha_fwd(pm, folded, pairs):
    """The oracle's alphaFwd [S][K][n], decoded batch by batch of 64 as the work list's groups are."""
    out = []
    for b0 in range(0, len(pairs), 64):
        ob, hb = _pair_bits(folded, pairs[b0:b0 + 64])
        out.append(O.decode_batch(pm, ob, hb, 0, pm.S, want_alpha_fwd=True)[2])
    return np.concatenate(out, axis=2)


def chain(sums, lo, hi):
    """(mant float64 [n], expo int32 [n]) of the sites [lo, hi)."""
    assert sums.dtype == F32
    n = sums.shape[0]
    m = np.ones(n, np.float64)
    e = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore"):
        for s in range(lo, hi):
            m = m * sums[:, s].astype(np.float64)
            ok = (m != 0) & np.isfinite(m)
            mm, de = np.frexp(m)
            m = np.where(ok, mm, m)
            e = e + np.where(ok, de, 0).astype(np.int32)
    return m, e


def expected(sums, edges=None):
    """(mant, expo, bin_mant, bin_expo); the bin outputs are None without edges."""
    mant, expo = chain(sums, 0, sums.shape[1])
    if edges is None:
        return mant, expo, None, None
    cells = [chain(sums, int(edges[b]), int(edges[b + 1])) for b in range(len(edges) - 1)]
    return mant, expo, np.stack([c[0] for c in cells], axis=1), np.stack([c[1] for c in cells], axis=1)


def log_likelihood(mant, expo):
    with np.errstate(divide="ignore"):
        return np.log(mant) + expo.astype(np.float64) * np.log(2.0)


# ---------------------------------------------------------------- the fp64 yardstick

def dense_log_likelihood(pm, folded, pair):
    """log P(observations of one pair | model) by a textbook forward in float64 on the dense transition matrices of
    tests/dense_reference.py: the sum of the logarithms of the per-site normalisers."""
    import dense_reference as DR

    x = folded[pair[0]] ^ folded[pair[1]]
    t = folded[pair[0]] & folded[pair[1]]
    Ts = {}

    def T(row):
        return Ts.setdefault(int(row), DR.dense_T(pm, int(row)))

    a = pm.pi.astype(np.float64) * DR.emission(pm, 0, x[0], t[0])
    ll = np.log(a.sum())
    a = a / a.sum()
    for p in range(1, pm.S):
        if pm.sequence:
            a = pm.hom[p].astype(np.float64) * (a @ T(pm.gap_row_f[p]))
            a = DR.emission(pm, p, x[p], t[p]) * (a @ T(pm.site_row_f[p]))
        else:
            a = DR.emission(pm, p, x[p], t[p]) * (a @ T(pm.step_row[p]))
        ll += np.log(a.sum())
        a = a / a.sum()
    return ll


# ---------------------------------------------------------------- the inputs

def _problem(K, S, seed, seq=False, n_hap=64):
    tables = synth.make_model_tables(K)
    if seq:  # (conftest.seq_problem's generator: dense sites of varying spacing)
        haps = synth.make_haps(n_hap, S, seed=seed, cm_per_mb=1.2, bp_per_site=2500, switch_per_cm=2.0)
    else:
        haps = synth.make_haps(n_hap, S, seed=seed, cm_per_mb=25.0, switch_per_cm=0.6)
    bits, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, n_hap, time=200, decoding_sequence=seq)
    return pm, bits, folded


ALL_PAIRS = O.enumerate_all_pairs(32)  # 2016 pairs of 64 haplotypes

E_200 = np.array([3, 64, 65, 130, 199], np.int32)  # an edge on a multiple of 64, a one-site bin, sites outside the bins

# name -> (K, S, pairs, sequence mode, edge sets).  70 pairs: a full group and a ragged one of 6.
#   models: every member of the lane-per-pair family is reached -- K = 2, 3 -> 16, 20 -> 32, 40 -> 48, 64, 69, 50 and 100
#     exact, 128 -- at 129 sites (two words of haplotype bits and one site)
#   sites: 1, 2, 63, 64, 65, 200 at K = 69 (129: above)
#   pairs: 1, 63, 64, 65, 200 at K = 69, S = 65
CASES = {}
for _K in (2, 3, 16, 20, 64, 128, 50, 69, 100):
    CASES[f"K{_K}"] = (_K, 129, 70, False, {})
for _S in (1, 2, 63, 64, 200):
    CASES[f"S{_S}"] = (69, _S, 70, False, {})
CASES["S200"] = (69, 200, 70, False, {"E_200": E_200, "whole": np.array([0, 200], np.int32)})
CASES["S65"] = (69, 65, 200, False, {"every_site": np.arange(66, dtype=np.int32)})
CASES["seq40"] = (40, 150, 70, True, {})
CASES["seq69"] = (69, 150, 70, True, {"E_150": np.array([0, 1, 64, 100, 150], np.int32)})
PAIR_COUNTS = (1, 63, 64, 65, 200)  # prefixes of the S65 list

_cache = {}


def case(name):
    """(pm, bits, folded, pairs, sums, edge sets) of a case; the restatement runs once a process and is read-only."""
    if name not in _cache:
        K, S, n, seq, edge_sets = CASES[name]
        pm, bits, folded = _problem(K, S, seed=100 + K + S, seq=seq)
        pairs = ALL_PAIRS[37:37 + n]
        sums, _ = forward(pm, folded, pairs)
        sums.setflags(write=False)
        _cache[name] = (pm, bits, folded, pairs, sums, edge_sets)
    return _cache[name]


def cohort_problem():
    """The 700-site cohort of the product-path tests (pair_common.cohort_files) as a prepared model: (pm, bits, folded,
    haps), generated from the same seeds, with the file reader's genetic positions (float32(float32(cM) / 100))."""
    if "cohort" not in _cache:
        tables = synth.make_model_tables(69)
        haps = synth.make_haps(N_HAP, SITES, seed=17, cm_per_mb=25.0, switch_per_cm=0.6)
        bits, derived, flipped = synth.fold_and_pack(haps.alleles)
        folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
        gen = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
        pm = O.prepare_model(tables, gen, haps.bp, derived, N_HAP, time=200)
        _cache["cohort"] = (pm, bits, folded, haps)
    return _cache["cohort"]


def cohort_sums():
    """forward() sums of pair_common.cohort_pairs() on the cohort, once a process."""
    if "cohort_sums" not in _cache:
        pm, _, folded, _ = cohort_problem()
        sums, _ = forward(pm, folded, cohort_pairs()[0])
        sums.setflags(write=False)
        _cache["cohort_sums"] = sums
    return _cache["cohort_sums"]


def zero_sum_problem():
    """The S200 problem with every emission of site 199 (the last) and of one site in the middle set to zero for the
    heterozygous observation only: a pair heterozygous at the last site has sum[199] == 0 (likelihood 0: mantissa 0,
    logarithm -inf); one heterozygous at the middle site has a zero sum there, then 0 * (1 / 0) = NaN in every later
    vector and sum.  Returns (pm, bits, folded, pairs, sums, the middle site)."""
    if "zero" not in _cache:
        import copy

        pm, bits, folded, pairs, _, _ = case("S200")
        pm = copy.deepcopy(pm)
        het = np.stack([folded[a] ^ folded[b] for a, b in pairs])
        mid = 60 + int(np.argmax(het[:, 60:140].sum(axis=0)))  # (the site of [60, 140) most pairs are heterozygous at)
        for site in (mid, 199):  # het: z = 0, t = 0 -> the emission is e1
            pm.e0m1[site] = pm.e0m1[site] + pm.e1[site]  # (the homozygous rows keep their values to within an ulp)
            pm.e1[site] = 0.0
        sums, _ = forward(pm, folded, pairs)
        sums.setflags(write=False)
        _cache["zero"] = (pm, bits, folded, pairs, sums, mid)
    return _cache["zero"]


def edge_case(name, K, seq=False):
    """(pm, bits, folded, pairs, sums) of edge_models.sweep_model(name, K, seq): the restatement on a model at a numeric
    edge, once a process and read-only."""
    key = ("edge", name, K, seq)
    if key not in _cache:
        import edge_models as E

        pm, bits, folded, pairs = E.sweep_model(name, K, seq)
        sums, _ = forward(pm, folded, pairs)
        sums.setflags(write=False)
        _cache[key] = (pm, bits, folded, pairs, sums)
    return _cache[key]
