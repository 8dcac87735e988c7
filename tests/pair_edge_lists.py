"""The edge models of tests/edge_models.py as inputs of the five posterior-reducing decodePairs entry points
(fsmc_decode_pair_posteriors, _minima, _bins, _cdf, _tail_summaries): the cases, the parameters of each call, the expected
values, and a comparison of bit patterns.  Nothing here calls the code under test.

Every parameter that has to meet a value of the data -- a quantile equal to a running sum, a scale of the expected times at
which the means are a few subnormal ulps -- is read off the ORACLE's posteriors of the case, and every expected value is one
of the existing numpy statements (pair_cdf_lists, pair_tail_lists, pair_bins_lists, pair_minima_lists,
pair_common.posterior_tables) applied to them.  tests/test_pair_edge_lists.py proves on the CPU which regime each case
reaches; tests/test_gpu_pair_edges.py runs the library on them.

A case is (builder, K, seq): 96 pairs, a full group and a half-full one (edge_models.N_PAIRS), 400 sites in array mode
and 300 in sequence mode.  K = 69 is an exact member, K = 33 a padded one (48: ghost states above the model's), K = 200 a
wave-group member."""
import copy
import functools

import numpy as np

import edge_models as E
import pair_bins_lists as BL
import pair_cdf_lists as CL
import pair_minima_lists as ML
import pair_tail_lists as TL
from pair_common import posterior_tables

BUILDERS = {
    "benign": lambda K, seq: E.benign(K, seq),
    "subnormal-1e-30": lambda K, seq: E.subnormal(K, 1e-30, seq),
    "subnormal-1e-38": lambda K, seq: E.subnormal(K, 1e-38, seq),
    "zero-states": lambda K, seq: E.zero_states(K),
    "degenerate": lambda K, seq: E.degenerate(K, seq),
    "degenerate_with_dead_states": lambda K, seq: E.degenerate_with_dead_states(K, seq),
}
EDGE_BUILDERS = [name for name in BUILDERS if name != "benign"]
K69_CASES = [(name, 69, False) for name in EDGE_BUILDERS]
K33_CASES = [(name, 33, False) for name in EDGE_BUILDERS]
K200_CASES = [(name, 200, False) for name in ("subnormal-1e-30", "degenerate_with_dead_states")]  # dump-fed reducers only
SEQ_CASE = ("subnormal-1e-30", 69, True)
DUMP_CASES = K69_CASES + K33_CASES + K200_CASES + [SEQ_CASE]  # cdf and tail summaries
POSTERIOR_CASES = [(name, K, False) for K in (69, 33, 200) for name in ("subnormal-1e-30", "degenerate_with_dead_states")]
MINIMA_CASES = [(name, 69, False) for name in ("benign", "degenerate", "subnormal-1e-30")]
BINS_CASES = MINIMA_CASES + [("degenerate", 33, False)]

TINY = np.finfo(np.float32).tiny  # the smallest normal float32
ULP = np.float32(2.0 ** -149)     # the smallest positive subnormal: np.float32(1e-45)
assert ULP == np.float32(1e-45) and ULP > 0


def case_id(case):
    return f"{case[0]}-K{case[1]}{'-seq' if case[2] else ''}"


def is_subnormal(a):
    """Non-zero and below the normal range of the array's own type."""
    a = np.abs(np.asarray(a))
    return (a > 0) & (a < np.finfo(a.dtype).tiny)


@functools.lru_cache(maxsize=None)
def model(name, K, seq=False):
    """(pm, bits, folded, pairs) of a builder, built once a process and shared by the tests: read-only."""
    return BUILDERS[name](K, seq)


@functools.lru_cache(maxsize=None)
def posteriors(case):
    """[(post [S][K][64] float32, pairs of the batch)]: the oracle's posteriors of the case's 96 pairs, read-only."""
    pm, _, folded, pairs = model(*case)
    batches = CL.oracle_posteriors(pm, folded, pairs)
    for post, _ in batches:
        post.setflags(write=False)
    return tuple(batches)


@functools.lru_cache(maxsize=None)
def running_sums(case):
    """cdf [K][n][S] float32: the fp32 running sum over the states of every pair and site, in the order of
    pair_cdf_lists.reduce (ascending k, one add a state).  Only the parameters below and the regime proofs read it; the
    expected values come from CL.reduce."""
    parts = []
    for post, n in posteriors(case):
        S, K, _ = post.shape
        cdf = np.zeros((S, post.shape[2]), np.float32)
        out = np.empty((K, n, S), np.float32)
        for k in range(K):
            cdf = cdf + post[:, k, :]
            out[k] = cdf[:, :n].T
        parts.append(out)
    out = np.concatenate(parts, axis=1)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- cuts and quantiles

def dead_state(K):
    """The middle one of the states that zero_states and degenerate_with_dead_states kill."""
    return K // 2


def cuts(case):
    """At most 8 state cuts: the first state, 4, 8, 32 (half the states of a model that has no more than 64), all K, and
    round the middle dead state d = K / 2: the cut d - 1 ends on the live state below it, d just below it, d + 1 just
    above -- the tails of the last two are equal bit for bit where state d is dead."""
    K = case[1]
    d = dead_state(K)
    out = sorted({1, 4, 8, 32 if K > 64 else K // 2, K, d - 1, d, d + 1})
    assert len(out) <= 8 and out[0] >= 1 and out[-1] == K
    return out


def most_common(values):
    """(value, count) of the most frequent bit pattern of a float32 array."""
    v, c = np.unique(np.ascontiguousarray(values, np.float32).view(np.uint32), return_counts=True)
    i = int(np.argmax(c))
    return v[i:i + 1].view(np.float32)[0], int(c[i])


@functools.lru_cache(maxsize=None)
def quantile_set(case):
    """dict name -> float32 quantile, at most 8, read off the oracle's running sums of the case:
      "eq":  the most common value of cdf[K/2 - 1] (the degenerate builders put thousands of cells on it: `>=` is met
             with equality there, and with dead states the running sum stays on it for a state);
      "eq+", "eq-": its float32 neighbours;
      "sub": the median of the positive subnormal values of cdf[3], where the case has any -- of cdf[2], [1] or [0] where
             cdf[3] has none (33 states: the running sum leaves the subnormal range after the first state);
      "ulp": the smallest positive subnormal;  "one": 1.0."""
    K = case[1]
    cdf = running_sums(case)
    eq, _ = most_common(cdf[K // 2 - 1])
    out = {"eq": eq, "eq+": np.nextafter(eq, np.float32(2)), "eq-": np.nextafter(eq, np.float32(0))}
    for k in (3, 2, 1, 0):
        sub = np.sort(cdf[k][is_subnormal(cdf[k])])
        if sub.size:
            out["sub"] = sub[sub.size // 2]
            break
    out["ulp"] = ULP
    out["one"] = np.float32(1.0)
    assert len(out) <= 8 and all(0 < q <= 1 and q.dtype == np.float32 for q in out.values())
    return out


def quantiles(case):
    return list(quantile_set(case).values())


@functools.lru_cache(maxsize=None)
def expected_cdf(case):
    """(tail [n_cuts][96][S] float32, qstate [n_q][96][S] int32): CL.reduce with cuts(case) and quantiles(case)."""
    parts = [CL.reduce(post, n, cuts(case), quantiles(case)) for post, n in posteriors(case)]
    tail = np.concatenate([p[0] for p in parts], axis=1)
    qstate = np.concatenate([p[1] for p in parts], axis=1)
    tail.setflags(write=False)
    qstate.setflags(write=False)
    return tail, qstate


# ---------------------------------------------------------------- bin edges and site weights

def edge_sets(S):
    """"wide": [0, 1, 65, 66, 330, 400] -- a one-site bin, a 64-site bin that starts off a multiple of 64, a bin of 264 sites
    (more than the 256 = kPairBinsBlock strides of 64 a lane loads together), a last bin of 70; with the 300 sites of
    sequence mode [0, 1, 33, 300] (one site, 32 sites, 267 sites).  "sixteen": 0, 16, ... -- bins of sixteen sites."""
    wide = [0, 1, 65, 66, 330, 400] if S >= 400 else [0, 1, 33, S]
    return {"wide": np.array(wide, np.int32), "sixteen": np.arange(0, S + 1, 16, dtype=np.int32)}


def site_weights(S):
    """float32 [S]: normal values in [0.001, 0.051), every fifth site a subnormal (a random multiple below 2^20 of the
    smallest one), every seventh an exact zero, sites 0 ... 64 subnormal or zero throughout -- so the first two bins of
    "wide" and the first four of "sixteen" have subnormal lengths whatever the tail --, site 200 holds 2^100."""
    rng = np.random.default_rng(400)
    w = (rng.random(S) * 0.05 + 0.001).astype(np.float32)
    sub = (rng.integers(1, 1 << 20, S).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    t = np.arange(S)
    w[(t % 5 == 1) | (t < 65)] = sub[(t % 5 == 1) | (t < 65)]
    w[t % 7 == 3] = 0.0
    w[200] = np.float32(2.0 ** 100)
    assert np.isfinite(w).all() and is_subnormal(w).sum() > 65 and (w == 0).sum() > 40 and (w >= TINY).sum() > 100
    return w


@functools.lru_cache(maxsize=None)
def expected_tail(case, edges_name):
    """(tail_sum [n_cuts][S] float64, bin_tail_mean, bin_tail_length [n_cuts][96][B] float32): TL.expected of
    expected_cdf's tails with edge_sets and site_weights."""
    S = model(*case)[0].S
    want = TL.expected(expected_cdf(case)[0], edge_sets(S)[edges_name], site_weights(S))
    for w in want:
        w.setflags(write=False)
    return want


# ---------------------------------------------------------------- expected coalescence times

TIMES = ("own", "2^-140", "few-ulp", "+0", "-0")


def scaled_times(pm, exponent):
    """float32(float64(exp_times) * 2^exponent): one rounding, into the subnormal range where it falls there."""
    return (pm.exp_times.astype(np.float64) * 2.0 ** exponent).astype(np.float32)


@functools.lru_cache(maxsize=None)
def few_ulp_exponent(case):
    """The power of two that takes the largest posterior mean of the case's own rows to 8 ... 16 subnormal ulps: the
    products post * time and their sums over the states are then small integers of ulps, rounded at every step, and the
    pairs of a site and the sites of a bin tie en masse.  Near -150 for these models."""
    top = float(rows(case, "own")[0].max())
    assert top > 0
    return int(np.floor(np.log2(16.0 * 2.0 ** -149 / top)))


def times(case, variant):
    """The expected coalescence times passed to the posteriors, minima and bins calls, float32 [K]."""
    pm = model(*case)[0]
    if variant == "own":
        return pm.exp_times.copy()
    if variant == "2^-140":
        return scaled_times(pm, -140)
    if variant == "few-ulp":
        return scaled_times(pm, few_ulp_exponent(case))
    assert variant in ("+0", "-0")
    return np.full(pm.K, 0.0 if variant == "+0" else -0.0, np.float32)


def model_with_times(case, variant):
    """A shallow copy of the case's PreparedModel whose exp_times are times(case, variant): the oracle's per-pair
    outputs read them from the model."""
    pm = copy.copy(model(*case)[0])
    pm.exp_times = times(case, variant)
    return pm


@functools.lru_cache(maxsize=None)
def rows(case, variant):
    """(mean [96][S] float32, MAP [96][S] int32): ML.oracle_rows with the variant's times, read-only."""
    _, _, folded, pairs = model(*case)
    mean, mp = ML.oracle_rows(model_with_times(case, variant), folded, pairs)
    mean.setflags(write=False)
    mp.setflags(write=False)
    return mean, mp


def expected_minima(case, variant, split=None):
    """(min_mean, argmin_mean, min_map, argmin_map) over the 96 pairs: ML.first_minima; with ``split`` the chain of two
    calls, pairs [0, split) and then [split, 96) with pair_base = split (ML.continue_minima)."""
    mean, mp = rows(case, variant)
    if split is None:
        return ML.first_minima(mean) + ML.first_minima(mp)
    out = ()
    for r in (mean, mp):
        m, a = ML.first_minima(r[:split])
        out += ML.continue_minima(m, a, r[split:], split)
    return out


def expected_bins(case, variant, edges_name):
    """BL.expected of rows(case, variant) over edge_sets."""
    mean, mp = rows(case, variant)
    return BL.expected(mean, mp, edge_sets(mean.shape[1])[edges_name])


def expected_posteriors(case, variant, acc=None, pairs=slice(None)):
    """(rows [n][K][S], sum [K][S]): pair_common.posterior_tables with the variant's times, the sum continued in a copy of
    ``acc`` (zeros if None)."""
    _, _, folded, all_pairs = model(*case)
    return posterior_tables(model_with_times(case, variant), folded, all_pairs[pairs], None if acc is None else acc.copy())


# ---------------------------------------------------------------- comparing bit patterns

def bits(a):
    """The array as unsigned integers of its item size: -0.0 and +0.0, or two NaNs of different payload, differ."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what=""):
    """Float arrays as bit patterns (so -0.0 against +0.0 fails, which == and np.array_equal let pass), integer arrays
    with np.array_equal; dtype and shape first."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} cells differ"
        return
    diff = bits(got) != bits(want)
    if diff.any():
        at = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} cells differ in their bits, the first at {at}: "
                             f"got {got[at]!r} ({bits(got)[at]:#x}), want {want[at]!r} ({bits(want)[at]:#x})")
