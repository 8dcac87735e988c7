"""fsmc_decode_pair_loglik on the GPU: per pair, the likelihood of its observations from the forward sweep alone, as
mantissa and exponent, over the whole sequence and over bins of sites.  Mantissas and exponents are np.array_equal to
the numpy restatement of tests/pair_loglik_lists.py (tests/test_pair_loglik_lists.py shows on the CPU that the
restatement is the oracle's forward sweep and what the inputs reach).  The edge models (edge_models.SWEEP_CASES) are the
numeric edges the decode kernels are tested at."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
from conftest import expected_member
from fastsmc_amd import api, capi
from pair_common import (EDGES_700, pairs_array as _pairs_array, upload as _upload, cohort_files as _cohort_files,
                         params as _params, cohort_pairs as _cohort_pairs)

pytestmark = pytest.mark.gpu

INT_MIN = np.iinfo(np.int32).min
NAMES = ("mant", "expo", "bin_mant", "bin_expo")


def _open(pm, bits):
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    return ctx, model


def _assert_equal(got, want, msg="", equal_nan=False):
    assert len(got) == len(want) == 4
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (name, msg)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, msg, g.dtype, w.dtype, g.shape, w.shape)
        same = np.array_equal(g, w, equal_nan=equal_nan and g.dtype == np.float64)
        assert same, f"{name} {msg}: {int((g != w).sum())} of {g.size} values differ"


def _sentinels(n, B):
    """(mant, expo, bin_mant, bin_expo) prefilled with values no result has: NaN and INT_MIN."""
    return (np.full(n, np.nan), np.full(n, INT_MIN, np.int32), np.full((n, B), np.nan), np.full((n, B), INT_MIN, np.int32))


def _untouched(a):
    return bool(np.isnan(a).all()) if a.dtype == np.float64 else bool((a == INT_MIN).all())


@pytest.mark.parametrize("name", list(LL.CASES))
def test_models_sites_and_bins(name):
    """Every case of pair_loglik_lists: the members of the family (K = 2 ... 128, exact and padded), 1 ... 200 sites,
    sequence mode; the totals alone, then with each of the case's edge sets, then the bins alone."""
    pm, bits, _, pairs, sums, edge_sets = LL.case(name)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_loglik(model)
    assert ctx.last_kernel() == expected_member(pm.K)
    assert ctx.last_kernel_ms() > 0
    assert ctx.last_pair_loglik_slices() == 1
    _assert_equal(got, LL.expected(sums), name)
    for ename, edges in edge_sets.items():
        want = LL.expected(sums, edges)
        _assert_equal(ctx.decode_pair_loglik(model, edges), want, f"{name} {ename}")
        _assert_equal(ctx.decode_pair_loglik(model, edges, want_total=False), (None, None) + want[2:],
                      f"{name} {ename}, bins alone")
    ctx.close()


@pytest.mark.parametrize("case", E.SWEEP_CASES + E.SWEEP_SEQ_CASES, ids=E.sweep_id)
def test_numeric_edges(case):
    """The edge models of the decode kernels (subnormal table entries and vectors, states at exactly +0 beside the ghost
    states, every state equal, identical and complementary haplotypes) at an exact and two padded members, and the two
    sequence-mode ones at 69 states: all 96 pairs, two groups, bit for bit -- tests/test_pair_viterbi_lists.py shows that
    every pair has a finite, non-zero likelihood."""
    name, K, seq = case
    pm, bits, _, pairs, sums = LL.edge_case(name, K, seq)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_loglik(model)
    assert ctx.last_kernel() == expected_member(K)
    ctx.close()
    _assert_equal(got, LL.expected(sums), E.sweep_id(case))


@pytest.fixture
def s65():
    pm, bits, _, pairs, sums, edge_sets = LL.case("S65")
    ctx, model = _open(pm, bits)
    yield ctx, model, pm, pairs, sums, edge_sets["every_site"]
    ctx.close()


def test_pair_counts(s65):
    """1, 63, 64, 65 and 200 pairs: a lone lane, a group one short, a full group, one lane in a second group, four
    groups; rows beyond the list stay untouched."""
    ctx, model, pm, pairs, sums, edges = s65
    want = LL.expected(sums, edges)
    for n in LL.PAIR_COUNTS:
        _upload(ctx, pm, pairs[:n])
        bufs = _sentinels(n + 3, len(edges) - 1)
        got = ctx.decode_pair_loglik(model, edges, out=bufs)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g[:n], w[:n]), (n, name)
            assert _untouched(g[n:]), (n, name)


def test_more_groups_than_waves(s65):
    """A list of more groups than the launch has waves, built from repeats of the 200 distinct pairs: every wave pulls
    several groups from the queue."""
    ctx, model, pm, pairs, sums, _ = s65
    n_groups = ctx.info()["n_cu"] * 8 + 37
    idx = (np.arange(n_groups * 64 - 5) * 7) % len(pairs)  # (7 and 200 are coprime: every lane sees every pair)
    _upload(ctx, pm, [pairs[i] for i in idx])
    edges = np.array([0, 64, 65], np.int32)
    got = ctx.decode_pair_loglik(model, edges)
    assert ctx.last_pair_loglik_slices() == 1
    assert 0 < ctx.info()["n_slots"] < n_groups
    want = LL.expected(sums, edges)
    _assert_equal(got, tuple(w[idx] for w in want), f"{n_groups} groups")


def test_slices_do_not_show(s65):
    ctx, model, pm, pairs, sums, edges = s65
    want = LL.expected(sums, edges)
    _upload(ctx, pm, pairs)  # four groups, the last of 8 pairs
    for slice_groups, n_slices in ((1, 4), (2, 2), (0, 1)):
        ctx.set_pair_loglik_slice(slice_groups)
        got = ctx.decode_pair_loglik(model, edges)
        assert ctx.last_pair_loglik_slices() == n_slices
        _assert_equal(got, want, f"slice {slice_groups}")


def test_cohort_edges_700():
    pm, bits, _, _ = LL.cohort_problem()
    pairs = _cohort_pairs()[0]
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_loglik(model, EDGES_700)
    assert ctx.last_kernel() == 69
    _assert_equal(got, LL.expected(LL.cohort_sums(), EDGES_700), "EDGES_700")
    ctx.close()


def test_zero_and_nan_sums():
    """Sums that reach zero: at the last site the likelihood is zero (mantissa +0.0, logarithm -inf); in the middle
    every later sum is NaN and the NaN stays.  NaNs compare equal here whatever their payload; everything else by bits."""
    pm, bits, _, pairs, sums, mid = LL.zero_sum_problem()
    edges = np.array([0, mid + 1, 200], np.int32)
    want = LL.expected(sums, edges)
    ctx, model = _open(pm, bits)
    _upload(ctx, pm, pairs)
    got = ctx.decode_pair_loglik(model, edges)
    ctx.close()
    _assert_equal(got, want, "zero sums", equal_nan=True)
    zero = want[0] == 0
    assert zero.any() and not np.signbit(got[0][zero]).any()
    ll = capi.log_likelihood(got[0], got[1])
    assert (ll[zero] == -np.inf).all() and np.array_equal(np.isnan(ll), np.isnan(want[0]))


def test_errors(s65):
    """Every FSMC_EINVAL, nothing touched, each followed by a good call."""
    ctx, model, pm, pairs, sums, edges = s65
    B = len(edges) - 1
    want = LL.expected(sums, edges)
    _upload(ctx, pm, pairs)

    def good():
        _assert_equal(ctx.decode_pair_loglik(model, edges), want, "after an error")

    def refused(text, keep=(0, 1, 2, 3), e=edges, n_bins=None, mdl=None):
        bufs = _sentinels(len(pairs), B if n_bins is None else n_bins)
        out = tuple(b if i in keep else None for i, b in enumerate(bufs))
        with pytest.raises(capi.FsmcError) as ei:
            ctx.decode_pair_loglik(mdl or model, e, out=out)
        assert ei.value.code == -1 and text in str(ei.value), (text, str(ei.value))  # FSMC_EINVAL
        assert all(_untouched(b) for b in bufs)
        good()

    good()
    for keep in ((0,), (1,), (0, 2, 3), (1, 2, 3), (2,), (3,), (0, 1, 2), (0, 1, 3)):  # a half of a pair of outputs
        refused("come together", keep=keep)
    refused("at least one pair of outputs", keep=())
    refused("need bin edges", e=None, n_bins=0)
    refused("one bin at least", e=[7], n_bins=0)
    refused("strictly ascending", e=[5, 30, 30, 64], n_bins=3)
    refused("strictly ascending", e=[5, 30, 20, 64], n_bins=3)
    refused("[0, sites]", e=[-1, 30, 64], n_bins=2)
    refused("[0, sites]", e=[5, 30, 66], n_bins=2)
    assert ctx.last_pair_loglik_slices() == 1  # (of the good call)
    groups = capi.whole_sequence_groups(len(pairs), pm.S)
    groups["from"][1] = 10
    groups["scan_from"][1] = 10
    ctx.upload_worklist(_pairs_array(pairs), groups)
    with pytest.raises(capi.FsmcError) as ei:
        ctx.decode_pair_loglik(model, edges)
    assert ei.value.code == -1 and "whole-sequence" in str(ei.value)
    _upload(ctx, pm, pairs)
    good()
    # a model of more than 128 states on the same haplotypes: the wave-group family has no forward kernel
    wide, wide_bits, _ = LL._problem(130, 65, seed=100 + 69 + 65)
    assert np.array_equal(wide_bits, LL.case("S65")[1])
    refused("more than 128 states", mdl=ctx.create_model(wide))


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

FIELDS = ("per_pair_likelihood_mantissas", "per_pair_likelihood_exponents", "per_pair_bin_likelihood_mantissas",
          "per_pair_bin_likelihood_exponents")


def _within_4_ulp(got, mant, expo):
    want = np.log(mant) + expo * np.log(2)
    return bool((np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all())


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_product_path(tmp_path, monkeypatch, flush_pairs):
    """ASMC.decodePairs(a, b, log_likelihoods=True[, site_bins=EDGES_700]) on a synthetic cohort's files: mantissas and
    exponents are the restatement's, the logarithms log(m) + e ln 2 to 4 ulp (two implementations of log and one add).
    With FSMC_DIAG_FLUSH_PAIRS=128 two flushes fill the fields at the pairs written so far.  Alongside
    per_pair_posterior_means the means are what they are without the request; a second call gives the first one's
    results; without the keyword every new field is empty."""
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    root, _, _, _, _ = _cohort_files(tmp_path)
    p = _params(root)
    asmc = api.ASMC(p)
    pairs, a, b = _cohort_pairs()
    pm = LL.cohort_problem()[0]
    assert np.array_equal(np.array(api.Data(p).geneticPositions, np.float32), pm.gen)  # (the restatement's model)
    want = LL.expected(LL.cohort_sums(), EDGES_700)

    def four(res):
        return tuple(np.array(getattr(res, f)) for f in FIELDS)

    asmc.decodePairs(a, b, log_likelihoods=True)
    res = asmc.get_copy_of_results()
    m, e, bm, be = four(res)
    assert m.dtype == np.float64 and e.dtype == np.int32
    assert np.array_equal(m, want[0]) and np.array_equal(e, want[1])
    assert bm.size == 0 and be.size == 0 and np.array(res.per_pair_bin_log_likelihoods).size == 0
    ll = np.array(res.per_pair_log_likelihoods)
    assert ll.dtype == np.float64 and ll.shape == (len(pairs),) and _within_4_ulp(ll, m, e)
    assert np.array(res.per_pair_posterior_means).size == 0

    for _ in range(2):  # two calls in a row
        asmc.decodePairs(a, b, log_likelihoods=True, site_bins=EDGES_700)
        res = asmc.get_copy_of_results()
        got = four(res)
        for name, g, w in zip(FIELDS, got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
        assert _within_4_ulp(np.array(res.per_pair_log_likelihoods), got[0], got[1])
        bll = np.array(res.per_pair_bin_log_likelihoods)
        assert bll.shape == (len(pairs), len(EDGES_700) - 1) and _within_4_ulp(bll, got[2], got[3])

    asmc.decodePairs(a, b, per_pair_posterior_means=True)
    res = asmc.get_copy_of_results()
    means = np.array(res.per_pair_posterior_means)
    assert means.shape == (len(pairs), pm.S)
    assert all(g.size == 0 for g in four(res)) and np.array(res.per_pair_log_likelihoods).size == 0
    asmc.decodePairs(a, b, per_pair_posterior_means=True, log_likelihoods=True)
    res = asmc.get_copy_of_results()
    assert np.array_equal(np.array(res.per_pair_posterior_means), means)
    assert np.array_equal(four(res)[0], want[0]) and np.array_equal(four(res)[1], want[1])
