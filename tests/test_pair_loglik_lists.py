"""What tests/pair_loglik_lists.py claims, shown on the CPU: its float32 restatement of the forward sweep is the
oracle's, bit for bit, on every input of tests/test_gpu_pair_loglik.py; its log-likelihoods are those of an fp64 dense
forward to within fp32 rounding; and the inputs reach the regimes the GPU tests are there for."""
import numpy as np
import pytest

import edge_models as E
import pair_loglik_lists as LL
from pair_common import EDGES_700

# The largest |log-likelihood of the restatement - fp64 dense forward| over every fourth pair of every case, measured
# on the CPU: 1.38e-6 (the 50-state case; values of -0.2 ... -230).  The error is fp32 rounding of the sums, which
# grows with the sites; nothing derives a tighter bound, so four times the measured value is allowed.
MEASURED_DENSE_DIFFERENCE = 1.38e-6
DENSE_BOUND = 4 * MEASURED_DENSE_DIFFERENCE


@pytest.mark.parametrize("name", list(LL.CASES))
def test_restatement_is_the_oracles_forward_sweep(name):
    pm, _, folded, pairs, sums, _ = LL.case(name)
    again, alpha = LL.forward(pm, folded, pairs)
    assert np.array_equal(again, sums)
    assert sums.dtype == np.float32 and sums.shape == (len(pairs), pm.S)
    assert np.array_equal(alpha, LL.oracle_alpha_fwd(pm, folded, pairs))
    # the scaled vector of the last site sums to 1 give or take rounding: `sums` are the sums BEFORE the scaling
    assert np.allclose(alpha[pm.S - 1].sum(axis=0), 1.0, atol=1e-5)
    assert (sums > 0).all() and np.isfinite(sums).all()


@pytest.mark.parametrize("case", E.SWEEP_CASES + E.SWEEP_SEQ_CASES, ids=E.sweep_id)
def test_restatement_is_the_oracles_forward_sweep_at_the_edges(case):
    """The edge models of tests/test_gpu_pair_loglik.py (subnormal table entries and vectors, states at exactly +0, every
    state equal, identical and complementary haplotypes; array and sequence mode): the oracle's alphaFwd bit for bit,
    subnormals and zeros included, and no zero sum, so that every pair has a likelihood to compare."""
    name, K, seq = case
    pm, _, folded, pairs, sums = LL.edge_case(name, K, seq)
    again, alpha = LL.forward(pm, folded, pairs)
    assert np.array_equal(again, sums)
    assert np.array_equal(alpha, LL.oracle_alpha_fwd(pm, folded, pairs))
    assert (sums > 0).all() and np.isfinite(sums).all()
    tiny = np.finfo(np.float32).tiny
    print(f"{E.sweep_id(case)}: {int(((alpha > 0) & (alpha < tiny)).sum())} subnormal and {int((alpha == 0).sum())} zero "
          f"entries of alpha, smallest sum {sums.min():.3e}")
    if name == "subnormal-1e-38":  # the forward vectors themselves carry subnormals, not only the tables
        assert ((alpha > 0) & (alpha < tiny)).sum() > 100


def test_restatement_on_the_cohort():
    pm, _, folded, _ = LL.cohort_problem()
    pairs = LL.cohort_pairs()[0]
    sums = LL.cohort_sums()
    _, alpha = LL.forward(pm, folded, pairs[:64])
    assert np.array_equal(alpha, LL.oracle_alpha_fwd(pm, folded, pairs[:64]))
    assert sums.shape == (200, 700) and (sums > 0).all()


@pytest.mark.parametrize("name", list(LL.CASES))
def test_log_likelihoods_agree_with_the_dense_forward(name):
    pm, _, folded, pairs, sums, _ = LL.case(name)
    mant, expo, _, _ = LL.expected(sums)
    assert ((mant >= 0.5) & (mant < 1)).all()
    ll = LL.log_likelihood(mant, expo)
    worst = 0.0
    for i in range(0, len(pairs), 4):
        worst = max(worst, abs(ll[i] - LL.dense_log_likelihood(pm, folded, pairs[i])))
    print(f"{name}: largest difference to the dense forward {worst:.3e}")
    assert worst <= DENSE_BOUND, (name, worst)


def test_chain_is_the_product_of_the_sums():
    """mant * 2^expo is the product of the sums (in fp64, to rounding), and the bins of contiguous edges multiply up to
    the chain over their union -- to rounding only: the total is a chain of its own."""
    _, _, _, _, sums, edge_sets = LL.case("S200")
    mant, expo, bm, be = LL.expected(sums, edge_sets["E_200"])
    direct = np.log(sums.astype(np.float64)).sum(axis=1)
    assert np.allclose(LL.log_likelihood(mant, expo), direct, rtol=0, atol=1e-10)
    m, e = LL.chain(sums, 3, 199)
    assert np.allclose(LL.log_likelihood(bm, be).sum(axis=1), LL.log_likelihood(m, e), rtol=0, atol=1e-10)
    # one bin over everything IS the total, bit for bit
    mant1, expo1, bm1, be1 = LL.expected(sums, edge_sets["whole"])
    assert np.array_equal(bm1[:, 0], mant1) and np.array_equal(be1[:, 0], expo1)


def test_inputs_reach_their_regimes():
    edge_sets = {}
    for name, (K, S, n, seq, sets) in LL.CASES.items():
        for ename, e in sets.items():
            assert e[0] >= 0 and e[-1] <= S and (np.diff(e) > 0).all(), (name, ename)
            edge_sets[ename] = (S, e)
        assert n % 64 != 0, "a ragged last group"
    edge_sets["EDGES_700"] = (700, np.array(EDGES_700))
    every = [e for _, e in edge_sets.values()]
    assert any(((e[1:-1] % 64) == 0).any() for e in every), "an inner bin edge on a multiple of 64"
    assert any(((e % 64) != 0).any() for e in every), "a bin edge off the multiples of 64"
    assert any((np.diff(e) == 1).any() for e in every), "a one-site bin"
    assert any(e[0] > 0 and e[-1] < S for S, e in edge_sets.values()), "sites before the first edge and after the last"
    S, e = edge_sets["every_site"]
    assert S == 65 and np.array_equal(e, np.arange(66))
    assert {K for K, *_ in LL.CASES.values()} >= {2, 3, 16, 20, 64, 128, 50, 69, 100}
    assert {S for _, S, *_ in LL.CASES.values()} >= {1, 2, 63, 64, 65, 129, 200}
    assert max(LL.PAIR_COUNTS) <= LL.CASES["S65"][2] and set(LL.PAIR_COUNTS) == {1, 63, 64, 65, 200}
    assert [(K, S) for K, S, _, seq, _ in LL.CASES.values() if seq] == [(40, 150), (69, 150)]
    # the pairs differ: no two rows of sums of a case are equal, so a lane that took another lane's pair shows
    _, _, _, _, sums, _ = LL.case("S65")
    assert len({r.tobytes() for r in sums}) > 150


def test_zero_sum_problem_reaches_zero_and_nan():
    pm, _, folded, pairs, sums, mid = LL.zero_sum_problem()
    mant, expo, bm, be = LL.expected(sums, np.array([0, mid + 1, 200], np.int32))
    zero, nan = mant == 0, np.isnan(mant)
    assert zero.sum() >= 2 and nan.sum() >= 2 and (~zero & ~nan).sum() >= 2
    assert np.array_equal(sums[:, mid] == 0, nan)            # a zero sum in the middle: NaN from the next site on
    assert np.array_equal((sums[:, 199] == 0) & ~nan, zero)  # a zero sum at the last site: likelihood zero
    ll = LL.log_likelihood(mant, expo)
    assert (ll[zero] == -np.inf).all() and np.isnan(ll[nan]).all() and np.isfinite(ll[~zero & ~nan]).all()
    # the bin that ends at the zero site has likelihood zero, the bin after it is NaN
    assert (bm[nan, 0] == 0).all() and np.isnan(bm[nan, 1]).all()
