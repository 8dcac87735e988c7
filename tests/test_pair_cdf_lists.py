"""What the inputs of the fsmc_decode_pair_cdf tests reach, proved on the CPU oracle (no GPU): the order of the sum, the
`>=` rule and the K-1 fallback all show in the expected values of tests/pair_cdf_lists.py, so an implementation that
sums in another order, compares with `>`, or forgets the fallback cannot pass the GPU tests.  The bounds asserted are
conditions on the inputs, kept well below what was measured over the list's 192 x 640 = 122 880 pair-sites (figures in
the comments)."""
import numpy as np
import pytest

import pair_cdf_lists as CL

N_CELLS = 192 * 640


@pytest.fixture(scope="module")
def post(small_problem):
    """[S][K][192] float32: the oracle's posteriors of PAIRS_192, the batches side by side."""
    return np.concatenate([p[:, :, :n] for p, n in CL.posteriors_192(small_problem)], axis=2)


@pytest.fixture(scope="module")
def std(small_problem):
    return CL.expected_192(small_problem)


def _rows(x):
    """[S][192] -> [192][S], the layout of the expected values."""
    return np.ascontiguousarray(x.T)


def _tree_sum(x):
    """Sum over axis 1 by a pairwise tree: neighbours added, level by level, an odd level padded with +0.0."""
    x = np.asarray(x, np.float32)
    while x.shape[1] > 1:
        if x.shape[1] % 2:
            x = np.concatenate([x, np.zeros_like(x[:, :1])], axis=1)
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _descending_sum(x):
    acc = np.zeros((x.shape[0], x.shape[2]), np.float32)
    for k in range(x.shape[1] - 1, -1, -1):
        acc = acc + x[:, k, :]
    return acc


def test_shapes_and_cuts(small_problem, std):
    pm = small_problem["model"]
    cut_list = CL.cuts(pm)
    assert cut_list[0] == 1 and cut_list[-1] == pm.K == 69 and 1 <= cut_list[1] <= 69
    tail, qstate = std
    assert tail.shape == qstate.shape == (4, 192, 640)
    assert tail.dtype == np.float32 and qstate.dtype == np.int32
    assert qstate.min() >= 0 and qstate.max() <= 68


def test_the_order_of_the_sum_shows(small_problem, post, std):
    tail = std[0]
    cut_list = CL.cuts(small_problem["model"])
    t25, t69 = tail[cut_list.index(25)], tail[cut_list.index(69)]
    differs = int((_rows(_tree_sum(post[:, :25, :])) != t25).sum())
    print(f"ascending vs pairwise tree, c = 25: {differs} of {N_CELLS} cells differ")  # measured: tens of thousands
    assert differs >= 10000
    differs = int((_rows(_tree_sum(post)) != t69).sum())
    print(f"ascending vs pairwise tree, c = 69: {differs} cells differ")
    assert differs >= 10000
    differs = int((_rows(_descending_sum(post)) != t69).sum())
    print(f"ascending vs descending, c = 69: {differs} cells differ")
    assert differs >= 10000


def test_quantile_one_reaches_the_fallback_and_the_compare(small_problem, post, std):
    """q = 1.0: at many cells no state reaches it (cdf[K-1] < 1 after rounding), a float64 running sum rounded to
    fp32 finds another state, and `>` in place of `>=` finds another state."""
    K = 69
    q1 = std[1][CL.QS.index(1.0)]
    cdf = np.zeros_like(post)
    acc = np.zeros((post.shape[0], post.shape[2]), np.float32)
    for k in range(K):
        acc = acc + post[:, k, :]
        cdf[:, k, :] = acc
    one = np.float32(1.0)
    never = _rows((cdf >= one).sum(axis=1) == 0)
    print(f"q = 1.0: no state reaches it at {int(never.sum())} cells")  # measured: 49 874
    assert int(never.sum()) >= 1000
    assert (q1[never] == K - 1).all()

    def first(mask):  # [S][K][n] bool -> [n][S] int32, K-1 where none
        return _rows(np.where(mask.any(axis=1), mask.argmax(axis=1), K - 1).astype(np.int32))

    assert np.array_equal(first(cdf >= one), q1)  # (the definition, stated a second way)
    cdf64 = np.cumsum(post.astype(np.float64), axis=1).astype(np.float32)
    differs = int((first(cdf64 >= one) != q1).sum())
    print(f"q = 1.0: a float64 running sum rounded to fp32 gives another state at {differs} cells")  # measured: 81
    assert differs >= 10
    differs = int((first(cdf > one) != q1).sum())
    print(f"q = 1.0: `>` gives another state at {differs} cells")  # measured: 47
    assert differs >= 10


def test_the_median_is_not_the_map(small_problem, std):
    med = std[1][CL.QS.index(0.5)]
    distinct = np.unique(med).size
    print(f"q = 0.5: {distinct} distinct median states")  # measured: 64
    assert distinct >= 32
    _, mp = CL.rows_192(small_problem)
    share = float((med != mp).mean())
    print(f"q = 0.5: the median state differs from the MAP state at {100 * share:.1f} % of the cells")  # measured: 96.9 %
    assert share >= 0.5


def test_the_last_state_is_reached_properly(post, std):
    """q = 0.975: K-1 as a state whose cdf reaches q, not as the fallback."""
    q975 = std[1][CL.QS.index(0.975)]
    acc = np.zeros((post.shape[0], post.shape[2]), np.float32)
    for k in range(69):
        acc = acc + post[:, k, :]
    proper = (q975 == 68) & _rows(acc >= np.float32(0.975))
    print(f"q = 0.975: state K-1 reached properly at {int(proper.sum())} cells")  # measured: 31 850
    assert int(proper.sum()) >= 1000


def test_invariants(small_problem, std):
    tail, qstate = std
    cut_list = CL.cuts(small_problem["model"])
    order = np.argsort(cut_list, kind="stable")
    for a, b in zip(order[:-1], order[1:]):
        assert (tail[a] <= tail[b]).all(), (cut_list[a], cut_list[b])  # non-decreasing in c
    for j in range(len(CL.QS) - 1):
        assert CL.QS[j] < CL.QS[j + 1] and (qstate[j] <= qstate[j + 1]).all()  # non-decreasing in q
    full = tail[cut_list.index(69)]
    assert (full >= 1 - 1e-5).all() and (full <= 1 + 1e-5).all()
    share = float((full != np.float32(1.0)).mean())
    print(f"tail[c = K] is not exactly 1 at {100 * share:.1f} % of the cells")  # measured: 72.6 %
    assert share > 0.5
