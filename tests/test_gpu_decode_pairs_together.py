"""ASMC.decodePairs with every output asked for in ONE call: each field equals, bit for bit, the field of a call that asks
for one family of outputs alone (the rows, the posteriors, the minima, the site bins, the tail probabilities and quantile
states, the tail summaries) -- which tests/test_gpu_pair_*.py tie to the oracle.  A flush serves its consumers one after
the other from the same work list at the same "pairs written so far"; this pins that none of them disturbs another, with
one flush and with two (FSMC_DIAG_FLUSH_PAIRS=128: 128 and 72 pairs), and that nothing of a call's request is left behind
for the next call."""
import numpy as np
import pytest

from fastsmc_amd import api
from pair_common import EDGES_700, N_PAIRS, SITES, cohort_files, cohort_pairs, params

pytestmark = pytest.mark.gpu

FIELDS = ("per_pair_posteriors", "sum_of_posteriors", "per_pair_posterior_means", "min_posterior_means",
          "argmin_posterior_means", "per_pair_MAPs", "min_MAPs", "argmin_MAPs", "bin_edges", "bin_mean_posterior_means",
          "bin_min_posterior_means", "bin_argmin_posterior_means", "bin_min_MAPs", "bin_argmin_MAPs", "tail_times",
          "tail_states", "quantiles", "per_pair_tail_probabilities", "per_pair_quantile_states", "tail_summary_times",
          "tail_summary_states", "site_weights", "sum_of_tail_probabilities", "per_pair_bin_tail_means",
          "per_pair_bin_tail_lengths")
MINIMA = ("min_posterior_means", "argmin_posterior_means", "min_MAPs", "argmin_MAPs")


def _fields(res):
    return {name: np.array(getattr(res, name)) for name in FIELDS}


@pytest.mark.parametrize("flush_pairs", [None, 128])
def test_all_outputs_in_one_call_are_those_of_a_call_each(tmp_path, monkeypatch, flush_pairs):
    if flush_pairs:
        monkeypatch.setenv("FSMC_DIAG_FLUSH_PAIRS", str(flush_pairs))
    p = params(cohort_files(tmp_path)[0])
    asmc = api.ASMC(p)
    _, a, b = cohort_pairs()
    w = api.site_widths(np.array(api.Data(p).geneticPositions, np.float32))
    times = [50, 200]
    # one family of outputs a call: its keywords and the fields it fills
    families = (
        ("rows", dict(per_pair_posterior_means=True, per_pair_MAPs=True),
         ("per_pair_posterior_means", "per_pair_MAPs") + MINIMA),
        ("posteriors", dict(per_pair_posteriors=True, sum_of_posteriors=True),
         ("per_pair_posteriors", "sum_of_posteriors")),
        ("minima", dict(min_posterior_means=True, min_MAPs=True), MINIMA),
        ("bins", dict(site_bins=EDGES_700),
         ("bin_edges", "bin_mean_posterior_means", "bin_min_posterior_means", "bin_argmin_posterior_means",
          "bin_min_MAPs", "bin_argmin_MAPs")),
        ("cdf", dict(tail_times=times, quantiles=[0.5]),
         ("tail_times", "tail_states", "quantiles", "per_pair_tail_probabilities", "per_pair_quantile_states")),
        ("tail summaries", dict(tail_summary_times=times, site_bins=EDGES_700, site_weights=w),
         ("tail_summary_times", "tail_summary_states", "site_weights", "sum_of_tail_probabilities",
          "per_pair_bin_tail_means", "per_pair_bin_tail_lengths", "bin_edges")),
    )
    alone, indices = {}, None
    for family, kwargs, names in families:
        asmc.decodePairs(a, b, **kwargs)
        res = asmc.get_copy_of_results()
        alone[family] = _fields(res)
        indices = res.per_pair_indices if indices is None else indices
        assert res.per_pair_indices == indices, family
        assert all(alone[family][name].size > 0 for name in names), family

    everything = {}
    for _, kwargs, _ in families:
        everything.update(kwargs)
    assert sorted(everything) == sorted(
        ("per_pair_posteriors", "sum_of_posteriors", "per_pair_posterior_means", "per_pair_MAPs", "min_posterior_means",
         "min_MAPs", "site_bins", "tail_times", "quantiles", "tail_summary_times", "site_weights"))
    asmc.decodePairs(a, b, **everything)
    res = asmc.get_copy_of_results()
    together = _fields(res)
    assert res.per_pair_indices == indices and len(indices) == N_PAIRS
    assert together["per_pair_posteriors"].shape == (N_PAIRS, 69, SITES)
    seen = set()
    for family, _, names in families:
        for name in names:
            g, want = together[name], alone[family][name]
            assert g.dtype == want.dtype and g.shape == want.shape, (family, name, g.dtype, want.dtype, g.shape, want.shape)
            assert np.array_equal(g, want), f"{name} differs from the call for the {family} alone"
            seen.add(name)
    assert seen == set(FIELDS)

    # straight after: the minima alone, and every other field empty -- nothing of the last request is left
    asmc.decodePairs(a, b, min_posterior_means=True)
    res = asmc.get_copy_of_results()
    after = _fields(res)
    assert res.per_pair_indices == indices
    for name in ("min_posterior_means", "argmin_posterior_means"):
        assert np.array_equal(after[name], alone["minima"][name]), name
    for name in FIELDS:
        if name not in ("min_posterior_means", "argmin_posterior_means"):
            assert after[name].size == 0, name
