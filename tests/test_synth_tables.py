"""synth.make_model_tables at the one genetic distance its closed forms cannot take, r = 1/(2N) (a = 1/N - 2r = 0):
an error, not NaN tables; and the tables of the suite's and the benchmark's population size (N = 15000) unchanged."""
import hashlib

import numpy as np
import pytest

from fastsmc_amd import synth

FIELDS = ("discretization", "expected_times", "initial_state_prob", "column_ratios", "keys", "D", "B", "U", "RR",
          "classic_emission", "compressed_emission", "folded_ascertained_csfs", "ascertained_csfs", "csfs",
          "folded_csfs", "homozygous_keys", "homozygous")

# sha256 of the FIELDS' bytes, in order, as the generator produced them before r = 1/(2N) was refused
N15000 = {
    69: "52f6254fd39840c3da210185615b08a569575f3df83c43bd7455434ebe1f0833",
    256: "ac7344706a1d2e1d598711063a48ef4009bbc74ae6f3d75ebe84cdb256cb92ab",
    600: "be9c2b80d2d787d388122552c55622eecb6d8219cc65addbec55150e38a61ec4",
}


def _digest(t):
    h = hashlib.sha256()
    for f in FIELDS:
        h.update(np.ascontiguousarray(getattr(t, f)).tobytes())
    return h.hexdigest()


def test_key_equal_to_one_over_two_n_is_refused():
    keys = synth.genetic_distance_keys()
    assert np.any(keys == 1.0 / (2.0 * 1e5))  # 5e-6 is on the grid
    with pytest.raises(ValueError, match="1/\\(2N\\)"):
        synth.make_model_tables(16, N=1e5)


@pytest.mark.parametrize("K", sorted(N15000))
def test_tables_of_the_suite_and_bench_population_are_unchanged(K):
    assert not np.any(synth.genetic_distance_keys() == 1.0 / (2.0 * 15000.0))
    t = synth.make_model_tables(K)
    for f in FIELDS:
        if f != "discretization":  # (its last boundary is +inf)
            assert np.all(np.isfinite(getattr(t, f))), f
    assert _digest(t) == N15000[K]
