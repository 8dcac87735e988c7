"""bench.py's `--dump-outputs` writer (write_outputs) and its argument checks, without a GPU: every array is float32 or
float64, integer record fields survive exactly, an output beyond the budget becomes a fixed, seeded, ordered sample."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from fastsmc_amd import capi  # noqa: E402


def _records(n, seed=3):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, capi.IBD_DTYPE)
    rec["pair"] = np.sort(rng.integers(0, 2**32 - 1, n, dtype=np.uint64)).astype(np.uint32)
    rec["start"] = rng.integers(0, 2**31 - 1, n)
    rec["end"] = rec["start"] + rng.integers(0, 1000, n)
    for f in ("prob", "post_mean", "map"):
        rec[f] = rng.random(n, dtype=np.float32)
    return rec


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_ibd_records_are_written_field_by_field(tmp_path):
    rec = _records(1000)
    shapes = bench.write_outputs(str(tmp_path), "ibd", rec)
    got = _load(str(tmp_path))
    assert set(got) == {f"ibd_{f}" for f in rec.dtype.names} == set(shapes)
    for f in rec.dtype.names:
        a = got[f"ibd_{f}"]
        assert a.dtype in (np.float32, np.float64) and a.shape == (1000,)
        assert np.array_equal(a.astype(rec.dtype[f]), rec[f]), f  # (u32 / i32 exact in float64)
    assert got["ibd_pair"].dtype == np.float64 and got["ibd_prob"].dtype == np.float32


def test_sum_plane_is_written_as_float32(tmp_path):
    plane = np.random.default_rng(1).random((400, 69), dtype=np.float32)
    bench.write_outputs(str(tmp_path), "sums", plane)
    got = _load(str(tmp_path))
    assert list(got) == ["sum_over_pairs"] and got["sum_over_pairs"].dtype == np.float32
    assert np.array_equal(got["sum_over_pairs"], plane)


def test_output_beyond_the_budget_is_a_fixed_seeded_sample(tmp_path):
    rec = _records(50000)
    budget = 200000
    outs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        bench.write_outputs(d, "ibd", rec, budget=budget)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= budget
        outs.append(_load(d))
    a, b = outs
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["ibd_sample_index"].astype(np.int64)
    assert 0 < idx.size < rec.size and np.all(np.diff(idx) > 0)
    for f in rec.dtype.names:
        assert np.array_equal(a[f"ibd_{f}"].astype(rec.dtype[f]), rec[f][idx]), f


def test_the_default_budget_is_64_mb():
    assert bench.DUMP_BUDGET_BYTES == 64 << 20


def test_steps_below_one_are_refused():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bad], capture_output=True, text=True,
                           cwd=ROOT, timeout=120)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-500:]
