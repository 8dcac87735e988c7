"""bench.py's plain line against `--full` and its `--dump-outputs` on a small list (the shape of
tests/test_gpu_bench_strong.py): `--steps` is the number of timed steps, the dumped arrays are the records the last
step returned (the `--dump-records` array, field by field), two runs of the same command dump the same arrays, and the
CPU baseline rides on `--full` only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--workload", "c3", "--haps", "64", "--sites", "700", "--pairs", "1500", "--warmup", "1"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SHAPE, *args],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_line_dumps_the_last_steps_records(tmp_path):
    rec_path = str(tmp_path / "records.npy")
    outs = []
    for name, steps in (("a", 3), ("b", 2)):
        d = str(tmp_path / name)
        line = _bench("--steps", str(steps), "--dump-outputs", d, "--dump-records", rec_path)
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["cpu_baseline"] is None and "other_workloads" not in line["config"]
        outs.append(_load(d))
    rec = np.load(rec_path)
    a, b = outs
    assert rec.size == a["ibd_pair"].size > 0 and set(a) == {f"ibd_{f}" for f in rec.dtype.names}
    for f in rec.dtype.names:
        assert a[f"ibd_{f}"].dtype in (np.float32, np.float64)
        assert np.array_equal(b[f"ibd_{f}"].astype(rec.dtype[f]), rec[f]), f
        assert np.array_equal(a[f"ibd_{f}"], b[f"ibd_{f}"]), f


def test_full_line_carries_the_cpu_baseline():
    line = _bench("--steps", "1", "--full", "--cpu-pairs", "64")
    assert line["steps"] == 1 and line["cpu_baseline"]["unit"] == "pairs/s" and line["cpu_baseline"]["value"] > 0
