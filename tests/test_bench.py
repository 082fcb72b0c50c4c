"""bench.py's contract: a plain run prints one short result line for the headline measurement only, --dump-outputs writes
what the last timed step computed (the same files for the same arguments), --full keeps the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    for opt in ("--steps", "--warmup", "--gpus", "--full", "--dump-outputs"):
        assert opt in out.stdout
    bad = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert bad.returncode != 0 and "--steps" in bad.stderr


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """dump_outputs() on a stand-in integrator (bench.py is imported in a child: it sets OpenMP placement variables at
    import): every array float64, the sample the same from call to call, within the byte budget, and the columns of the
    state those of the sampled systems."""
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r)
import bench

class Fake:
    def __init__(self, dim, n):
        self.dim, self.batch_size = dim, n
        self.state = np.arange(dim * n, dtype=np.float64).reshape(dim, n)
        self.dtime = (np.full(n, 240.0), np.arange(n) * 1e-20)
    def propagate_res_arrays(self):
        n = self.batch_size
        return (np.full(n, -4294967299, dtype=np.int64), np.full(n, 0.5), np.full(n, 2.0), (np.arange(n) %% 7).astype(np.uint64))

small = bench.dump_sample(1000, 100)
assert np.array_equal(small, np.arange(1000))
a, b = bench.dump_sample(1 << 20, 344), bench.dump_sample(1 << 20, 344)
assert np.array_equal(a, b) and len(a) * 344 <= bench.DUMP_BYTES < (len(a) + 1) * 344
assert np.all(np.diff(a) > 0) and a[-1] < (1 << 20)
bench.dump_outputs(Fake(36, 1 << 20), sys.argv[1])
print("OK")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-3000:]
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(n + ".npy" for n in ("state", "time_hi", "time_lo", "outcome", "min_h", "max_h", "n_steps",
                                               "sample_index"))
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    idx = arrays["sample_index"].astype(np.int64)
    k = len(idx)
    assert arrays["state"].shape == (36, k) and k < (1 << 20)
    assert np.array_equal(arrays["state"][5], 5 * (1 << 20) + idx)
    assert np.all(arrays["time_hi"] == 240.0) and np.array_equal(arrays["n_steps"], idx % 7)
    assert np.all(arrays["outcome"] == -4294967299.0)


def _plain_run(tmp_path, tag):
    d = tmp_path / tag
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--systems", "8192", "--dump-outputs", str(d)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return lines[0], {f[:-4]: np.load(d / f) for f in os.listdir(d)}


@pytest.mark.gpu
def test_bench_plain_run_line_and_dumped_outputs(tmp_path):
    """The plain run the benchmark is timed with: the headline line alone (no CPU baseline, no extra legs), short enough
    for any consumer of the last line, and the outputs of its last timed step - the same, bit for bit, from two runs."""
    line, first = _plain_run(tmp_path, "a")
    assert len(line) < 8192, len(line)
    d = json.loads(line)
    assert d["metric"] == "ODE systems x steps/sec (fp64)" and d["unit"] == "system-steps/s" and d["higher_is_better"]
    assert d["dtype"] == "f64" and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "cpu_baseline" not in d and "extra_workloads" not in d
    assert d["config"]["systems_per_gpu"] == 8192 and d["config"]["all_outcomes_time_limit"]
    assert all(a.dtype == np.float64 for a in first.values())
    assert first["state"].shape == (36, 8192) and np.array_equal(first["sample_index"], np.arange(8192))
    # (Four calls of propagate_until(t + 60): every system ends at t = 240 with the time-limit outcome.)
    assert np.all(first["time_hi"] == 240.0) and np.all(np.isfinite(first["state"]))
    assert np.all(first["n_steps"] > 0)
    _, second = _plain_run(tmp_path, "b")
    assert sorted(first) == sorted(second)
    for k in first:
        assert np.array_equal(first[k], second[k]), k
