"""What a plain `bench.py` run does and writes: exactly --steps timed steps, the headline fields, nothing of
what --full adds, and (--dump-outputs DIR) the y of its last timed step, checked here against the CSR product."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, check_y

sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("parity", "matvec_kernel", "host_api", "cpu_baseline", "configs")


@pytest.mark.parametrize("steps", [1, 2, 4, 5, 7, 10, 128, 1001])
def test_batches_hold_exactly_the_steps(steps):
    sizes = bench.split_steps(steps)
    assert sum(sizes) == steps and len(sizes) == min(bench.BATCHES, steps)
    assert max(sizes) - min(sizes) <= 1


class _Rows:
    def __init__(self, n):
        self.n, self.lo, self.hi = n, 0, n


@pytest.mark.parametrize("n", [1000, 5000])
def test_dump_writes_y_or_a_fixed_sample(tmp_path, monkeypatch, n):
    """Above DUMP_WHOLE_MAX rows a seeded sample of DUMP_SAMPLE rows and their row numbers, else all of y."""
    import torch
    monkeypatch.setattr(bench, "DUMP_WHOLE_MAX", 2000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 300)
    y = torch.from_numpy(np.arange(n, dtype=np.float64) * 0.5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, None, y, _Rows(n), 1, 0)
    ya = np.load(tmp_path / "a" / "y.npy")
    assert ya.dtype == np.float64
    assert np.array_equal(ya, np.load(tmp_path / "b" / "y.npy"))
    if n <= 2000:
        assert np.array_equal(ya, y.numpy()) and not (tmp_path / "a" / "y_rows.npy").exists()
    else:
        rows = np.load(tmp_path / "a" / "y_rows.npy")
        assert rows.dtype == np.float64 and rows.size == 300 == np.unique(rows).size
        assert np.array_equal(ya, 0.5 * rows)
        assert np.array_equal(rows, np.load(tmp_path / "b" / "y_rows.npy"))


def _bench(args, tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("symmetric", [False, True], ids=["general", "symmetric"])
def test_plain_run_times_its_steps_and_dumps_y(tmp_path, symmetric):
    from sparsex_amd import synth
    out = _bench(["--steps", "7", "--warmup", "2", "--workload", "syn-cant", "--scale", "0.3", "--host-threads", "2",
                  "--dump-outputs", "dump"] + (["--symmetric"] if symmetric else []), tmp_path)
    assert all(k in out for k in HEADLINE) and not any(k in out for k in FULL_ONLY)
    assert out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 7 and out["protocol"]["timed_steps"] == 7 and sum(out["protocol"]["steps_per_batch"]) == 7
    assert len(out["protocol"]["batch_ms"]) == 5 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(2e-6 * out["config"]["nnz"] / out["ms_per_step"], rel=1e-3)
    csr = synth.syn_cant(0.3)
    y = np.load(tmp_path / "dump" / "y.npy")
    assert y.dtype == np.float64 and y.size == csr[3]
    check_y(csr, synth.random_x(csr[3]), y, bench.ALPHA)


@pytest.mark.gpu
def test_full_run_adds_the_rest(tmp_path):
    out = _bench(["--steps", "10", "--warmup", "2", "--workload", "syn-cant", "--scale", "0.3", "--host-threads", "2",
                  "--full", "--no-cpu-baseline"], tmp_path)
    assert all(k in out for k in HEADLINE) and out["protocol"]["timed_steps"] == 10
    assert out["parity"]["max_err_over_fp64_bound"] <= 1.0
    assert out["matvec_kernel"]["ms_per_step"] > 0 and "view_per_call" in out["host_api"]
    assert out["roofline"]["measured_mixed_peak"] > 0
    assert set(out["protocol"]["launch_modes"]) == {"hipGraph_ms_per_step", "stream_launches_ms_per_step"}
