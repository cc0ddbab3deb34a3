"""bench.py's contract: a plain run times exactly --steps steps and nothing else; --dump-outputs writes what the last timed
step computed; --full keeps the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_options_listed():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    steps, warmup, n, rows, pairs = 10, 2, 4096, 4096, 6
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == steps and out["blocks"] == 1 and out["value"] > 50 and out["ms_per_step"] > 0
    for k in ("other_configs", "strong_cfg5", "host_api", "cpu_baseline"):
        assert k not in out, k
    assert out["no_ramp"] is None and "warm" not in out["roofline"]
    assert sorted(os.listdir(tmp_path)) == ["ndfft_out.npy"]
    y = np.load(tmp_path / "ndfft_out.npy")
    assert y.dtype == np.float64 and y.nbytes <= 64 << 20 and y.shape == (256, n, 2)
    # the timed steps start at pair 0 after max(W, 2 x pairs) warm-up steps: the last one transformed pair (12 + K - 1) mod 6
    p = (max(warmup, 2 * pairs) + steps - 1) % pairs
    sel = np.sort(np.random.default_rng(20241008).choice(rows, y.shape[0], replace=False))
    for i in (0, len(sel) // 2, len(sel) - 1):
        ref = np.fft.fft(synth.complex_array((1, n), offset=(p * rows + int(sel[i])) * n), axis=1)[0]
        got = y[i, :, 0] + 1j * y[i, :, 1]
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-10, i
