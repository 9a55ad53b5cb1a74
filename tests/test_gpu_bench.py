"""bench.py's plain run (-m gpu): `--steps` is the number of timed steps, the line carries the headline and nothing that `--full` adds,
and `--dump-outputs` writes what the last timed step returned - the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, out_dir):
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, "bench.py"] + args + ["--dump-outputs", str(out_dir)], capture_output=True, text=True,
                         timeout=600, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "x.npy"))


def _bits(a):
    return a.view(np.int32)


def test_plain_run_times_exactly_steps_and_dumps_the_last_output(tmp_path):
    d, a = _bench(["--steps", "3", "--warmup", "2"], tmp_path / "a")
    assert d["metric"] == "denoising steps/sec (8-bar prmat2c, batch 16)" and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16x3" and d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["windows"] == 1 and len(d["windows_ms_per_step"]) == 1 and d["windows_ms_per_step"][0] == d["ms_per_step"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    assert not {"sclk_mhz", "roofline", "fp32_mode", "f16x3_mode", "small_batch", "config3", "long_parity", "cpu_baseline"} & set(d)
    assert a.dtype == np.float32 and a.shape == (16, 2, 128, 128) and np.isfinite(a).all() and a.std() > 0
    # same arguments -> same inputs -> the same output, bit for bit
    _, b = _bench(["--steps", "3", "--warmup", "2"], tmp_path / "b")
    assert np.array_equal(_bits(a), _bits(b))
    # warm-up and timed steps are one trajectory: 2 + 3 steps end where 4 + 1 end, and one timed step more goes on from there
    _, c = _bench(["--steps", "1", "--warmup", "4"], tmp_path / "c")
    assert np.array_equal(_bits(a), _bits(c))
    _, e = _bench(["--steps", "4", "--warmup", "2"], tmp_path / "e")
    assert np.isfinite(e).all() and not np.array_equal(_bits(a), _bits(e))
