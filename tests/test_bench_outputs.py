"""bench.py's plain run and its --dump-outputs: exactly --steps timed steps, the result line's headline fields, nothing of --full,
and the outputs of the last timed step as float32 / float64 .npy files within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_whole_or_a_fixed_sorted_sample(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    small = torch.arange(10, dtype=torch.float32)
    assert torch.equal(bench._dump_sample(small, 0), small)
    monkeypatch.setattr(bench, "DUMP_MAX_ENTRIES", 64)
    big = torch.arange(10000, dtype=torch.float32).view(100, 100)
    a, b = bench._dump_sample(big, 0), bench._dump_sample(big, 0)
    assert a.shape == (64,) and torch.equal(a, b)                      # the same positions on every call
    assert bool((a[1:] >= a[:-1]).all()) and 0 <= float(a.min()) and float(a.max()) < 10000
    assert not torch.equal(bench._dump_sample(big, 1), a)              # another seed, other positions


@pytest.mark.gpu
def test_plain_bench_times_steps_and_dumps_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "bedroom21", "--steps", "2",
                        "--warmup", "3", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] and line["value"] > 0
    assert line["steps"] == 2 and line["statistic"] == "one timed region of 2 steps"
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) / line["value"] < 1e-2
    assert not {"roofline", "cpu_baseline", "other_configs", "full_loop", "sample", "train"} & set(line)
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"sample_x.npy", "train_loss.npy", "train_params.npy", "train_grads.npy"}
    assert files["sample_x.npy"].shape == (256, 21, 62) and files["train_loss.npy"].shape == (1,)
    assert files["train_params.npy"].shape == files["train_grads.npy"].shape
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
