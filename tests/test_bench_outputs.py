"""CPU: bench.py's --dump-outputs writer and the plain / --full split of its command line."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

import bench  # noqa: E402


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=240, env=env)


def test_dump_outputs_formats(tmp_path):
    named = [("loss", torch.tensor(1.25, dtype=torch.bfloat16)),
             ("codes level0", torch.arange(2 ** 40, 2 ** 40 + 6, dtype=torch.int64).view(1, 2, 3)),
             ("buffer.embed", torch.arange(8, dtype=torch.float32).view(2, 4).requires_grad_(True))]
    bench.dump_outputs(str(tmp_path / "out"), named)
    got = {f: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["buffer.embed.npy", "codes_level0.npy", "loss.npy"]
    assert got["loss.npy"].dtype == np.float32 and got["loss.npy"].shape == () and got["loss.npy"] == 1.25
    # 64-bit integers go to float64: exact where float32 would round
    assert got["codes_level0.npy"].dtype == np.float64 and got["codes_level0.npy"].shape == (1, 2, 3)
    assert (got["codes_level0.npy"].ravel() == np.arange(2 ** 40, 2 ** 40 + 6)).all()
    assert got["buffer.embed.npy"].dtype == np.float32 and got["buffer.embed.npy"].shape == (2, 4)


def test_dump_outputs_samples_over_budget(tmp_path, monkeypatch):
    """Over the budget, an array larger than its share is cut to a fixed sample of its elements:
    the same indices in every call, in order, and the files stay within the budget."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = torch.arange(5000, dtype=torch.float32)
    small = torch.arange(10, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("big", big + (d == "b")), ("small", small)])
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (4096 // 2 // 4,) and (np.diff(a) > 0).all() and len(set(a.tolist())) == len(a)
    assert (b == a + 1).all()  # the same elements of the second call's array
    assert (np.load(tmp_path / "a" / "small.npy") == small.numpy()).all()
    assert a.nbytes + small.numel() * 4 <= 4096


def test_plain_and_full_runs_of_the_plumbing_bench(tmp_path):
    """--dump-outputs / --full on the CPU stand-in step: the same arguments give the same arrays,
    --steps sets the number of timed steps, the result line keeps its fields."""
    lines = []
    for d, extra in (("a", []), ("b", ["--full"])):
        r = _bench("--gpus", "1", "--cpu-plumbing", "--steps", "3", "--warmup", "1", "--dump-outputs",
                   str(tmp_path / d), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert {"metric", "value", "unit", "higher_is_better", "dtype"} <= set(line)
    a, b = np.load(tmp_path / "a" / "buf.npy"), np.load(tmp_path / "b" / "buf.npy")
    assert a.dtype == np.float32 and a.shape == (1 << 16,) and (a == 1.0).all() and (a == b).all()
