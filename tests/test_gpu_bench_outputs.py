"""bench.py on the GPU at a tiny size: a plain run times exactly --steps steps and measures nothing
else, --dump-outputs writes what the last step computed, and the same arguments give the same
inputs (and, the step being deterministic, the same outputs) run after run."""
import json
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--config", "2l_dflt", "--size", "32", "32", "32", "--steps", "2", "--warmup", "2"]


def _run(monkeypatch, capsys, extra):
    monkeypatch.setattr("sys.argv", ["bench.py", *ARGS, *extra])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import torch
    with torch.random.fork_rng(devices=[0]):  # bench seeds the global generators: leave them as they were
        bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_dumps_the_last_step(gpu, tmp_path, monkeypatch, capsys):
    lines = [_run(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 2 and line["warmup"] == 2 and line["launch"] == "hip_graph"
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 2) < 1e-6  # batch 2
        assert line["unit"] == "volumes/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert not {"roofline", "roofline_top", "cpu_baseline"} & set(line)  # those are --full's
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == sorted(b) and {"loss.npy", "params.npy"} <= set(a)
    assert any(f.startswith("buffer.") and f.endswith("embed.npy") for f in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a["loss.npy"]) == lines[0]["config"]["final_loss"]
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.isfinite(a[f]).all(), f
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), f
