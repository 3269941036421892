"""GPU: `python -m vq3d.train_prior` end to end on a tiny code store -- training through the captured
step (fused head, device-side mixup draws), validation metrics, the checkpoints, resuming, and the
hand-over to the sampler (vq3d.sample reads what this entry writes: the pipeline's missing stage)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 16


@pytest.fixture(autouse=True, scope="module")
def _restore_operand_dtype():
    """PixelSNAIL.hidden leaves its compute dtype in pixelsnail's module state, which the bare-layer tests of
    tests/test_gpu_pixelsnail.py (run later in the same process) read as fp32: put it back"""
    from vq3d import pixelsnail as PS
    prev = PS._compute[0], PS._shadow[0]
    yield
    PS._compute[0], PS._shadow[0] = prev


TINY = ["--use-model", "pixelsnail", "--metric", "cross_entropy", "--batch-size", "2", "--model-dim", "32",
        "--num-blocks", "1", "--num-layers-per-block", "1", "--gpus", "1", "--log_every_n_steps", "1"]


def _store(root, volumes):
    from vq3d.extract import CodeStore
    with CodeStore(str(root), [K], len(volumes)) as st:
        for i, v in enumerate(volumes):
            st.put(i, [v])
    return str(root)


def _datamodule(root):
    from vq3d import train_prior as TP
    return TP.CodesDataModule(root, embedding_id=0, batch_size=2, num_workers=0)  # no worker processes in a test


@pytest.fixture(scope="module")
def run(gpu, tmp_path_factory):
    """24 random (1, 4, 4, 4) volumes, 4 steps with graphs on (StepGraph warms up for 2 steps: at least
    one replay), validation every 2 batches"""
    from vq3d import train_prior as TP
    tmp = tmp_path_factory.mktemp("prior")
    g = np.random.default_rng(0)
    root = _store(tmp / "codes", [g.integers(0, K, (1, 4, 4, 4)) for _ in range(24)])
    out = tmp / "run"
    argv = [root, "0"] + TINY + ["--max_steps", "4", "--val_check_interval", "2", "--mixup-alpha", "0.2",
                                 "--lr", "1e-3", "--default_root_dir", str(out)]
    model, opt, history, ckpt = TP.cli(argv, datamodule=_datamodule(root))
    return dict(root=root, out=out, model=model, history=history, ckpt=ckpt)


def test_checkpoints_and_validation_metrics(run):
    from vq3d import train_prior as TP
    ckdir = run["out"] / "checkpoints"
    assert (ckdir / "last.ckpt").exists()
    assert len(glob.glob(str(ckdir / "epoch=*-step=*.ckpt"))) == 1
    vm = run["model"].val_metrics
    assert set(vm) == set(TP.VAL_KEYS) and len(vm) == 7
    assert all(math.isfinite(v) for v in vm.values()), vm
    assert 0.0 <= vm["val_accuracy"] <= 1.0
    assert vm["val_bits_per_dim"] == pytest.approx(vm["val_loss_mean"] / math.log(2), rel=1e-12)
    assert vm["val_loss_min"] <= vm["val_loss_median"] <= vm["val_loss_max"]
    # two validations (steps 2 and 4): the kept score is the lower, vm the later
    assert run["ckpt"].monitor == "val_loss_mean" and run["ckpt"].best_score <= vm["val_loss_mean"] + 1e-12
    # the step logs: every step here, six keys, finite
    assert [s for s, _ in run["history"]] == [1, 2, 3, 4]
    for _, log in run["history"]:
        assert set(log) == {"train_loss_min", "train_loss_max", "train_loss_mean", "train_loss_median",
                            "train_loss_std", "train_bits_per_dim"}
        assert all(math.isfinite(v) for v in log.values()), log
    # the replayed steps (3, 4) saw their own batches and mixup draws: their logs differ
    assert run["history"][2][1] != run["history"][3][1]


def test_the_sampler_accepts_the_checkpoint(run, gpu):
    from vq3d.checkpoint import load_from_checkpoint
    from vq3d.pixelsnail import PixelSNAIL
    from vq3d.sample import sample_codes
    m = load_from_checkpoint(PixelSNAIL, str(run["out"] / "checkpoints" / "last.ckpt")).to(gpu)
    assert m.input_dim == K
    for (n, p), (_, q) in zip(m.state_dict().items(), run["model"].state_dict().items()):
        assert torch.equal(p, q), n
    m.eval()
    codes = sample_codes(m, (2, 2, 2), batch_size=2, seed=1)
    assert codes.shape == (2, 2, 2, 2) and codes.dtype == torch.int64
    assert int(codes.min()) >= 0 and int(codes.max()) < K


def test_resume_continues_at_the_saved_step(run, monkeypatch, tmp_path):
    from vq3d import train_prior as TP
    from vq3d.checkpoint import load_checkpoint
    last = str(run["out"] / "checkpoints" / "last.ckpt")
    ck = load_checkpoint(last)
    assert ck["global_step"] == 4
    seen = {}
    fit = TP._fit

    def spy(args, model, opt, reducer, ckpt, datamodule, rank, world, dev, epoch0, step, scaler):
        seen.update(epoch0=epoch0, step=step, adam=opt.step_count,
                    sd={n: v.detach().cpu().clone() for n, v in model.state_dict().items()})
        ckpt.best_path = None  # leave the first run's best checkpoint file alone
        return fit(args, model, opt, reducer, ckpt, datamodule, rank, world, dev, epoch0, step, scaler)
    monkeypatch.setattr(TP, "_fit", spy)
    argv = [run["root"], "0"] + TINY + ["--max_steps", "6", "--hip-graph", "0", "--resume_from_checkpoint", last,
                                        "--default_root_dir", str(tmp_path)]
    _, opt, history, _ = TP.cli(argv, datamodule=_datamodule(run["root"]))
    assert (seen["epoch0"], seen["step"], seen["adam"]) == (ck["epoch"], 4, 4)
    assert set(seen["sd"]) == set(ck["state_dict"])
    for n, v in ck["state_dict"].items():
        assert torch.equal(seen["sd"][n], v), n
    assert [s for s, _ in history] == [5, 6] and opt.step_count == 6
    assert load_checkpoint(str(tmp_path / "checkpoints" / "last.ckpt"))["global_step"] == 6


def test_loss_falls_on_a_constant_store(gpu, tmp_path):
    """every volume the same constant code: after 30 eager steps the logged training loss is below the first"""
    from vq3d import train_prior as TP
    root = _store(tmp_path / "codes", [np.full((1, 4, 4, 4), 3)] * 24)
    argv = [root, "0"] + TINY + ["--max_steps", "30", "--hip-graph", "0", "--lr", "1e-2", "--causal-dropout-prob", "0",
                                 "--attention-dropout-prob", "0", "--default_root_dir", str(tmp_path / "run")]
    _, _, history, _ = TP.cli(argv, datamodule=_datamodule(root))
    assert history[0][0] == 1 and history[-1][0] == 30
    first, last = history[0][1]["train_loss_mean"], history[-1][1]["train_loss_mean"]
    print(f"constant store: train_loss_mean {first:.4f} -> {last:.4f}")
    assert last < first
    assert os.path.exists(tmp_path / "run" / "checkpoints" / "last.ckpt")
