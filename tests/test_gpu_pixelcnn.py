"""Conditioned PixelCNN prior on the GPU (vq3d.pixelcnn: the PixelSNAIL blocks plus vq3d.cond_embed and the
fused add-pre-activation) against the reference's own outputs (tests/golden/pcnn_*.npz), its sampler against
one full forward, and `python -m vq3d.train_pixelcnn` / `vq3d.sample --use-model pixelcnn` end to end.

Tolerances are those of tests/test_gpu_pixelsnail.py (test_causal_block_golden, test_pixelsnail_model_golden):
fp32 path 1e-4 of the logits' max, every gradient tensor 1e-3, the whole gradient 1e-4 relative L2; bf16
path: logits / loss 3e-2, every weight-tensor gradient 8e-2 of its max, the whole gradient 3e-2 relative L2
with cosine >= 0.999, the scalar bias / scale gradients as one vector 0.1.  The sampler's are
tests/test_gpu_sample.py's: fp32 1e-4 and bf16 3e-2 of max |logit|.
"""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

G = "tests/golden/"
CL = torch.channels_last_3d


@pytest.fixture(autouse=True, scope="module")
def _restore_operand_dtype():
    """the model's forward leaves its compute dtype in pixelsnail's module state, which bare-layer tests read as
    fp32: put it back"""
    from vq3d import pixelsnail as PS
    prev = PS._compute[0], PS._shadow[0]
    yield
    PS._compute[0], PS._shadow[0] = prev


def P_of(d, pre="p/"):
    return {k[len(pre):]: torch.tensor(d[k]) for k in d.files if k.startswith(pre)}


def rel(a, b):
    a = np.asarray(a.detach().float().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def test_conditioned_block_golden(gpu):
    from vq3d import pixelsnail as PS
    d = np.load(G + "pcnn_block_cond.npz")
    c = d["x"].shape[2]
    m = PS.PreActFixupCausalResBlock(c, c, 3, mask="B", dropout_prob=0.0, bottleneck_divisor=4, condition_dim=c)
    m.load_state_dict(P_of(d), strict=True)
    m = m.to(gpu)
    xs = [torch.tensor(d["x"][i]).to(gpu).contiguous(memory_format=CL).requires_grad_(True) for i in range(3)]
    e = torch.tensor(d["cond"]).to(gpu).contiguous(memory_format=CL).requires_grad_(True)
    y = m(xs, condition=e)
    assert rel(y, d["y"]) < 1e-5
    y.backward(torch.tensor(d["gy"]).to(gpu))
    assert rel(torch.stack([t.grad for t in xs]), d["gx"]) < 1e-4
    assert rel(e.grad, d["gcond"]) < 1e-4
    scale = max(np.abs(d["g/" + n]).max() for n, _ in m.named_parameters())
    for n, p in m.named_parameters():
        err = np.abs(p.grad.detach().cpu().numpy() - d["g/" + n]).max()
        assert err <= max(1e-4 * np.abs(d["g/" + n]).max(), 1e-5 * scale), n
    # the cache form: the projection popped from the deque gives the same output
    from collections import deque
    with torch.no_grad():
        cache = deque([m.project_condition(e.detach(), tuple(e.shape[2:]))])
        assert torch.equal(m(xs, condition_cache=cache), y.detach()) and not cache


def _model(gpu, dtype, d=None, **kw):
    from vq3d import pixelcnn as PC
    d = np.load(G + "pcnn_model_cond.npz") if d is None else d
    k, kc, md, nr, bd = (int(c) for c in d["cfg"])
    args = PC.default_args(num_embeddings=[k, kc], model_dim=md, num_resblocks=nr, bottleneck_divisor=bd,
                           dropout_prob=0.0, use_pre_activation=True, use_conditioning=True, mixup_alpha=0, lr=1e-3)
    m = PC.PixelCNN(args, compute_dtype=dtype)
    m.load_state_dict(P_of(d), strict=True)
    return m.to(gpu), d


def _check_gradients(m, d, gp, dtype, gtol):
    """every parameter gradient against the golden's, as tests/test_gpu_pixelsnail.py::test_pixelsnail_model_golden"""
    scale = max(np.abs(d[gp + n]).max() for n, _ in m.named_parameters())
    worst = 0.0
    sc_mine, sc_ref, all_mine, all_ref = [], [], [], []
    for n, p in m.named_parameters():
        ref = d[gp + n]
        mine = p.grad.detach().cpu().numpy()
        all_mine.append(mine.ravel())
        all_ref.append(ref.ravel())
        if p.numel() == 1 and dtype == "bf16":
            sc_mine.append(mine.ravel())
            sc_ref.append(ref.ravel())
            continue
        err = np.abs(mine - ref).max() / max(np.abs(ref).max(), 1e-3 * scale)
        worst = max(worst, err)
        assert err <= gtol, n
    print(dtype, "worst tensor gradient error (of max(|ref|, 1e-3 scale))", worst)
    a, b = np.concatenate(all_mine).astype(np.float64), np.concatenate(all_ref).astype(np.float64)
    l2 = np.linalg.norm(a - b) / np.linalg.norm(b)
    cos = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    print(dtype, "whole gradient rel L2", l2, "cosine", cos)
    assert l2 <= (1e-4 if dtype == "fp32" else 3e-2) and cos >= 0.999
    if sc_mine:
        a, b = np.concatenate(sc_mine).astype(np.float64), np.concatenate(sc_ref).astype(np.float64)
        sl2 = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(dtype, "scalar-parameter gradients as one vector: rel L2", sl2)
        assert sl2 <= 0.1


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("dtype,tol,gtol", [("fp32", 1e-4, 1e-3), ("bf16", 3e-2, 8e-2)])
def test_pixelcnn_model_golden(gpu, dtype, tol, gtol, mix):
    """whole conditioned prior: logits, loss and every parameter gradient of a training step (dropout 0), without
    mixup and with the lam / index the reference's mixup_data drew for the golden"""
    m, d = _model(gpu, dtype)
    m.train()
    k = m.input_dim
    data, cond = torch.tensor(d["data"]).to(gpu), torch.tensor(d["condition"]).to(gpu)
    codes = data.squeeze(1)
    onehot = torch.nn.functional.one_hot(codes, k).permute(0, 4, 1, 2, 3).float()
    if mix:
        lam, index = float(d["lam"]), torch.tensor(d["index"])
        loss, _ = m.cross_entropy_onehot(onehot, codes, (lam, index), cond)
        gp, want_logits, want_loss = "gm/", d["logits_mix"], d["loss_mix"]
    else:
        loss, _ = m.cross_entropy((data, cond))
        gp, want_logits, want_loss = "g/", d["logits"], d["loss"]
    loss.backward()
    with torch.no_grad():
        if mix:
            lam_t = torch.tensor(lam, dtype=torch.float32, device=gpu)
            idx = index.to(gpu)
            logits = m.logits(lam * onehot + (1 - lam) * onehot[idx], cond, mix=(lam_t, idx))
        else:
            logits = m.logits(onehot, cond)
    print(dtype, "mix", mix, "loss", float(loss), float(want_loss), "logits rel", rel(logits, want_logits))
    assert rel(logits, want_logits) < tol
    assert abs(float(loss) - float(want_loss)) < tol * abs(float(want_loss))
    _check_gradients(m, d, gp, dtype, gtol)
    for n, p in m.named_parameters():
        if "condition" in n:
            assert float(p.grad.abs().max()) > 0, n


@pytest.mark.parametrize("dtype,tol,gtol", [("fp32", 1e-4, 1e-3), ("bf16", 3e-2, 8e-2)])
def test_unconditioned_model_golden(gpu, dtype, tol, gtol):
    """use_conditioning=False at the published top prior's width (model-dim 16: the 4-channel branches' 1x1x1
    convs fall back to F.linear): logits, loss and every gradient against the reference's, then the sampler"""
    from vq3d import pixelcnn as PC
    from vq3d.sample import sample_codes
    d = np.load(G + "pcnn_model_plain.npz")
    k, _, md, nr, bd = (int(c) for c in d["cfg"])
    args = PC.default_args(num_embeddings=[k, 0], model_dim=md, num_resblocks=nr, bottleneck_divisor=bd,
                           dropout_prob=0.0, use_pre_activation=True, use_conditioning=False, mixup_alpha=0, lr=1e-3)
    m = PC.PixelCNN(args, compute_dtype=dtype)
    m.load_state_dict(P_of(d), strict=True)
    m = m.to(gpu).train()
    data = torch.tensor(d["data"]).to(gpu)
    loss, _ = m.cross_entropy((data,))
    loss.backward()
    onehot = torch.nn.functional.one_hot(data.squeeze(1), k).permute(0, 4, 1, 2, 3).float()
    with torch.no_grad():
        logits = m.logits(onehot)
    print(dtype, "plain loss", float(loss.detach()), float(d["loss"]), "logits rel", rel(logits, d["logits"]))
    assert rel(logits, d["logits"]) < tol
    assert abs(float(loss.detach()) - float(d["loss"])) < tol * abs(float(d["loss"]))
    _check_gradients(m, d, "g/", dtype, gtol)
    m.eval()
    codes, rows = sample_codes(m, (2, 3, 4), batch_size=2, seed=3, return_logits=True)
    with torch.no_grad():
        full = m.logits(torch.nn.functional.one_hot(codes, k).permute(0, 4, 1, 2, 3).float())
    assert float((rows - full).abs().max()) <= (1e-4 if dtype == "fp32" else 3e-2) * float(full.abs().max())
    with pytest.raises(ValueError, match="without conditioning"):
        m.hidden(onehot, condition=torch.zeros((2, 1, 1, 1), dtype=torch.int64, device=gpu))


def test_the_condition_changes_the_logits(gpu):
    m, d = _model(gpu, "fp32")
    m.eval()
    data, cond = torch.tensor(d["data"]).to(gpu), torch.tensor(d["condition"]).to(gpu)
    onehot = torch.nn.functional.one_hot(data.squeeze(1), m.input_dim).permute(0, 4, 1, 2, 3).float()
    with torch.no_grad():
        a = m.logits(onehot, cond)
        b = m.logits(onehot, (cond + 1) % m.condition_dim)
        c = m(onehot, condition=cond.squeeze(1))
    assert rel(b, d["logits_other"]) < 1e-4 and torch.equal(a, c)
    assert float((a - b).abs().max()) > 1e-3 * float(a.abs().max())
    # the loss through the fused head (what the training step runs) is the logits' cross-entropy
    rows, pred = m.loss_rows(onehot, data.squeeze(1), condition=cond)
    ce = torch.nn.functional.cross_entropy(a, data.squeeze(1), reduction="none")
    assert float((rows - ce).abs().max()) < 1e-4 and torch.equal(pred, a.argmax(1))


@pytest.mark.parametrize("lanes", [True, False])
def test_gradients_are_bit_identical_run_to_run(gpu, lanes):
    """bf16, with the captured step's device-side mixup, the three stack streams on their lanes and not"""
    from vq3d import pixelsnail as PS
    m, d = _model(gpu, "bf16")
    m.train()
    data, cond = torch.tensor(d["data"]).to(gpu), torch.tensor(d["condition"]).to(gpu).squeeze(1)
    codes = data.squeeze(1)
    onehot = torch.nn.functional.one_hot(codes, m.input_dim).permute(0, 4, 1, 2, 3).float()
    lam_t = torch.tensor(0.3, dtype=torch.float32, device=gpu)
    index_t = torch.tensor([1, 0], dtype=torch.int64, device=gpu)
    prev = PS.lanes_mode()
    PS.set_lanes(lanes)
    try:
        runs = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            rows, _ = m.loss_rows(onehot, codes, (lam_t, index_t), condition=cond)
            rows.mean().backward()
            torch.cuda.synchronize()
            runs.append([rows.detach().clone()] + [p.grad.detach().clone() for p in m.parameters()])
    finally:
        PS.set_lanes(prev)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(float(g.abs().max()) > 0 for (n, _), g in zip(m.named_parameters(), runs[0][1:]) if "condition" in n)


# ------------------------------------------------------------------ the sampler
def _fresh(gpu, dtype="fp32", k=16, kc=8):
    """freshly initialised (branch_conv3 is zero then), every parameter perturbed"""
    from vq3d import pixelcnn as PC
    torch.manual_seed(0)
    m = PC.PixelCNN(PC.default_args(num_embeddings=[k, kc], model_dim=32, num_resblocks=2, use_pre_activation=True,
                                    use_conditioning=True), compute_dtype=dtype)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, p in sorted(m.named_parameters()):
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(gpu).eval()


def _teacher_forced(m, size, csize, batch, tol, **kw):
    from vq3d.sample import sample_codes
    cond = torch.randint(0, m.condition_dim, (batch,) + csize, generator=torch.Generator().manual_seed(2)).to(
        m.parse_output.weight.device)
    codes, rows = sample_codes(m, size, batch_size=batch, seed=3, return_logits=True, condition=cond, **kw)
    assert codes.shape == (batch,) + size and codes.dtype == torch.int64 and codes.is_cuda
    with torch.no_grad():
        onehot = torch.nn.functional.one_hot(codes, m.input_dim).permute(0, 4, 1, 2, 3).float()
        full = m.logits(onehot, cond)
        other = m.logits(onehot, (cond + 1) % m.condition_dim)
    scale = float(full.abs().max())
    err = float((rows - full).abs().max())
    print(f"size {size} {m.compute_dtype}: teacher-forced error {err:.3e}, max |logit| {scale:.3f}, bound {tol * scale:.3e}")
    assert torch.isfinite(rows).all() and scale > 0
    assert err <= tol * scale
    assert len(torch.unique(codes)) > 1
    assert float((rows - other).abs().max()) > err  # the rows are those of THIS condition
    return codes, rows, cond


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_sampler_rows_equal_one_full_conditioned_forward(gpu, dtype, tol):
    m, _ = _model(gpu, dtype)
    _teacher_forced(m.eval(), (4, 4, 4), (2, 2, 1), 2, tol)


def test_sampler_rows_equal_one_full_forward_odd_grid(gpu):
    _teacher_forced(_fresh(gpu), (3, 5, 7), (2, 2, 3), 2, 1e-4)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_equals_eager(gpu, dtype):
    from vq3d.sample import sample_codes
    m, _ = _model(gpu, dtype)
    m.eval()
    cond = torch.randint(0, m.condition_dim, (2, 2, 2, 1), generator=torch.Generator().manual_seed(2)).to(gpu)
    eager, rows = sample_codes(m, (4, 4, 4), batch_size=2, seed=5, return_logits=True, condition=cond)
    replayed, rows_g = sample_codes(m, (4, 4, 4), batch_size=2, seed=5, return_logits=True, graphs=True, condition=cond)
    assert torch.equal(eager, replayed) and torch.equal(rows, rows_g)


# ------------------------------------------------------------------ the entries
K, KC = 16, 8
TINY = ["--metric", "cross_entropy", "--use-pre-activation", "True", "--use-conditioning", "True", "--batch-size", "2",
        "--model-dim", "32", "--num-resblocks", "1", "--gpus", "1", "--log_every_n_steps", "1"]


def _two_level_store(root, n=24, seed=0):
    """upper level random (1, 2, 2, 2) codes; the lower level (1, 4, 4, 4) a fixed function of the upper: each
    lower voxel is twice the code of the upper voxel above it"""
    from vq3d.extract import CodeStore
    g = np.random.default_rng(seed)
    with CodeStore(str(root), [K, KC], n) as st:
        for i in range(n):
            up = g.integers(0, KC, (1, 2, 2, 2))
            low = 2 * up.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
            st.put(i, [low, up])
    return str(root)


@pytest.mark.parametrize("mixup", ["0", "0.4"])
def test_command_line_trains_checkpoints_and_samples(tmp_path, mixup):
    """python -m vq3d.train_pixelcnn in a child process on a two-level store (captured steps: the condition is the
    StepGraph's second static input), then python -m vq3d.sample --use-model pixelcnn --condition-from on its
    checkpoint"""
    from vq3d.checkpoint import load_checkpoint, load_from_checkpoint
    from vq3d.pixelcnn import PixelCNN
    root = _two_level_store(tmp_path / "codes")
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "vq3d.train_pixelcnn", root, "0"] + TINY + [
        "--max_steps", "4", "--val_check_interval", "2", "--mixup-alpha", mixup, "--lr", "1e-3", "--default_root_dir",
        str(out)]
    run = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    last = out / "checkpoints" / "last.ckpt"
    assert last.exists()
    steps = [ln for ln in run.stdout.splitlines() if "train_loss_mean" in ln]
    assert len(steps) == 4 and "val_accuracy" in run.stdout
    sd = load_checkpoint(str(last))["state_dict"]
    m = load_from_checkpoint(PixelCNN, str(last))
    assert m.use_conditioning and (m.input_dim, m.condition_dim) == (K, KC) and len(m.layers) == 2
    for key in ["embed_condition.weight", "embed_condition.bias"] + [f"layers.{i}.condition.{p}" for i in range(2)
                                                                     for p in ("weight", "bias")]:
        assert key in sd and torch.equal(m.state_dict()[key], sd[key]), key
    if mixup != "0":
        return
    # the sampler's entry reads the checkpoint and a directory holding the level above
    from vq3d.extract import CodeStore
    g = np.random.default_rng(5)
    with CodeStore(str(tmp_path / "upper"), [KC], 2) as st:
        for i in range(2):
            st.put(i, [g.integers(0, KC, (1, 2, 2, 2))])
    codes = tmp_path / "sampled"
    cmd = [sys.executable, "-m", "vq3d.sample", str(last), "--use-model", "pixelcnn", "--condition-from",
           str(tmp_path / "upper"), "--size", "4", "4", "4", "--num-samples", "3", "--batch-size", "2", "--dtype", "bf16",
           "--out", str(codes)]
    run = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert json.loads((codes / "meta.json").read_text()) == {"num_dbs": 1, "length": 3, "num_embeddings": [K]}
    level = np.load(codes / "level0.npy")
    assert level.shape == (3, 1, 4, 4, 4) and level.min() >= 0 and level.max() < K
    # without the condition the entry refuses a conditioned checkpoint
    run = subprocess.run(cmd[:6] + cmd[8:], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert run.returncode != 0 and "--condition-from is required" in run.stderr


def test_loss_falls_when_the_lower_level_follows_the_upper(gpu, tmp_path):
    """the lower level a fixed function of the upper: after 30 eager steps the logged training loss is below the
    first (the criterion of test_gpu_train_prior.py::test_loss_falls_on_a_constant_store), and the trained model
    needs the true condition: an unconditioned model would also learn that every lower code is even"""
    from vq3d import train_pixelcnn as TC
    from vq3d import train_prior as TP
    root = _two_level_store(tmp_path / "codes")
    argv = [root, "0"] + TINY + ["--max_steps", "30", "--hip-graph", "0", "--lr", "1e-2", "--dropout-prob", "0",
                                 "--mixup-alpha", "0", "--default_root_dir", str(tmp_path / "run")]
    dm = TP.CodesDataModule(root, embedding_id=0, batch_size=2, num_workers=0)
    model, _, history, _ = TC.cli(argv, datamodule=dm)
    assert history[0][0] == 1 and history[-1][0] == 30
    first, last = history[0][1]["train_loss_mean"], history[-1][1]["train_loss_mean"]
    print(f"conditioned store: train_loss_mean {first:.4f} -> {last:.4f}")
    assert last < first
    assert (tmp_path / "run" / "checkpoints" / "last.ckpt").exists()
    # what it learnt is the condition, not only that lower codes are even: on a batch of the store, the trained
    # model's loss under the true upper level is below its loss under another upper level's codes
    from vq3d.train_prior import onehot_codes
    batch = next(iter(dm.val_dataloader()))
    codes, cond = batch[0].squeeze(1).to(gpu), batch[1].squeeze(1).to(gpu)
    model.eval()
    with torch.no_grad():
        true_rows, _ = model.loss_rows(onehot_codes(codes, K), codes, condition=cond)
        other_rows, _ = model.loss_rows(onehot_codes(codes, K), codes, condition=(cond + 3) % KC)
    print(f"trained loss under the true condition {float(true_rows.mean()):.4f}, under another {float(other_rows.mean()):.4f}")
    assert float(true_rows.mean()) < 0.5 * float(other_rows.mean())
