"""GPU: the prior sampler -- the head-and-sampling kernel (csrc/sample.hip) against the host
restatement of its definition (vq3d.sample, tests/test_sample_cpu.py), and the whole sampler
teacher-forced against one full forward of the model.

Kernel bounds.  logits_out against a float64 evaluation of the same (rounded) operands: the fp32
accumulation bound 2 c 2^-24 sum_c |hid W| per logit.  Codes: the restatement's draw from the kernel's
own logits_out; a row whose two best float64 scores are closer than 1e-3 is left out (the fp32 noise
of device and host logf may differ in the last place), and at most 0.5 % of a case's rows may be --
every case here has fewer than 200 rows, so none.
Whole sampler: the logit rows the draws used against `m.logits(one_hot(codes))`, within the
project's bounds for this model (tests/test_gpu_pixelsnail.py): 1e-4 (fp32) and 3e-2 (bf16) of the
largest |logit|.  That one comparison covers causality, the slab-prefix crop, the background crop
and the one-hot writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

G = "tests/golden/"
CL = torch.channels_last_3d
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(8, 32, 2), (128, 64, 1), (256, 256, 3), (512, 1024, 1), (1000, 8, 2)]  # (k, c, batch)
GRID, NPOS = (4, 4, 4), 64
TIE = 1e-3


def _inputs(k, c, batch, dtype, grid=GRID, seed=0):
    """hidden rows ~ N(0, 1) in dtype, parse_output parameters giving logits of scale 4"""
    g = torch.Generator().manual_seed(1000 * k + c + seed)
    hid = torch.randn((batch, c) + grid, generator=g).to(dtype).contiguous(memory_format=CL)
    weight = torch.randn((k, c), generator=g) * (4.0 / c ** 0.5)
    bias = torch.randn(k, generator=g)
    return hid, weight, bias


def _state(k, batch, dtype, dev):
    """an onehot / codes pair filled with sentinels, so a stray write shows"""
    x = torch.full((batch, k) + GRID, 0.25, dtype=dtype, device=dev).contiguous(memory_format=CL)
    codes = torch.full((batch, NPOS), -7, dtype=torch.int64, device=dev)
    return x, codes


def _scalar(v, dev):
    return torch.tensor(v, dtype=torch.int64, device=dev)


@pytest.mark.parametrize("temperature", [1.0, 0.6])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k,c,batch", SHAPES)
def test_kernel_matches_the_restatement(gpu, k, c, batch, dtype, temperature):
    from vq3d import sample as S
    dt = DTYPES[dtype]
    hid, weight, bias = _inputs(k, c, batch, dt)
    # float64 evaluation of the operands the kernel multiplies
    w64 = (weight if dt == torch.float32 else weight.to(dt)).double()
    rows64 = hid.permute(0, 2, 3, 4, 1).reshape(batch, NPOS, c).double()
    hid_g, w_g, b_g = hid.to(gpu), weight.to(gpu), bias.to(gpu)
    seed, base = 2 ** 40 + 17, 5
    excluded = total = 0
    for p in (0, NPOS // 2, NPOS - 1):
        x, codes = _state(k, batch, dt, gpu)
        x0, c0 = x.clone(), codes.clone()
        lg = torch.full((batch, k), float("nan"), device=gpu)
        S.sample_step(hid_g, w_g, b_g, _scalar(p, gpu), temperature, _scalar(seed, gpu), base, x, codes, lg)
        lg = lg.cpu()
        prod = rows64[:, p, None, :] * w64[None]                      # (batch, k, c)
        ref = bias.double() + prod.sum(-1)
        bound = 2 * c * 2.0 ** -24 * prod.abs().sum(-1)
        err = (lg.double() - ref).abs()
        print(f"k {k} c {c} {dtype} p {p}: logit error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        # the draw, from the kernel's own logits
        want = S.draw_codes(lg.numpy(), temperature, seed, base, p)
        top2 = np.sort(S.perturbed_scores(lg.numpy(), temperature, seed, base, p, np.float64), axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) >= TIE
        total += batch
        excluded += int((~clear).sum())
        got = codes[:, p].cpu().numpy()
        assert np.array_equal(got[clear], want[clear]), (p, got, want)
        assert ((0 <= got) & (got < k)).all()
        # only row p changed, and it is an exact one-hot of the code
        xr, x0r = (t.permute(0, 2, 3, 4, 1).reshape(batch, NPOS, k) for t in (x, x0))
        others = torch.arange(NPOS, device=gpu) != p
        assert torch.equal(xr[:, others], x0r[:, others]) and torch.equal(codes[:, others], c0[:, others])
        assert torch.equal(xr[:, p].float().cpu(), torch.nn.functional.one_hot(torch.from_numpy(got), k).float())
    assert excluded <= 0.005 * total, (excluded, total)


def test_zero_temperature_takes_the_first_maximum(gpu):
    from vq3d import sample as S
    k, c, batch = 16, 8, 2
    hid = torch.zeros((batch, c) + GRID).contiguous(memory_format=CL)
    hid[:, 0] = 1.0
    weight = torch.zeros((k, c))
    weight[[3, 9, 12], 0] = 2.0   # three equal maxima
    bias = torch.zeros(k)
    x, codes = _state(k, batch, torch.float32, gpu)
    for seed in (0, 1):
        S.sample_step(hid.to(gpu), weight.to(gpu), bias.to(gpu), _scalar(7, gpu), 0.0, _scalar(seed, gpu), 0, x, codes)
        assert codes[:, 7].tolist() == [3, 3]


def test_out_of_range_position_writes_nothing(gpu):
    from vq3d import sample as S
    k, c, batch = 8, 32, 2
    hid, weight, bias = _inputs(k, c, batch, torch.float32)
    hid_g, w_g, b_g = hid.to(gpu), weight.to(gpu), bias.to(gpu)
    prefix = hid[:, :, :2].contiguous(memory_format=CL).to(gpu)  # 32 hidden positions of the 64
    for h, p in ((hid_g, -1), (hid_g, NPOS), (hid_g, 2 ** 40), (prefix, 32), (prefix, 40)):
        x, codes = _state(k, batch, torch.float32, gpu)
        lg = torch.full((batch, k), 3.5, device=gpu)
        x0, c0, l0 = x.clone(), codes.clone(), lg.clone()
        S.sample_step(h, w_g, b_g, _scalar(p, gpu), 1.0, _scalar(0, gpu), 0, x, codes, lg)
        assert torch.equal(x, x0) and torch.equal(codes, c0) and torch.equal(lg, l0), p
    x, codes = _state(k, batch, torch.float32, gpu)
    S.sample_step(prefix, w_g, b_g, _scalar(31, gpu), 1.0, _scalar(0, gpu), 0, x, codes)  # the prefix's last row
    assert (codes[:, 31] >= 0).all() and int((codes != -7).sum()) == batch


def test_unsupported_sizes_are_errors(gpu):
    from vq3d import _lib as L
    from vq3d import sample as S
    for k, c in ((7, 32), (1032, 32), (8, 12), (8, 1032)):
        hid = torch.zeros((1, c) + GRID, device=gpu).contiguous(memory_format=CL)
        x, codes = _state(k, 1, torch.float32, gpu)
        args = (hid, torch.zeros((k, c), device=gpu), torch.zeros(k, device=gpu), _scalar(0, gpu), 1.0,
                _scalar(0, gpu), 0, x, codes, None)
        with pytest.raises(ValueError):
            S.sample_step(*args)
        with pytest.raises(L.Vq3dError):
            S.sample_step_kernel(*args)
        assert int((codes != -7).sum()) == 0


def test_operator_equals_ctypes_binding(gpu):
    import vq3d.library  # noqa: F401
    from vq3d import functional as Fn
    from vq3d import sample as S
    k, c, batch = 256, 256, 3
    hid, weight, bias = _inputs(k, c, batch, torch.bfloat16)
    out = []
    for binding in ("ctypes", "library"):
        x, codes = _state(k, batch, torch.bfloat16, gpu)
        lg = torch.empty((batch, k), device=gpu)
        try:
            Fn.set_binding(binding)
            S.sample_step(hid.to(gpu), weight.to(gpu), bias.to(gpu), _scalar(9, gpu), 1.0, _scalar(3, gpu), 0, x,
                          codes, lg)
        finally:
            Fn.set_binding("ctypes")
        out.append((x, codes, lg))
    assert all(torch.equal(a, b) for a, b in zip(*out))


# ------------------------------------------------------------------ the whole sampler
def _golden_prior(gpu, dtype):
    from vq3d import pixelsnail as PS
    d = np.load(G + "psnail_model_32.npz")
    ne, md, nl, nb, bd = (int(c) for c in d["cfg"])
    args = PS.default_args(num_embeddings=[ne, 0], model_dim=md, num_layers_per_block=nl, num_blocks=nb,
                           bottleneck_divisor=bd)
    m = PS.PixelSNAIL(args, compute_dtype=dtype)
    m.load_state_dict({k[2:]: torch.tensor(d[k]) for k in d.files if k.startswith("p/")}, strict=True)
    return m.to(gpu).eval()


def _fresh_prior(gpu, dtype="fp32", k=8, **kw):
    """freshly initialised (branch_conv3 is zero then), every parameter perturbed"""
    from vq3d import pixelsnail as PS
    torch.manual_seed(0)
    m = PS.PixelSNAIL(PS.default_args(num_embeddings=[k, 0], model_dim=32, num_layers_per_block=2, num_blocks=2, **kw),
                      compute_dtype=dtype)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, p in sorted(m.named_parameters()):
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(gpu).eval()


def _teacher_forced(m, size, batch, tol, **kw):
    from vq3d.sample import sample_codes
    codes, rows = sample_codes(m, size, batch_size=batch, seed=3, return_logits=True, **kw)
    assert codes.shape == (batch,) + size and codes.dtype == torch.int64 and codes.is_cuda
    assert rows.shape == (batch, m.input_dim) + size and rows.dtype == torch.float32
    with torch.no_grad():
        full = m.logits(torch.nn.functional.one_hot(codes, m.input_dim).permute(0, 4, 1, 2, 3).float())
    scale = float(full.abs().max())
    err = float((rows - full).abs().max())
    print(f"size {size} {m.compute_dtype}: teacher-forced error {err:.3e}, max |logit| {scale:.3f}, bound {tol * scale:.3e}")
    assert torch.isfinite(rows).all() and scale > 0
    assert err <= tol * scale
    assert len(torch.unique(codes)) > 1
    return codes


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_sampler_rows_equal_one_full_forward(gpu, dtype, tol):
    _teacher_forced(_golden_prior(gpu, dtype), (4, 4, 4), 2, tol)


def test_sampler_rows_equal_one_full_forward_odd_grid(gpu):
    _teacher_forced(_fresh_prior(gpu), (3, 5, 7), 2, 1e-4)


def test_sampler_is_deterministic(gpu):
    from vq3d.sample import sample_codes
    m = _golden_prior(gpu, "bf16")
    a = sample_codes(m, (4, 4, 4), batch_size=2, seed=5)
    assert torch.equal(a, sample_codes(m, (4, 4, 4), batch_size=2, seed=5))
    assert not torch.equal(a, sample_codes(m, (4, 4, 4), batch_size=2, seed=6))
    # sample_base continues the stream of samples: sample 1 of the batch is sample 0 of base 1 (fp32: a
    # batch of another size may run other kernels, whose rounding a 16-bit draw could feel)
    m32 = _golden_prior(gpu, "fp32")
    pair = sample_codes(m32, (4, 4, 4), batch_size=2, seed=5)
    assert torch.equal(pair[1], sample_codes(m32, (4, 4, 4), batch_size=1, seed=5, sample_base=1)[0])
    assert not torch.equal(pair[0], pair[1])
    cold = sample_codes(m, (4, 4, 4), batch_size=2, seed=5, temperature=0.0)
    assert torch.equal(cold, sample_codes(m, (4, 4, 4), batch_size=2, seed=77, temperature=0.0))
    assert torch.equal(cold[0], cold[1])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_equals_eager(gpu, dtype):
    from vq3d import pixelsnail as PS
    from vq3d.sample import sample_codes
    m = _golden_prior(gpu, dtype)
    eager, rows = sample_codes(m, (4, 4, 4), batch_size=2, seed=5, return_logits=True)
    lanes = PS.lanes_mode()
    replayed, rows_g = sample_codes(m, (4, 4, 4), batch_size=2, seed=5, return_logits=True, graphs=True)
    assert PS.lanes_mode() == lanes
    assert torch.equal(eager, replayed) and torch.equal(rows, rows_g)


def test_command_line_round_trip(tmp_path):
    """python -m vq3d.sample in a child process (started before this test touches the GPU): the code
    directory, and with a VQ-VAE checkpoint and its other level's codes the decoded NRRD volumes"""
    import vq3d
    from vq3d import pixelsnail as PS
    from vq3d.checkpoint import load_from_checkpoint, save_checkpoint
    from vq3d.decode import read_nrrd
    from vq3d.extract import CodeStore
    from vq3d.sample import sample_codes
    k, size, n = 256, (2, 2, 2), 3
    torch.manual_seed(0)
    prior = PS.PixelSNAIL(PS.default_args(num_embeddings=[k, 0], model_dim=32, num_layers_per_block=1, num_blocks=1))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, p in sorted(prior.named_parameters()):
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    save_checkpoint(str(tmp_path / "prior.ckpt"), prior)
    # a 2-level VQ-VAE on 32^3 volumes: bottom codes (8, 8, 8), top codes (2, 2, 2) -- the sampled level
    vqvae = vq3d.VQVAE(vq3d.default_args(n_bottleneck_blocks=2))
    save_checkpoint(str(tmp_path / "vqvae.ckpt"), vqvae)
    rng = np.random.default_rng(0)
    with CodeStore(str(tmp_path / "bottom"), [k], 2) as st:
        for i in range(2):
            st.put(i, [rng.integers(0, k, size=(1, 8, 8, 8), dtype=np.int64)])
    out, nrrd = tmp_path / "codes", tmp_path / "volumes"
    cmd = [sys.executable, "-m", "vq3d.sample", str(tmp_path / "prior.ckpt"), "--size", *map(str, size),
           "--num-samples", str(n), "--batch-size", "2", "--seed", "21", "--temperature", "0.9", "--out", str(out),
           "--vqvae-ckpt", str(tmp_path / "vqvae.ckpt"), "--levels-from", str(tmp_path / "bottom"), "--level", "1",
           "--nrrd", str(nrrd)]
    run = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    meta = json.loads((out / "meta.json").read_text())
    assert meta == {"num_dbs": 1, "length": n, "num_embeddings": [k]}
    level = np.load(out / "level0.npy")
    assert level.shape == (n, 1) + size and level.dtype == np.int64
    assert level.min() >= 0 and level.max() < k
    for i in range(n):
        vol, hdr = read_nrrd(str(nrrd / f"sample{i}.nrrd"))
        assert vol.shape == (32, 32, 32) and hdr["type"] == "longlong"
    # the same samples in this process: the seed and the global sample index fix them
    dev = torch.device("cuda:0")
    m = load_from_checkpoint(PS.PixelSNAIL, str(tmp_path / "prior.ckpt")).to(dev).eval()
    here = torch.cat([sample_codes(m, size, 2, 0.9, 21, 0), sample_codes(m, size, 1, 0.9, 21, 2)]).cpu().numpy()
    assert np.array_equal(level[:, 0], here)
    assert os.path.getsize(out / "level0.npy") < 4096
