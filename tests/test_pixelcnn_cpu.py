"""No GPU: the definition of the conditioned PixelCNN's condition embedding
(vq3d.cond_embed.cond_embed_reference) against the reference's chain one-hot -> trilinear interpolation ->
1x1x1 conv in torch and against the reference's own outputs (tests/golden/pcnn_cond_*.npz); the PixelCNN's
module tree, seeded init and argument parsing against the reference's; the refused variants; the training
entry's parser; the sampler's condition plumbing; the new operators' fakes; the entries' size checks.

Tolerances of the definition: integer grid ratios 1e-12 (float64 against float64); other ratios
4e-6 * sum |terms|, the fp32 rounding of the source index the definition (and ATen's fp32 kernel) makes and a
float64 F.interpolate does not -- about 3x the 1.2e-6 measured on this chain at values of order 1.
"""
import ctypes
from collections import deque

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden

GRIDS = [((2, 3, 1), (8, 6, 5)), ((1, 1, 1), (2, 3, 4)), ((3, 3, 3), (3, 3, 3)), ((3, 5, 2), (7, 9, 3)),
         ((5, 4, 3), (3, 4, 7))]
INTEGER = {GRIDS[0], GRIDS[1], GRIDS[2]}


def _chain(codes, w, be, out, lam=None, index=None):
    """(e, sum |terms|) of the reference's chain in float64 torch (pixelcnn.py:116-128, :310)"""
    kc = w.shape[1]
    ok = (codes >= 0) & (codes < kc)
    oh = F.one_hot(codes.clamp(0, kc - 1), kc).double() * ok.unsqueeze(-1)
    it = F.interpolate(oh.permute(0, 4, 1, 2, 3), size=out, mode="trilinear")
    if lam is not None:
        it = lam * it + (1 - lam) * it[index]
    m = w.shape[0]
    return F.conv3d(it, w.view(m, kc, 1, 1, 1), be), F.conv3d(it, w.abs().view(m, kc, 1, 1, 1), be.abs())


def _case(cin, b=3, kc=8, m=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, kc, (b,) + cin, generator=g)
    w = torch.randn((m, kc), generator=g, dtype=torch.float64)
    be = torch.randn((m,), generator=g, dtype=torch.float64)
    return codes, w, be


def _close(e, ref, terms, grid):
    err = (e - ref).abs()
    if grid in INTEGER:
        assert float(err.max()) <= 1e-12
    else:
        assert bool((err <= 4e-6 * terms).all()), float((err / terms).max())


@pytest.mark.parametrize("cin,out", GRIDS)
def test_reference_equals_the_torch_chain(cin, out):
    from vq3d.cond_embed import cond_embed_reference
    codes, w, be = _case(cin)
    ref, terms = _chain(codes, w, be, out)
    e = cond_embed_reference(codes, w, be, out)
    assert e.dtype == torch.float64 and tuple(e.shape) == (3, 8) + out
    _close(e, ref, terms, (cin, out))


@pytest.mark.parametrize("cin,out", GRIDS)
def test_reference_mixup_prefix_and_foreign_codes(cin, out):
    from vq3d.cond_embed import cond_embed_reference
    codes, w, be = _case(cin, seed=1)
    lam, index = torch.tensor(0.3, dtype=torch.float32), torch.tensor([1, 1, 0])  # not a permutation
    ref, terms = _chain(codes, w, be, out, float(lam), index)
    _close(cond_embed_reference(codes, w, be, out, lam, index), ref, terms, (cin, out))
    # a slab prefix is the crop of the full grid's e, never an interpolation to the smaller grid
    for d_out in range(1, out[0] + 1):
        e = cond_embed_reference(codes, w, be, out, lam, index, d_out=d_out)
        _close(e, ref[:, :, :d_out], terms[:, :, :d_out], (cin, out))
    # codes -1 and Kc contribute nothing
    bad = codes.clone()
    bad.view(-1)[0::3] = -1
    bad.view(-1)[1::3] = w.shape[1]
    ref, terms = _chain(bad, w, be, out)
    _close(cond_embed_reference(bad, w, be, out), ref, terms, (cin, out))
    gone = torch.full_like(codes, -1)
    assert torch.equal(cond_embed_reference(gone, w, be, out), be.view(1, -1, 1, 1, 1).expand(3, -1, *out))


@pytest.mark.parametrize("name", ["pcnn_cond_int", "pcnn_cond_frac"])
def test_reference_equals_the_golden(name):
    """against the reference's own fp32 embed_condition(F.interpolate(idx_to_one_hot(...)))"""
    from vq3d.cond_embed import cond_embed_reference
    d = golden(name)
    w, be = torch.tensor(d["weight"]).double().view(16, 8), torch.tensor(d["bias"]).double()
    codes, dims = torch.tensor(d["codes"]), tuple(int(v) for v in d["dims"])
    e = cond_embed_reference(codes, w, be, dims)
    _, terms = _chain(codes, w, be, dims)  # each element's own sum |terms|, as for the chain above
    err = (e - torch.tensor(d["e"]).double()).abs()
    assert bool((err <= 4e-6 * terms).all()), float((err / terms).max())


def test_reference_gradcheck():
    from vq3d.cond_embed import cond_embed_reference
    codes, w, be = _case((3, 5, 2), b=2)
    w.requires_grad_(True)
    be.requires_grad_(True)
    lam, index = torch.tensor(0.25), torch.tensor([1, 0])
    assert torch.autograd.gradcheck(lambda ww, bb: cond_embed_reference(codes, ww, bb, (4, 6, 3), lam, index), (w, be))


def test_cpu_tensors_take_the_definition():
    from vq3d.cond_embed import cond_embed, cond_embed_reference
    codes, w, be = _case((2, 3, 1))
    e = cond_embed(codes, w.float(), be.float(), (8, 6, 5), dtype=torch.bfloat16)
    assert e.dtype == torch.bfloat16 and e.is_contiguous(memory_format=torch.channels_last_3d)
    ref = cond_embed_reference(codes, w.float().bfloat16(), be.float(), (8, 6, 5))
    assert torch.equal(e, ref.to(torch.bfloat16))


# ------------------------------------------------------------------ the model
def _args(**kw):
    from vq3d import pixelcnn as PC
    return PC.default_args(**{**dict(num_embeddings=[16, 8], model_dim=32, num_resblocks=2, dropout_prob=0.0,
                                     use_pre_activation=True, use_conditioning=True, mixup_alpha=0, lr=1e-3), **kw})


@pytest.mark.parametrize("name,seed,kw", [
    ("pcnn_init_cond", 3, {}),
    ("pcnn_init_plain", 4, dict(model_dim=16, use_conditioning=False, num_embeddings=[16, 0]))])
def test_module_tree_and_seeded_init(name, seed, kw):
    from vq3d.pixelcnn import PixelCNN
    d = golden(name)
    torch.manual_seed(seed)
    m = PixelCNN(_args(**kw))
    sd = m.state_dict()
    assert set(sd) == {k[2:] for k in d.files}
    for k in d.files:
        assert tuple(sd[k[2:]].shape) == d[k].shape, k
        assert torch.equal(sd[k[2:]], torch.tensor(d[k])), k
    assert [n for n, _ in m.named_children()] == (
        ["parse_input", "embed_condition", "layers", "parse_output"] if m.use_conditioning
        else ["parse_input", "layers", "parse_output"])
    assert len(m.layers) == 3
    if m.use_conditioning:
        assert all(f"layers.{i}.condition.{p}" in sd for i in range(3) for p in ("weight", "bias"))
        assert tuple(sd["embed_condition.weight"].shape) == (32, 8, 1, 1, 1)
        assert tuple(sd["layers.1.condition.weight"].shape) == (8, 32, 1, 1, 1)
    else:
        assert m.embed_condition is None and m.condition_dim == 0 and not any("condition" in k for k in sd)
    opt = m.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["amsgrad"] and opt.defaults["lr"] == 1e-3


def test_argparse_defaults_are_the_references():
    from argparse import ArgumentParser
    from vq3d import pixelcnn as PC
    a = PC.PixelCNN.add_model_specific_args(ArgumentParser()).parse_args([])
    # pixel_model/pixelcnn.py:190-210
    want = dict(model_dim=32, kernel_size=3, num_resblocks=18, dropout_prob=0.5, use_pre_activation=False,
                use_gated_block=False, bottleneck_divisor=4, use_conditioning=False, use_concat_activation=False,
                mixup_alpha=1, use_mixup_batch_hack=False, metric=None, lr=1e-5)
    assert vars(a) == want
    d = vars(PC.default_args())
    assert {k: d[k] for k in want if k != "metric"} == {k: v for k, v in want.items() if k != "metric"}


def test_refused_variants_say_why():
    from vq3d import pixelsnail as PS
    from vq3d.pixelcnn import PixelCNN
    with pytest.raises(NotImplementedError, match=r"layers\.py:610"):
        PixelCNN(_args(use_pre_activation=False))
    with pytest.raises(NotImplementedError, match="concat_activation"):
        PixelCNN(_args(use_concat_activation=True))
    a = _args(use_gated_block=True)
    assert PixelCNN(a).use_gated_block is False and a.use_gated_block is False  # forced by the reference itself
    with pytest.raises(ValueError):
        PixelCNN(_args(metric="mse"))
    with pytest.raises(NotImplementedError):  # PixelSNAIL conditioning stays refused
        PS.PixelSNAIL(PS.default_args(use_conditioning=True, num_embeddings=[16, 8]))
    m = PixelCNN(_args())
    x = torch.zeros((1, 16, 2, 2, 2))
    with pytest.raises(ValueError, match="condition"):
        m.hidden(x)
    with pytest.raises(TypeError, match="int64"):
        m.hidden(x, condition=torch.zeros((1, 8, 2, 2, 2)))
    with pytest.raises(ValueError, match="slab prefix"):
        m.hidden(x, full_dims=(1, 2, 2), condition=torch.zeros((1, 1, 1, 1), dtype=torch.int64))
    plain = PixelCNN(_args(use_conditioning=False))
    with pytest.raises(ValueError, match="without conditioning"):
        plain.hidden(x, condition=torch.zeros((1, 1, 1, 1), dtype=torch.int64))


def test_train_pixelcnn_parser():
    from vq3d import train_pixelcnn as TC
    a = TC.parse_arguments(["codes", "1", "--metric", "cross_entropy", "--use-pre-activation", "True",
                            "--use-conditioning", "True", "--batch-size", "2", "--model-dim", "256",
                            "--num-resblocks", "45"])
    assert (a.level, a.batch_size, a.model_dim, a.num_resblocks, a.use_model) == (1, 2, 256, 45, "pixelcnn")
    assert a.use_conditioning is True and a.use_pre_activation is True and a.mixup_alpha == 1
    assert a.compute_dtype == "bf16" and isinstance(a.dataset_path, str)
    # the trainer defaults of pixel_model/train.py:28-44, as vq3d.train_prior's
    assert (a.gpus, a.accelerator, a.precision, a.val_check_interval, a.max_epochs) == ("-1", "ddp", 16, 0.5, 50000)
    d = TC.parse_arguments(["codes", "0"])
    assert d.use_pre_activation is False and d.use_conditioning is False and d.num_resblocks == 18


def test_train_prior_still_refuses_pixelcnn():
    from vq3d import train_prior as TP
    for argv in (["codes", "0", "--use-model", "pixelcnn"], ["codes", "0"]):
        with pytest.raises(NotImplementedError, match="DESIGN.md §8") as e:
            TP.parse_arguments(argv)
        assert "vq3d.train_pixelcnn" in str(e.value)


def test_batches_carry_the_condition():
    from vq3d import train_prior as TP

    class M:
        use_conditioning = True
    batch = [torch.zeros((2, 1, 4, 4, 4), dtype=torch.int64), torch.ones((2, 1, 2, 2, 2), dtype=torch.int64)]
    c = TP._condition(batch, torch.device("cpu"), M())
    assert tuple(c.shape) == (2, 2, 2, 2) and c.dtype == torch.int64
    assert TP._condition(batch[:1], torch.device("cpu"), M()) is None
    M.use_conditioning = False
    assert TP._condition(batch, torch.device("cpu"), M()) is None
    assert TP._cond_kw(None) == {} and TP._cond_kw(c) == {"condition": c}


# ------------------------------------------------------------------ the sampler
class _Head(torch.nn.Module):
    def __init__(self, k, c, condition_dim):
        super().__init__()
        self.parse_output = torch.nn.Conv3d(c, k, 1)
        self.compute_dtype = torch.float32
        self.condition_dim = condition_dim


def test_sample_codes_hands_the_condition_to_hidden():
    from vq3d.sample import sample_codes
    torch.manual_seed(0)
    k, c = 8, 8
    model = _Head(k, c, condition_dim=4).eval()
    cond = torch.randint(0, 4, (2, 1, 2, 1))
    seen = []

    def hidden_fn(prefix, dims, condition=None):
        seen.append((tuple(prefix.shape), tuple(dims), condition))
        # a hidden that depends on the condition: the draws must follow it
        h = torch.zeros((prefix.shape[0], c) + tuple(prefix.shape[2:]))
        h[:, 0] = 50.0
        h[:, 1:] = 0.0
        return (h * (1 + condition.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1, 1))).contiguous(
            memory_format=torch.channels_last_3d)
    out = sample_codes(model, (2, 2, 3), 2, temperature=0.0, hidden_fn=hidden_fn, condition=cond)
    assert tuple(out.shape) == (2, 2, 2, 3) and len(seen) == 12
    assert all(s[2] is cond and s[1] == (2, 2, 3) for s in seen)
    assert seen[0][0] == (2, k, 1, 2, 3) and seen[-1][0] == (2, k, 2, 2, 3)
    with pytest.raises(ValueError, match="conditioned"):
        sample_codes(model, (2, 2, 3), 2, hidden_fn=hidden_fn)
    with pytest.raises(ValueError, match="int64"):
        sample_codes(model, (2, 2, 3), 2, hidden_fn=hidden_fn, condition=cond[:1])
    # an unconditioned model: hidden_fn keeps its two-argument form
    plain = _Head(k, c, condition_dim=0).eval()
    out = sample_codes(plain, (1, 2, 2), 1, temperature=0.0,
                       hidden_fn=lambda p, dims: torch.zeros((1, c) + tuple(p.shape[2:])).contiguous(
                           memory_format=torch.channels_last_3d))
    assert tuple(out.shape) == (1, 1, 2, 2)


def test_sample_cli_flags():
    from vq3d import sample as S
    a = S.parse_arguments(["p.ckpt", "--size", "2", "2", "2", "--num-samples", "1", "--out", "o"])
    assert a.use_model == "pixelsnail" and a.condition_from is None and a.condition_level == 0
    a = S.parse_arguments(["p.ckpt", "--size", "2", "2", "2", "--num-samples", "1", "--out", "o", "--use-model",
                           "pixelcnn", "--condition-from", "up", "--condition-level", "1"])
    assert a.use_model == "pixelcnn" and str(a.condition_from) == "up" and a.condition_level == 1


def test_block_forward_pops_the_condition_cache(monkeypatch):
    """the block's module forward prefers condition_cache and pops it (layers.py:446-452); the popped
    projection is cropped to the stack's grid"""
    from vq3d import pixelsnail as PS
    blk = PS.PreActFixupCausalResBlock(16, 16, 3, condition_dim=16, dropout_prob=0.0)
    got = {}
    monkeypatch.setattr(blk, "run", lambda stack, aux=None, cond=None: got.setdefault("cond", cond) is None or stack)
    cache = deque([torch.arange(2 * 4 * 3 * 4 * 5, dtype=torch.float32).view(2, 4, 3, 4, 5), torch.zeros(1)])
    full = cache[0]
    blk.forward(torch.zeros((3, 2, 16, 2, 4, 5)), condition_cache=cache)
    assert len(cache) == 1 and torch.equal(got["cond"], full[:, :, :2])
    assert got["cond"].is_contiguous(memory_format=torch.channels_last_3d)
    with pytest.raises(ValueError, match="no crop"):
        PS.crop_condition(full, (4, 4, 5))


# ------------------------------------------------------------------ operators and entries
def test_new_operators_have_fakes_with_the_right_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import vq3d.library as Lb
    assert {"cond_embed", "cond_embed_backward"} <= set(Lb.OPS)
    with FakeTensorMode(allow_non_fake_inputs=True):
        codes = torch.empty((3, 2, 3, 1), dtype=torch.int64, device="cuda")
        table = torch.empty((8, 72), dtype=torch.bfloat16, device="cuda")
        bias = torch.empty((72,), device="cuda")
        e = torch.ops.vq3d.cond_embed(codes, table, bias, [8, 6, 5], 4, None, None)
        assert tuple(e.shape) == (3, 72, 4, 6, 5) and e.dtype == torch.bfloat16
        assert e.is_contiguous(memory_format=torch.channels_last_3d) and e.stride() == (72 * 4 * 6 * 5, 1, 2160, 360, 72)
        dwe, dbe = torch.empty((72, 8), device="cuda"), torch.empty((72,), device="cuda")
        g = torch.empty((3, 72, 8, 6, 5), dtype=torch.bfloat16, device="cuda").contiguous(
            memory_format=torch.channels_last_3d)
        assert torch.ops.vq3d.cond_embed_backward(g, codes, 8, None, None, dwe, dbe) is None


def test_python_entry_refuses_bad_sizes_before_any_launch():
    from vq3d.cond_embed import cond_embed
    codes = torch.zeros((2, 2, 2, 2), dtype=torch.int64)
    w, b = torch.zeros((16, 8)), torch.zeros(16)
    ok = dict(codes=codes, weight=w, bias=b, dims=(4, 4, 4))
    for kw, exc, word in (
            (dict(codes=codes.int()), TypeError, "int64"), (dict(codes=codes[0]), TypeError, "int64"),
            (dict(weight=torch.zeros((16, 4)), bias=b), ValueError, "Kc"),
            (dict(weight=torch.zeros((16, 1032))), ValueError, "Kc"),
            (dict(weight=torch.zeros((12, 8)), bias=torch.zeros(12)), ValueError, "multiple of 8"),
            (dict(weight=torch.zeros((1032, 8)), bias=torch.zeros(1032)), ValueError, "1024"),
            (dict(bias=torch.zeros(8)), ValueError, "fit"), (dict(dims=(4, 4)), ValueError, "grid"),
            (dict(dims=(4, 0, 4)), ValueError, "grid"), (dict(dims=(4, 4, (1 << 20) + 1)), ValueError, "2\\^20"),
            (dict(d_out=5), ValueError, "d_out"),
            (dict(d_out=0), ValueError, "d_out"), (dict(lam=torch.tensor(0.5)), ValueError, "together"),
            (dict(lam=torch.tensor(0.5), index=torch.zeros(3, dtype=torch.int64)), TypeError, "index"),
            (dict(lam=torch.tensor(0.5, dtype=torch.float64), index=torch.zeros(2, dtype=torch.int64)), TypeError, "lam"),
            (dict(dtype=torch.float64), TypeError, "dtype")):
        with pytest.raises(exc, match=word):
            cond_embed(**{**ok, **kw})


def test_abi_limits_are_checked_on_the_host():
    """the C entries refuse what the kernels cannot run, before any launch (no GPU touched)"""
    from vq3d import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    ok = dict(dtype=L.BF16, b=1, cd=1, ch=1, cw=1, d=2, h=2, w=2, d_out=2, m=8, kc=8)
    order = ("dtype", "b", "cd", "ch", "cw", "d", "h", "w", "d_out", "m", "kc")
    for kw, word in (({"dtype": 7}, b"dtype"), ({"m": 12}, b"multiple of 8"), ({"m": 1032}, b"1024"),
                     ({"kc": 4}, b"kc"), ({"kc": 1025}, b"kc"), ({"d_out": 3}, b"d_out"), ({"d_out": 0}, b"d_out"),
                     ({"b": 0}, b"grid"), ({"cw": 0}, b"grid"), ({"h": 0}, b"grid"), ({"w": (1 << 20) + 1}, b"2^20"),
                     ({"cd": (1 << 20) + 1}, b"2^20")):
        a = dict(ok, **kw)
        rc = lib.vq3d_cond_embed_fwd(*[a[n] for n in order], p, p, p, None, None, p, None)
        assert rc != 0 and word in lib.vq3d_last_error(), (kw, lib.vq3d_last_error())
    rc = lib.vq3d_cond_embed_fwd(*[ok[n] for n in order], p, p + 2, p, None, None, p, None)
    assert rc != 0 and b"aligned" in lib.vq3d_last_error()
    rc = lib.vq3d_cond_embed_fwd(*[ok[n] for n in order], p, None, p, None, None, p, None)
    assert rc != 0 and b"null" in lib.vq3d_last_error()
    nws = lib.vq3d_cond_embed_bwd_workspace_bytes(2, 2, 3, 2, 16)
    assert nws == 2 * 12 * 16 * 4
    bo = [ok[n] for n in order if n != "d_out"]
    rc = lib.vq3d_cond_embed_bwd(*bo, p, p, None, None, p, p, p, 0, None)
    assert rc != 0 and b"workspace" in lib.vq3d_last_error()
    rc = lib.vq3d_cond_embed_bwd(*bo, p, None, None, None, p, p, p, 64, None)
    assert rc != 0 and b"null" in lib.vq3d_last_error()
    for fn, args in ((lib.vq3d_preact_add_act_fwd, (7, 8, p, p, p, p, p, None)),
                     (lib.vq3d_preact_add_act_bwd, (7, 8, p, p, p, p, p, p, p, None))):
        assert fn(*args) != 0 and b"dtype" in lib.vq3d_last_error()
    assert lib.vq3d_preact_add_act_fwd(L.BF16, 8, p, None, p, p, p, None) != 0 and b"null" in lib.vq3d_last_error()
