"""Sampling codes from a trained PixelSNAIL or PixelCNN prior, the counterpart of the reference's
`PixelSNAIL.sample` (pixel_model/pixelsnail.py:219-272), `PixelCNN.sample` (pixelcnn.py:213-287) and
pixel_model/sample_embeddings.py.

    python -m vq3d.sample PRIOR_CKPT --size d h w --num-samples N [--batch-size B] [--temperature T]
        [--seed S] --out DIR [--vqvae-ckpt CKPT --levels-from DIR... --nrrd DIR]
        [--use-model pixelsnail|pixelcnn] [--condition-from DIR [--condition-level J]]

A conditioned PixelCNN (the lower levels of a hierarchy, generated top-down) takes the codes of the level
above from --condition-from; its layers' condition projections are computed once per batch on the full grid
and cropped for every prefix.

The reference fills a (b, K, d, h, w) tensor position by position in raster order (last axis
fastest), runs its whole forward on the crop of everything visited so far and draws
`F.gumbel_softmax(logits_at_position, tau, hard=True)`.  What is computed here, for sample b of a
(d, h, w) grid and raster index p:

1. x is the one-hot of the codes drawn so far in the model's compute dtype, zero where unvisited;
2. hid = `PixelSNAIL.hidden` (everything before parse_output, eval mode) of the slab prefix
   x[:, :, :s + 1], s = p // (h w), with the first s + 1 slabs of the full-size background -- the
   model is causal and the prefix keeps raster order, so row p is that of a forward on the whole
   partly filled volume;
3. logit[k] = bias[k] + sum_c hid[b, p, c] W[k, c] in fp32 (16-bit hid: W rounded to that format);
4. code = argmax_k (logit[k] / T + g_k), first index on a tie, g_k = -log(-log(u_k)) from a
   counter-based hash of (seed, sample_base + b, p, k); T = 0: the plain argmax;
5. codes[b, p] = code and x[b, p, :] becomes its one-hot.

Steps 3-5 are one launch of csrc/sample.hip (vq3d_prior_sample_step, every sample of the batch) on
GPU tensors; the prefix forward is the model's own, already tested, eval forward: no activation
caches, no second implementation of the network.  `temperature` is a real temperature: code ~
softmax(logit / T).  The reference's `tau` is not -- F.gumbel_softmax divides logits and noise
together, (logit + g) / tau, so its hard sample is argmax(logit + g) for every tau > 0 -- and T = 1
is the reference's distribution at any tau.

CPU tensors take the same definition in numpy / torch (`sample_step_reference`, written from the
definition and not from the HIP source: the tests hold the kernel to it); the network itself has
no CPU path, so a CPU run needs an injected `hidden_fn`.
"""
import json
import os
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

CL = torch.channels_last_3d
K_MIN, K_MAX, C_MAX = 8, 1024, 1024
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------ the definition, on the host
def _u32(v):
    return np.asarray(v, dtype=np.uint64) & _M32


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def _mix32(x):
    """the lowbias32 finisher on uint32 values held in uint64 arrays"""
    x = x ^ (x >> np.uint64(16))
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> np.uint64(15))
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> np.uint64(16))


def gumbel_hash(seed, sample, p, k):
    """The 32-bit hash of (seed, global sample index, raster index, code index): numpy broadcasting
    over `sample` and `k`; seed, sample and p are taken modulo 2^64."""
    seed, p = int(seed) % 2 ** 64, int(p) % 2 ** 64
    sample = np.asarray([int(v) % 2 ** 64 for v in np.asarray(sample, dtype=object).reshape(-1)],
                        dtype=np.uint64).reshape(np.shape(sample))
    h0 = _mix32(_u32(seed & 0xFFFFFFFF) ^ _mul32(_u32(seed >> 32), 0x9E3779B1)
                ^ _mul32(sample & _M32, 0xC2B2AE3D) ^ _mul32(sample >> np.uint64(32), 0x165667B1))
    h1 = _mix32(h0 ^ _mul32(_u32(p & 0xFFFFFFFF), 0x85EBCA77) ^ _mul32(_u32(p >> 32), 0x9E3779B1))
    return _mix32(h1 ^ _mul32(_u32(k), 0x27D4EB2F)).astype(np.uint32)


def uniform_from_hash(h, dtype=np.float32):
    """u = (float(hash >> 9) + 0.5) 2^-23: strictly inside (0, 1) and exact in fp32"""
    return (np.asarray(h >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)


def perturbed_scores(logits, temperature, seed, sample_base, p, dtype=np.float32):
    """logit / T + g for a (b, K) array of logit rows of samples sample_base .. sample_base + b - 1
    at raster index p, in `dtype` arithmetic; T = 0: the logits themselves"""
    lg = np.asarray(logits).astype(dtype)
    if temperature == 0:
        return lg
    b, k = lg.shape
    h = gumbel_hash(seed, (int(sample_base) + np.arange(b, dtype=object)).reshape(b, 1), p, np.arange(k).reshape(1, k))
    u = uniform_from_hash(h, dtype)
    return lg / dtype(temperature) + -np.log(-np.log(u))


def draw_codes(logits, temperature, seed, sample_base, p):
    """the codes (b,) drawn from fp32 logit rows (b, K): the first index of the largest score"""
    return np.argmax(perturbed_scores(logits, temperature, seed, sample_base, p), axis=1).astype(np.int64)


def head_logits(hid_rows, weight, bias):
    """step 3 for (b, c) hidden rows: fp32 logits (b, K); 16-bit rows round the weight to their format"""
    w = weight.reshape(weight.shape[0], -1)
    if hid_rows.dtype != torch.float32:
        w = w.to(hid_rows.dtype)
    return bias.float() + hid_rows.float() @ w.float().t()


def _check_step(hidden, weight, bias, onehot, codes, logits_out, temperature):
    b, c = hidden.shape[:2]
    k = onehot.shape[1]
    if not (K_MIN <= k <= K_MAX):
        raise ValueError(f"{K_MIN} <= K <= {K_MAX}, got {k}")
    if c % 8 or not 0 < c <= C_MAX:
        raise ValueError(f"the hidden width must be a multiple of 8, at most {C_MAX}, got {c}")
    if (weight.numel() != k * c or bias.numel() != k or onehot.shape[0] != b
            or tuple(codes.shape) != (b, onehot[0, 0].numel())
            or (logits_out is not None and tuple(logits_out.shape) != (b, k))):
        raise ValueError("hidden, weight, bias, onehot, codes and logits_out do not fit together")
    if len({t.device for t in (hidden, weight, bias, onehot, codes)}) != 1:
        raise ValueError("every tensor must be on one device")
    if not (temperature >= 0 and temperature < float("inf")):
        raise ValueError(f"temperature must be finite and not negative (0: argmax), got {temperature}")
    if tuple(hidden.shape[3:]) != tuple(onehot.shape[3:]) or hidden.shape[2] > onehot.shape[2]:
        raise ValueError(f"a {tuple(hidden.shape[2:])} hidden is no slab prefix of a {tuple(onehot.shape[2:])} grid")


def sample_step_reference(hidden, weight, bias, pos, temperature, seed, sample_base, onehot, codes, logits_out=None):
    """Steps 3-5 on CPU tensors, in place, with the kernel's arguments: hidden (b, c, d', h, w) and
    onehot (b, K, d, h, w) channels-last, codes (b, d h w), pos and seed 0-d integer tensors."""
    b, c = hidden.shape[:2]
    k = onehot.shape[1]
    p = int(pos)
    npos, hpos = onehot[0, 0].numel(), hidden[0, 0].numel()
    if not 0 <= p < min(npos, hpos):
        return
    rows = hidden.permute(0, 2, 3, 4, 1).reshape(b, hpos, c)[:, p]
    lg = head_logits(rows, weight, bias)
    code = torch.from_numpy(draw_codes(lg.numpy(), float(temperature), int(seed), int(sample_base), p))
    codes[:, p] = code
    onehot.permute(0, 2, 3, 4, 1).reshape(b, npos, k)[:, p] = torch.nn.functional.one_hot(code, k).to(onehot.dtype)
    if logits_out is not None:
        logits_out.copy_(lg)


def sample_step_kernel(hidden, weight, bias, pos, temperature, seed, sample_base, onehot, codes, logits_out=None):
    """The C-ABI call (GPU tensors, in place, on the current stream)."""
    from . import _lib as L
    b, c = hidden.shape[:2]
    L.call("vq3d_prior_sample_step", L.dtype_code(hidden), L.ptr(hidden), hidden[0, 0].numel(), c, L.ptr(weight),
           L.ptr(bias), onehot.shape[1], L.ptr(pos), float(temperature), L.ptr(seed), int(sample_base),
           L.dtype_code(onehot), L.ptr(onehot), L.ptr(codes), onehot[0, 0].numel(), b, L.ptr(logits_out), L.stream())


def sample_step(hidden, weight, bias, pos, temperature, seed, sample_base, onehot, codes, logits_out=None):
    """Head, draw and writes of raster position *pos for every sample of the batch (steps 3-5), in
    place: hidden (b, c, d', h, w) is the prefix's `PixelSNAIL.hidden`, onehot (b, K, d, h, w) the
    sampler's input, both channels-last; weight (K, c, ...) and bias (K,) are parse_output's fp32
    parameters; pos (int64) and seed (int64 bits of the uint64 seed) are 0-d tensors on the data's
    device, read and never written; codes (b, d h w) int64; logits_out (b, K) fp32 or None."""
    _check_step(hidden, weight, bias, onehot, codes, logits_out, temperature)
    for t, dt in ((weight, torch.float32), (bias, torch.float32), (pos, torch.int64), (seed, torch.int64),
                  (codes, torch.int64)) + (() if logits_out is None else ((logits_out, torch.float32),)):
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"expected a contiguous {dt} tensor, got {t.dtype}")
    if not (hidden.is_contiguous(memory_format=CL) and onehot.is_contiguous(memory_format=CL)):
        raise ValueError("hidden and onehot must be channels-last")
    args = (hidden, weight, bias, pos, float(temperature), seed, int(sample_base), onehot, codes, logits_out)
    if not hidden.is_cuda:
        return sample_step_reference(*args)
    from . import functional as Fn
    if Fn.binding() == "library":
        from . import library  # noqa: F401  (registers the operator)
        return torch.ops.vq3d.prior_sample_step(*args)
    return sample_step_kernel(*args)


# ------------------------------------------------------------------ the driver
def _seed_bits(seed):
    """the uint64 seed as the int64 a torch scalar holds"""
    s = int(seed) % 2 ** 64
    return s - 2 ** 64 if s >= 2 ** 63 else s


@torch.no_grad()
def sample_codes(model, size, batch_size=1, temperature=1.0, seed=0, sample_base=0, return_logits=False,
                 graphs=False, hidden_fn=None, condition=None):
    """Draw `batch_size` code volumes of `size` = (d, h, w) from the prior `model` (in eval mode), in
    raster order: int64 (b, d, h, w) codes on the model's device; with return_logits also the fp32
    (b, K, d, h, w) logit rows each draw actually used.

    temperature T: code ~ softmax(logits / T); 0: argmax; 1: the reference's distribution at any of its
    `tau`.  Sample i of the batch draws its noise as global sample sample_base + i of `seed`, so
    batches with consecutive bases continue one stream of samples whatever the batch size.
    Eager: one prefix forward and one kernel launch per position.  graphs=True: one captured HIP graph
    per slab count (prefix forward, kernel, pos += 1 on a single stream, lanes off), replayed h w times.
    No host synchronisation inside the loop.  hidden_fn(prefix_onehot, full_dims) replaces
    `model.hidden` (tests; CPU models, whose network has no CPU path).

    condition: int64 (b, cd, ch, cw) codes of the level above, for a conditioned prior (vq3d.pixelcnn):
    `model.condition_cache` -- every layer's full-grid condition projection -- is computed once and
    passed to `hidden` for every prefix, which crops it; an injected hidden_fn is called as
    hidden_fn(prefix_onehot, full_dims, condition=condition) instead."""
    if model.training:
        raise RuntimeError("sample_codes needs model.eval(): dropout would change the conditional distributions")
    d, h, w = (int(v) for v in size)
    if min(d, h, w) < 1 or batch_size < 1:
        raise ValueError(f"bad size {tuple(size)} or batch size {batch_size}")
    weight, bias = model.parse_output.weight.detach(), model.parse_output.bias.detach()
    dev, k = weight.device, weight.shape[0]
    b, hw, npos, dims = int(batch_size), h * w, d * h * w, (d, h, w)
    if condition is None:
        if getattr(model, "condition_dim", 0):
            raise ValueError("this prior is conditioned: pass `condition`, the codes of the level above")
        hidden = model.hidden if hidden_fn is None else hidden_fn
    else:
        if (not torch.is_tensor(condition) or condition.dtype != torch.int64 or condition.dim() != 4
                or condition.shape[0] != b):
            raise ValueError(f"condition must be an int64 ({b}, cd, ch, cw) tensor")
        if hidden_fn is not None:
            def hidden(prefix, full_dims):
                return hidden_fn(prefix, full_dims, condition=condition)
        else:
            cache = model.condition_cache(condition.to(dev), dims)

            def hidden(prefix, full_dims):
                return model.hidden(prefix, full_dims, condition_cache=cache)
    x = torch.zeros((b, k, d, h, w), dtype=model.compute_dtype, device=dev).contiguous(memory_format=CL)
    codes = torch.zeros((b, npos), dtype=torch.int64, device=dev)
    pos = torch.zeros((), dtype=torch.int64, device=dev)
    seed_t = torch.tensor(_seed_bits(seed), dtype=torch.int64, device=dev)
    row = torch.empty((b, k), dtype=torch.float32, device=dev) if return_logits else None
    rows = torch.empty((b, npos, k), dtype=torch.float32, device=dev) if return_logits else None

    def step(s):
        hid = hidden(x[:, :, :s + 1], dims)
        hid = hid if hid.is_contiguous(memory_format=CL) else hid.contiguous(memory_format=CL)
        sample_step(hid, weight, bias, pos, temperature, seed_t, sample_base, x, codes, row)
        pos.add_(1)

    if graphs and not dev.type == "cuda":
        raise ValueError("graphs=True replays HIP graphs: the model must be on the GPU")
    replay = _capture(step, d, pos) if graphs else step
    for s in range(d):
        for q in range(hw):
            replay(s)
            if rows is not None:
                rows[:, s * hw + q] = row
    out = codes.view(b, d, h, w)
    return (out, rows.view(b, d, h, w, k).permute(0, 4, 1, 2, 3)) if return_logits else out


def _capture(step, d, pos):
    """One HIP graph per slab count s + 1 = 1 .. d of step(s), captured on the current stream with the
    PixelSNAIL lanes off (one stream, no parallel branches in the graph); returns replay(s).  Each
    slab count runs once eagerly first (lazy initialisations must not happen inside a capture) with
    pos = -1, at which the kernel writes nothing, so the warm-up leaves no trace in the state."""
    from . import pixelsnail as PS
    lanes = PS.lanes_mode()
    PS.set_lanes(False)
    try:
        for s in range(d):
            pos.fill_(-1)
            step(s)
        graphs, pool = [], torch.cuda.graph_pool_handle()
        for s in range(d):
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                step(s)
            graphs.append(g)
        pos.zero_()
    finally:
        PS.set_lanes(lanes)
    return lambda s: graphs[s].replay()


# ------------------------------------------------------------------ command line
def build_parser():
    parser = ArgumentParser(description="sample code volumes from a PixelSNAIL or PixelCNN prior checkpoint")
    parser.add_argument("prior_ckpt", type=Path)
    parser.add_argument("--use-model", choices=("pixelsnail", "pixelcnn"), default="pixelsnail",
                        help="the model class of the checkpoint")
    parser.add_argument("--condition-from", type=Path, default=None,
                        help="code directory holding the level above (a conditioned PixelCNN's condition); sample i "
                             "takes row i (modulo its length)")
    parser.add_argument("--condition-level", type=int, default=0,
                        help="which level of --condition-from is the condition")
    parser.add_argument("--size", type=int, nargs=3, required=True, metavar=("D", "H", "W"),
                        help="the code grid, in the axis order of the codes the prior was trained on")
    parser.add_argument("--num-samples", type=int, required=True)
    parser.add_argument("--batch-size", type=int, default=1)
    parser.add_argument("--temperature", type=float, default=1.0,
                        help="code ~ softmax(logits / T); 0: argmax; 1: the reference's sampler at any tau")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--dtype", choices=("bf16", "fp16", "fp32"), default="bf16", help="compute dtype of the prior")
    parser.add_argument("--graphs", action="store_true", help="replay one captured HIP graph per slab count")
    parser.add_argument("--out", type=Path, required=True, help="code directory to write (meta.json, level0.npy)")
    parser.add_argument("--vqvae-ckpt", type=Path, default=None, help="decode the samples with this VQ-VAE")
    parser.add_argument("--levels-from", type=Path, nargs="*", default=[],
                        help="code directories holding the model's other levels, bottom -> top; sample i takes "
                             "row i (modulo their length) of each")
    parser.add_argument("--level", type=int, default=0,
                        help="where the sampled level sits among the decoder's levels (0: bottom)")
    parser.add_argument("--nrrd", type=Path, default=None, help="directory for the decoded sample{i}.nrrd volumes")
    return parser


def parse_arguments(argv=None):
    return build_parser().parse_args(argv)


def _other_levels(dirs):
    levels = []
    for root in dirs:
        with open(os.path.join(root, "meta.json")) as f:
            n = int(json.load(f)["num_dbs"])
        levels += [np.load(os.path.join(root, f"level{j}.npy"), mmap_mode="r") for j in range(n)]
    return levels


def decode_samples(args, sampled, dev):
    """decode_codes + write_nrrd of every sample: the sampled level at position --level among the
    levels of --levels-from"""
    from .checkpoint import load_from_checkpoint
    from .decode import decode_codes, write_nrrd
    from .model import VQVAE
    vqvae = load_from_checkpoint(VQVAE, str(args.vqvae_ckpt)).to(dev)
    others = _other_levels(args.levels_from)
    if not 0 <= args.level <= len(others):
        raise ValueError(f"--level {args.level} with {len(others)} other levels")
    args.nrrd.mkdir(parents=True, exist_ok=True)
    for i in range(sampled.shape[0]):
        levels = [np.array(lv[i % lv.shape[0]]) for lv in others]
        levels.insert(args.level, sampled[i])
        write_nrrd(str(args.nrrd / f"sample{i}.nrrd"), decode_codes(vqvae, levels).cpu().numpy())


def main(args):
    if not torch.cuda.is_available():
        raise RuntimeError("vq3d.sample runs the prior on the HIP path: a GPU is required")
    if (args.vqvae_ckpt is None) != (args.nrrd is None):
        raise ValueError("--vqvae-ckpt and --nrrd go together")
    from .checkpoint import load_from_checkpoint
    from .extract import CodeStore
    if getattr(args, "use_model", "pixelsnail") == "pixelcnn":
        from .pixelcnn import PixelCNN as Model
    else:
        from .pixelsnail import PixelSNAIL as Model
    dev = torch.device("cuda", torch.cuda.current_device())
    model = load_from_checkpoint(Model, str(args.prior_ckpt)).to(dev)
    conditioned = bool(getattr(model, "condition_dim", 0))
    cond_dir = getattr(args, "condition_from", None)
    if conditioned != (cond_dir is not None):
        raise ValueError("--condition-from is required exactly when the prior is conditioned "
                         f"(this checkpoint's condition_dim is {getattr(model, 'condition_dim', 0)})")
    cond_rows = None
    if conditioned:
        cond_rows = np.load(os.path.join(str(cond_dir), f"level{args.condition_level}.npy"), mmap_mode="r")
    model.compute_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    model.eval()
    n, size = args.num_samples, tuple(args.size)
    sampled = np.empty((n, 1) + size, dtype=np.int64)
    with CodeStore(str(args.out), [model.input_dim], n) as store:
        for base in range(0, n, args.batch_size):
            bs = min(args.batch_size, n - base)
            cond = None
            if cond_rows is not None:
                rows = np.stack([np.array(cond_rows[(base + i) % cond_rows.shape[0]]) for i in range(bs)])
                cond = torch.from_numpy(rows.reshape((bs,) + rows.shape[-3:]).astype(np.int64)).to(dev)
            c = sample_codes(model, size, bs, args.temperature, args.seed, base, graphs=args.graphs,
                             condition=cond).cpu().numpy()
            for i in range(bs):
                sampled[base + i, 0] = c[i]
                store.put(base + i, [sampled[base + i]])
    if args.vqvae_ckpt is not None:
        decode_samples(args, sampled, dev)
    return sampled


def cli(argv=None):
    main(parse_arguments(argv))
    return 0


if __name__ == "__main__":
    sys.exit(cli())
