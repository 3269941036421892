"""The conditioned PixelCNN prior's condition embedding (reference pixel_model/pixelcnn.py:113-128, :294,
:310 with mixup's blend, train_helpers.py:48-53): embed_condition of the trilinearly interpolated one-hot of
the upper level's codes.  One-hot, interpolation and the 1x1x1 conv are linear, so nothing of the chain is
materialised: e is a trilinear blend of columns of the (M, Kc) weight.

Inputs: codes c int64 (b, cd, ch, cw) with values in [0, Kc); the lower grid dims = (D, H, W); the weight
We (M, Kc) and bias be (M,); optionally mixup's lam (fp32 scalar) and index (int64 (b,)).  Per axis
n_in -> n_out, PyTorch's align_corners=False rule in fp32:

    s = float(n_in) / float(n_out);  src = max(s (o + 0.5) - 0.5, 0)
    i0 = min(floor(src), n_in - 1);  i1 = i0 + (i0 < n_in - 1);  t1 = src - i0;  t0 = 1 - t1

and for voxel v = (z, y, x) of sample B

    e0[B, v, :] = sum over the 8 corners j of tz ty tx We[:, c[B, corner_j(v)]]
    e[B, v, :]  = be + lam e0[B, v, :] + (1 - lam) e0[index[B], v, :]          (no mixup: be + e0)

A code outside [0, Kc) contributes nothing, forward and backward (an index value outside [0, b) stands for
the sample itself).  The table entries are We rounded to the compute dtype (not rounded in fp32 runs),
weights and accumulation are fp32, the sum is rounded once.  With d_out < D the result is the first d_out
slabs of the full grid's e (a crop, never an interpolation to the smaller grid).

GPU tensors run csrc/cond_embed.hip (vq3d_cond_embed_fwd / _bwd): the forward reads a transposed (Kc, M)
table in the output's format, made here once per forward from the weight or its 16-bit flat shadow; the
backward adds dWe and dbe in fp32 straight into the parameters' gradient buffers (pixelsnail._direct), in two
launches with a fixed summation order and no atomics.  lam and index are device tensors read when the
kernels run, so a captured step replays with new draws copied into them.  `cond_embed_reference` is the
definition in float64 torch, written from the text above and not from the HIP source: the tests hold the
kernels to it.  CPU tensors take it.  Measured: forward + backward is about 5x faster than the
unfused chain at the published mid level's shape; at a bottom-like shape it is no faster (2 % slower without
mixup, 13 % slower with it: the gather of the backward), and only the memory saving holds there.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

CL = torch.channels_last_3d
K_MIN, K_MAX, M_MAX, AXIS_MAX = 8, 1024, 1024, 1 << 20


# ------------------------------------------------------------------ the definition
def axis_coefficients(n_in, n_out):
    """(i0, i1, t0, t1) numpy arrays over the n_out positions: src in fp32, the weights float64 from it"""
    s = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    src = np.maximum(s * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    assert src.dtype == np.float32
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    t1 = src.astype(np.float64) - i0
    return i0, i1, 1.0 - t1, t1


def _e0(codes, table, dims, d_out):
    """e0 (b, d_out, H, W, M) float64 from the (Kc, M) float64 table"""
    b, cd, ch, cw = codes.shape
    kc = table.shape[0]
    D, H, W = dims
    az, ay, ax = axis_coefficients(cd, D), axis_coefficients(ch, H), axis_coefficients(cw, W)
    ok = (codes >= 0) & (codes < kc)
    rows = torch.where(ok.unsqueeze(-1), table[codes.clamp(0, kc - 1)], torch.zeros((), dtype=table.dtype))
    out = torch.zeros((b, d_out, H, W, table.shape[1]), dtype=torch.float64)
    for jz in (0, 1):
        iz, tz = torch.as_tensor(az[jz][:d_out]), torch.as_tensor(az[2 + jz][:d_out])
        for jy in (0, 1):
            iy, ty = torch.as_tensor(ay[jy]), torch.as_tensor(ay[2 + jy])
            for jx in (0, 1):
                ix, tx = torch.as_tensor(ax[jx]), torch.as_tensor(ax[2 + jx])
                wgt = tz.view(-1, 1, 1) * ty.view(1, -1, 1) * tx.view(1, 1, -1)
                out += wgt.unsqueeze(-1) * rows[:, iz][:, :, iy][:, :, :, ix]
    return out


def cond_embed_reference(codes, weight, bias, dims, lam=None, index=None, d_out=None):
    """e (b, M, d_out, H, W) float64 by the definition above (weight and bias are taken as they come: round
    the weight first to model a 16-bit table).  Differentiable in weight and bias by plain autograd."""
    codes = torch.as_tensor(codes).long().cpu()
    D, H, W = (int(v) for v in dims)
    d_out = D if d_out is None else int(d_out)
    w = weight.reshape(weight.shape[0], -1).double().cpu()
    e0 = _e0(codes, w.t(), (D, H, W), d_out)
    be = bias.double().cpu()
    if lam is None or index is None:
        e = be + e0
    else:
        lam = float(lam)
        idx = torch.as_tensor(index).long().cpu()
        idx = torch.where((idx >= 0) & (idx < codes.shape[0]), idx, torch.arange(codes.shape[0]))  # foreign: itself
        e = be + np.float64(np.float32(lam)) * e0 + (1.0 - np.float64(np.float32(lam))) * e0[idx]
    return e.permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------ the C-ABI calls
def cond_embed_fwd_kernel(codes, table, bias, dims, d_out, lam=None, index=None):
    """vq3d_cond_embed_fwd on the current stream: e (b, M, d_out, H, W) channels-last in the table's dtype"""
    b, cd, ch, cw = codes.shape
    kc, m = table.shape
    D, H, W = dims
    e = torch.empty((b, m, d_out, H, W), dtype=table.dtype, device=table.device).contiguous(memory_format=CL)
    L.call("vq3d_cond_embed_fwd", L.dtype_code(table), b, cd, ch, cw, D, H, W, d_out, m, kc, L.ptr(codes), L.ptr(table),
           L.ptr(bias), L.ptr(lam), L.ptr(index), L.ptr(e), L.stream())
    return e


def cond_embed_bwd_kernel(g, codes, kc, lam, index, dwe, dbe):
    """vq3d_cond_embed_bwd on the current stream: dwe (M, Kc) and dbe (M,), fp32, are added into"""
    b, cd, ch, cw = codes.shape
    m, D, H, W = g.shape[1:]
    nws = int(L.query("vq3d_cond_embed_bwd_workspace_bytes", b, cd, ch, cw, m))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=g.device)
    L.call("vq3d_cond_embed_bwd", L.dtype_code(g), b, cd, ch, cw, D, H, W, m, kc, L.ptr(codes), L.ptr(g), L.ptr(lam),
           L.ptr(index), L.ptr(dwe), L.ptr(dbe), L.ptr(ws), ctypes.c_size_t(nws), L.stream())


def _fwd(*args):
    from . import functional as Fn
    if Fn.binding() == "library":
        from . import library  # noqa: F401  (registers the operators)
        codes, table, bias, dims, d_out, lam, index = args
        return torch.ops.vq3d.cond_embed(codes, table, bias, list(dims), d_out, lam, index)
    return cond_embed_fwd_kernel(*args)


def _bwd(*args):
    from . import functional as Fn
    if Fn.binding() == "library":
        return torch.ops.vq3d.cond_embed_backward(*args)
    return cond_embed_bwd_kernel(*args)


def make_table(weight, dtype):
    """the transposed (Kc, M) table in dtype from the (M, Kc, 1, 1, 1) weight or its 16-bit flat shadow"""
    from . import pixelsnail as PS
    w = weight.detach() if dtype == torch.float32 else PS._w16(weight.detach(), dtype)
    return w.reshape(w.shape[0], -1).t().contiguous()


class CondEmbedFn(torch.autograd.Function):
    """e of GPU codes on cond_embed.hip.  Saves the codes (and lam / index); the backward is the two
    launches of vq3d_cond_embed_bwd, the gradients added into the parameters' buffers."""

    @staticmethod
    def forward(ctx, weight, bias, codes, dims, d_out, lam, index, dtype):
        table = make_table(weight, dtype)
        e = _fwd(codes, table, bias.detach(), dims, d_out, lam, index)
        ctx.prm = (weight, bias)
        ctx.full = d_out == dims[0]
        ctx.kc = table.shape[0]
        ctx.save_for_backward(codes, lam, index)
        return e

    @staticmethod
    def backward(ctx, g):
        from . import pixelsnail as PS
        if not ctx.full:
            raise RuntimeError("cond_embed: the backward takes the gradient of the full grid (d_out == D)")
        codes, lam, index = ctx.saved_tensors
        weight, bias = ctx.prm
        g = g if g.is_contiguous(memory_format=CL) else g.contiguous(memory_format=CL)
        dw, db = PS._param_grad(weight), PS._param_grad(bias)
        _bwd(g, codes, ctx.kc, lam, index, dw.view(dw.shape[0], -1), db)
        return (None if PS._direct(weight) else dw, None if PS._direct(bias) else db, None, None, None, None, None,
                None)


def _check(codes, weight, bias, dims, lam, index, d_out):
    if codes.dim() != 4 or codes.dtype != torch.int64:
        raise TypeError("codes must be an int64 (b, cd, ch, cw) tensor")
    if len(dims) != 3 or min(int(v) for v in dims) < 1 or min(codes.shape) < 1:
        raise ValueError(f"bad grid {tuple(dims)} or codes {tuple(codes.shape)}")
    if max(max(int(v) for v in dims), max(codes.shape[1:])) > AXIS_MAX:
        raise ValueError(f"an axis of the grid {tuple(dims)} or of the codes {tuple(codes.shape)} is longer than 2^20")
    m = weight.shape[0]
    kc = weight.numel() // max(m, 1)
    if weight.numel() != m * kc or bias.numel() != m:
        raise ValueError("weight and bias do not fit together")
    if not (K_MIN <= kc <= K_MAX):
        raise ValueError(f"{K_MIN} <= Kc <= {K_MAX}, got {kc}")
    if m % 8 or not 0 < m <= M_MAX:
        raise ValueError(f"the embedding width must be a multiple of 8, at most {M_MAX}, got {m}")
    if not 1 <= d_out <= int(dims[0]):
        raise ValueError(f"d_out must be in [1, {int(dims[0])}], got {d_out}")
    if (lam is None) != (index is None):
        raise ValueError("lam and index go together")
    if lam is not None:
        if not torch.is_tensor(lam) or lam.dtype != torch.float32 or lam.numel() != 1:
            raise TypeError("lam must be a one-element fp32 tensor")
        if not torch.is_tensor(index) or index.dtype != torch.int64 or tuple(index.shape) != (codes.shape[0],):
            raise TypeError("index must be an int64 (b,) tensor")
        if lam.device != codes.device or index.device != codes.device:
            raise ValueError("lam and index must be on the codes' device")
    if weight.device != codes.device or bias.device != codes.device:
        raise ValueError("codes, weight and bias must be on one device")


def cond_embed(codes, weight, bias, dims, lam=None, index=None, d_out=None, dtype=torch.float32):
    """e (b, M, d_out, H, W) channels-last in `dtype` (fp32, bf16 or fp16): see the module doc.  weight is
    embed_condition's (M, Kc[, 1, 1, 1]) fp32 parameter, bias its (M,) one; lam / index device tensors (both
    or neither).  Differentiable in weight and bias when d_out is None or D."""
    d_out = int(dims[0]) if d_out is None else int(d_out)
    dims = tuple(int(v) for v in dims)
    _check(codes, weight, bias, dims, lam, index, d_out)
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"unsupported dtype {dtype}")
    if not codes.is_cuda:
        w = weight if dtype == torch.float32 else weight.to(dtype)
        return cond_embed_reference(codes, w, bias, dims, lam, index, d_out).to(dtype).contiguous(memory_format=CL)
    codes = codes.contiguous()
    return CondEmbedFn.apply(weight, bias, codes, dims, d_out, lam, None if index is None else index.contiguous(),
                             dtype)
