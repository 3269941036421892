"""Reconstruction-quality metrics of the reference's validation (vqvae/model.py:20-30, 70-72, 132-136
and metrics/evaluate.py): slice-wise SSIM, NMSE and PSNR.

    slice_metrics(pred, target, nvs)   every figure from one fused kernel pass (csrc/metrics.hip)
    SSIM3DSlices(...)                  the reference's module: (pred, target) -> scalar SSIM
    nmse(orig, pred), psnr(orig, pred, data_range)   the two helpers of metrics/evaluate.py:18-24

The SSIM is PL 1.2's `metrics.functional.ssim` at the arguments the reference uses -- an 11 x 11
Gaussian window of sigma 1.5, k1 = 0.01, k2 = 0.03, mean reduction -- applied to every (b, d) slice of
a (B, 1, H, W, D) volume; include/vq3d.h (vq3d_slice_metrics) writes the definition out.  Two
deliberate differences from the reference's call: the inputs are not rounded to fp16 first
(model.py:134 `.half()`), and the masking / ELU of the loss can be applied inside the pass.

GPU tensors go to the kernel.  CPU tensors take a plain-torch fp32 evaluation of the same definition
(`_slice_metrics_torch`), so the module and `vq3d.evaluate` can be used and tested without a GPU;
it is never a fallback for a GPU tensor.
"""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch import nn

from .utils import cylinder_xy_mask

KERNEL_SIZE, SIGMA = (11, 11), (1.5, 1.5)
_ACTIVATIONS = {"none": 0, "elu": 1}


class SliceMetrics(NamedTuple):
    """Device tensors: `ssim_per_slice` is (B, D), the others are scalars."""
    ssim: torch.Tensor
    ssim_per_slice: torch.Tensor
    mse: torch.Tensor
    nmse: torch.Tensor
    psnr: torch.Tensor
    data_range: torch.Tensor


def gaussian_window(dtype=torch.float32, device=None):
    """The normalised 11-tap Gaussian (sigma 1.5) whose outer product is the SSIM window."""
    i = torch.arange(KERNEL_SIZE[0], dtype=torch.float64) - KERNEL_SIZE[0] // 2
    g = torch.exp(-0.5 * (i / SIGMA[0]) ** 2)
    return (g / g.sum()).to(dtype=dtype, device=device)


def _check(pred, target, nvs, activation, data_range, k1, k2, psnr_range):
    if activation not in _ACTIVATIONS:
        raise ValueError(f"activation must be 'none' or 'elu', not {activation!r}")
    if pred.dim() != 5 or pred.shape[1] != 1:
        raise ValueError(f"slice_metrics takes (B, 1, H, W, D) volumes, got {tuple(pred.shape)}")
    if tuple(target.shape) != tuple(pred.shape):
        raise ValueError(f"target {tuple(target.shape)} must have pred's shape {tuple(pred.shape)}")
    if pred.shape[2] < KERNEL_SIZE[0] or pred.shape[3] < KERNEL_SIZE[1]:
        raise ValueError(f"H and W must be at least {KERNEL_SIZE[0]} (the SSIM window), got "
                         f"{pred.shape[2]} x {pred.shape[3]}")
    if pred.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"pred must be fp32, bf16 or fp16, not {pred.dtype}")
    if target.dtype != torch.float32:
        raise TypeError(f"target must be fp32, not {target.dtype}")
    if target.device != pred.device:
        raise ValueError("pred and target must be on one device")
    if data_range is not None and not data_range > 0:
        raise ValueError(f"data_range must be positive (None: computed from the batch), got {data_range}")
    if k1 < 0 or k2 < 0:
        raise ValueError("k1 and k2 must not be negative")
    if not psnr_range > 0:
        raise ValueError("psnr_range must be positive")
    b, d = pred.shape[0], pred.shape[4]
    if nvs is None:
        nvs = torch.full((b,), d, dtype=torch.int64, device=pred.device)
    else:
        nvs = torch.as_tensor(nvs).to(device=pred.device, dtype=torch.int64).reshape(-1)
        if nvs.numel() != b:
            raise ValueError(f"nvs must hold one slice count per batch element ({b}), got {nvs.numel()}")
    return nvs.contiguous()


def slice_metrics_kernel(pred, target, nvs, elu, cylinder, data_range, k1, k2, psnr_range):
    """The C-ABI call: (ssim_per_slice (B, D), stats (5,) = {ssim, mse, nmse, psnr, data_range_used}),
    both on pred's device; data_range <= 0 asks for the computed range."""
    from . import _lib as L
    from . import ops
    b, _, h, w, d = pred.shape
    dev = pred.device
    per_slice = torch.empty((b, d), dtype=torch.float32, device=dev)
    stats = torch.empty(5, dtype=torch.float32, device=dev)
    ws = ops.workspace(L.query("vq3d_slice_metrics_workspace_size", b, h, w, d), dev)
    L.call("vq3d_slice_metrics", L.dtype_code(pred), L.ptr(pred), L.ptr(target), L.ptr(nvs), b, h, w, d, int(elu),
           int(cylinder), float(data_range), float(k1), float(k2), float(psnr_range), L.ptr(per_slice), L.ptr(stats),
           L.ptr(ws), L.stream())
    return per_slice, stats


def _slice_metrics_torch(pred, target, nvs, elu, cylinder, data_range, k1, k2, psnr_range):
    """The same definition in plain fp32 torch (CPU tensors)."""
    b, _, h, w, d = pred.shape
    p = pred.float()
    if elu:
        p = F.elu(p)
    p = p * (torch.arange(d, device=p.device).view(1, 1, 1, 1, d) < nvs.view(b, 1, 1, 1, 1))
    t = target
    if data_range > 0:
        rng = torch.tensor(float(data_range), dtype=torch.float32, device=p.device)
    else:
        rng = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    ps, ts = (v.permute(0, 4, 1, 2, 3).reshape(b * d, 1, h, w) for v in (p, t))
    g = gaussian_window(device=p.device)
    q = torch.cat([ps, ts, ps * ps, ts * ts, ps * ts], dim=1)  # (B D, 5, H, W)
    q = F.conv2d(q, g.view(1, 1, -1, 1).repeat(5, 1, 1, 1), groups=5)
    q = F.conv2d(q, g.view(1, 1, 1, -1).repeat(5, 1, 1, 1), groups=5)
    mp, mt, epp, ett, ept = q.unbind(1)
    spp, stt, spt = epp - mp * mp, ett - mt * mt, ept - mp * mt
    smap = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    per_slice = smap.mean(dim=(1, 2)).view(b, d)
    per_slice = torch.where(rng > 0, per_slice, torch.full_like(per_slice, math.nan))
    err, ref = (p - t) ** 2, t * t
    if cylinder:
        m = cylinder_xy_mask((h, w)).to(p.device).view(1, 1, h, w, 1)
        err, ref, count = err * m, ref * m, b * d * int(m.sum())
    else:
        count = p.numel()
    sse, st2 = err.double().sum(), ref.double().sum()
    mse = sse / count
    stats = torch.stack([per_slice.double().mean(), mse, sse / st2, 10 * torch.log10(psnr_range ** 2 / mse),
                         rng.double()]).float()
    return per_slice, stats


def slice_metrics(pred, target, nvs=None, *, activation="none", cylinder=False, data_range=None, k1=0.01, k2=0.03,
                  psnr_range=4.0):
    """Slice-wise SSIM, MSE, NMSE and PSNR of a reconstruction.

    pred (B, 1, H, W, D) fp32 / bf16 / fp16: the decoder output; target: the fp32 volume; nvs: valid
    slices per element (None: all).  p = activation(pred), zeroed where d >= nvs[b]; `data_range`
    None computes max(max p - min p, max t - min t) over the batch.  mse / nmse / psnr run over every
    voxel, or over the centre cylinder with cylinder=True (what the loss sees).  No gradients."""
    nvs = _check(pred, target, nvs, activation, data_range, k1, k2, psnr_range)
    args = (pred.detach().contiguous(), target.detach().contiguous(), nvs, bool(_ACTIVATIONS[activation]),
            bool(cylinder), 0.0 if data_range is None else float(data_range), float(k1), float(k2), float(psnr_range))
    if pred.is_cuda:
        from . import functional as Fn
        if Fn.binding() == "library":
            from . import library  # noqa: F401  (registers the operator)
            per_slice, stats = torch.ops.vq3d.slice_metrics(*args)
        else:
            per_slice, stats = slice_metrics_kernel(*args)
    else:
        with torch.no_grad():
            per_slice, stats = _slice_metrics_torch(*args)
    return SliceMetrics(stats[0], per_slice, stats[1], stats[2], stats[3], stats[4])


class SSIM3DSlices(nn.Module):
    """metrics/evaluate.py:27-36 with the ssim keyword arguments the reference passes: the mean SSIM
    over the (b, d) slices of two (B, 1, H, W, D) volumes.  Only PL's default window is built."""

    def __init__(self, data_range=None, kernel_size=KERNEL_SIZE, sigma=SIGMA, k1=0.01, k2=0.03):
        super().__init__()
        if tuple(kernel_size) != KERNEL_SIZE or tuple(float(s) for s in sigma) != SIGMA:
            raise ValueError(f"SSIM3DSlices supports kernel_size={KERNEL_SIZE}, sigma={SIGMA} only (got "
                             f"kernel_size={tuple(kernel_size)}, sigma={tuple(sigma)})")
        self.data_range, self.k1, self.k2 = data_range, k1, k2

    def forward(self, pred, target):
        return slice_metrics(pred, target.float(), data_range=self.data_range, k1=self.k1, k2=self.k2).ssim


def nmse(orig: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """Normalised mean squared error (metrics/evaluate.py:18-20), on the tensors as given."""
    return (pred - orig).square().sum() / orig.square().sum()


def psnr(orig: torch.Tensor, pred: torch.Tensor, data_range: float) -> torch.Tensor:
    """Peak signal-to-noise ratio in dB (metrics/evaluate.py:23-24), on the tensors as given."""
    return 10 * torch.log10(data_range ** 2 / (pred - orig).square().mean())
