"""The PixelSNAIL prior's output head fused with its loss (reference pixel_model/pixelsnail.py:78-82
parse_output + :112-161 the cross-entropy of shared_step, with mixup's two targets,
train_helpers.py:50-63).  For hidden rows (n, c), parse_output's weight (K, c) and bias (K,), targets
a (and b) of shape (n,) and a mixing weight lam (1 when lam or b is absent), per row v:

    logit[j] = bias[j] + sum_c hidden[v, c] weight[j, c]    fp32, nothing rounded after the sum; 16-bit
                                                            rows round the weight to their format
    lse[v]   = log sum_j exp(logit[j])
    loss[v]  = lse[v] - lam logit[a[v]] - (1 - lam) logit[b[v]]
    pred[v]  = the first index of the largest logit

A target outside [0, K) matches no code and contributes 0.  With both targets valid this is
lam CE(a) + (1 - lam) CE(b) of F.cross_entropy(reduction='none').

16-bit GPU rows run csrc/head_loss.hip (vq3d_prior_head_loss_fwd / _bwd): the (n, K) logits never
reach memory, training reads the unrounded fp32 logits the sampler draws from,
and lam is a device scalar, so a captured step replays with new mixup draws.  The backward writes
dlogits in the rows' format and takes dHidden, dW and dbias from vq3d_rows_gemm / vq3d_rows_wgrad,
the weight and bias gradients added straight into the parameters' gradient buffers (as
pixelsnail.PointwiseFn).  CPU tensors and fp32 / fp64 rows take `head_loss_reference`, the definition
in torch (written from the definition, not from the HIP source: the tests hold the kernel to it).
"""
import ctypes

import torch

from . import _lib as L

K_MIN, K_MAX, C_MAX = 8, 1024, 1024


def _picked(logits, target):
    """logit[v, target[v]], 0 where the target is no code"""
    k = logits.shape[1]
    ok = (target >= 0) & (target < k)
    val = logits.gather(1, target.clamp(0, k - 1).long().view(-1, 1)).view(-1)
    return torch.where(ok, val, torch.zeros_like(val))


def head_loss_reference(hidden, weight, bias, target_a, target_b=None, lam=None):
    """(loss (n,), pred (n,) int64) by the definition above, differentiable by plain autograd.
    Arithmetic in fp32 (fp64 rows: fp64); 16-bit rows take the weight rounded to their format."""
    w = weight.reshape(weight.shape[0], -1)
    dt = torch.float64 if hidden.dtype == torch.float64 else torch.float32
    if hidden.dtype in (torch.bfloat16, torch.float16):
        w = w.to(hidden.dtype)
    logits = bias.to(dt) + hidden.to(dt) @ w.to(dt).t()
    lse = torch.logsumexp(logits, dim=1)
    if target_b is None or lam is None:
        loss = lse - _picked(logits, target_a)
    else:
        lam = lam.to(dt) if torch.is_tensor(lam) else lam
        loss = lse - lam * _picked(logits, target_a) - (1 - lam) * _picked(logits, target_b)
    k = logits.shape[1]
    top = logits.detach() == logits.detach().max(dim=1, keepdim=True).values
    idx = torch.arange(k, device=logits.device).expand_as(top)
    pred = torch.where(top, idx, torch.full_like(idx, k)).min(dim=1).values.clamp(max=k - 1)
    return loss, pred


def _rows(t):
    from .pixelsnail import _rows_ok
    return _rows_ok(t)


def head_loss_fwd_kernel(hidden, w16, bias, target_a, target_b=None, lam=None):
    """vq3d_prior_head_loss_fwd on the current stream: (loss fp32 (n,), pred int32 (n,), lse fp32 (n,))"""
    n, c = hidden.shape
    k = w16.shape[0]
    loss = torch.empty(n, dtype=torch.float32, device=hidden.device)
    lse = torch.empty_like(loss)
    pred = torch.empty(n, dtype=torch.int32, device=hidden.device)
    L.call("vq3d_prior_head_loss_fwd", L.dtype_code(hidden), n, c, k, L.ptr(hidden), hidden.stride(0), L.ptr(w16),
           w16.stride(0), L.ptr(bias), L.ptr(target_a), L.ptr(target_b), L.ptr(lam), L.ptr(loss), L.ptr(lse),
           L.ptr(pred), L.stream())
    return loss, pred, lse


def head_loss_bwd_kernel(gloss, hidden, w16, bias, target_a, target_b, lam, lse):
    """vq3d_prior_head_loss_bwd on the current stream: dlogits (n, K) in the rows' format"""
    n, c = hidden.shape
    k = w16.shape[0]
    dlogits = torch.empty((n, k), dtype=hidden.dtype, device=hidden.device)
    L.call("vq3d_prior_head_loss_bwd", L.dtype_code(hidden), n, c, k, L.ptr(hidden), hidden.stride(0), L.ptr(w16),
           w16.stride(0), L.ptr(bias), L.ptr(target_a), L.ptr(target_b), L.ptr(lam), L.ptr(lse), L.ptr(gloss),
           L.ptr(dlogits), k, L.stream())
    return dlogits


def head_grads(dlogits, hidden, w16, dw, db, want_hidden=True):
    """dHidden = dlogits W (returned, or None) and dw (K, c) += dlogits^T hidden, db (K,) += column sums of
    dlogits (fp32 buffers, either may be None together with nothing to add): vq3d_rows_gemm (trans_w = 1)
    and vq3d_rows_wgrad"""
    from .pixelsnail import _gemm_rows
    n, c = hidden.shape
    k = w16.shape[0]
    gx = _gemm_rows(dlogits, w16, 1, None, c) if want_hidden else None
    if dw is not None:
        nws = int(L.query("vq3d_rows_wgrad_workspace_bytes", n, k, c))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=hidden.device)
        L.call("vq3d_rows_wgrad", L.dtype_code(dlogits), n, k, c, L.ptr(dlogits), dlogits.stride(0), L.ptr(hidden),
               hidden.stride(0), L.ptr(dw), L.ptr(db), L.ptr(ws), ctypes.c_size_t(nws), L.stream())
    return gx


def _fwd(*args):
    from . import functional as Fn
    if Fn.binding() == "library":
        from . import library  # noqa: F401  (registers the operators)
        loss, pred, lse = torch.ops.vq3d.prior_head_loss(*args)
        return loss, pred, lse
    return head_loss_fwd_kernel(*args)


def _bwd(*args):
    from . import functional as Fn
    if Fn.binding() == "library":
        return torch.ops.vq3d.prior_head_loss_backward(*args)
    return head_loss_bwd_kernel(*args)


class HeadLossFn(torch.autograd.Function):
    """(loss rows, pred) of 16-bit GPU rows on head_loss.hip.  Saves the rows, the 16-bit weight and
    lse (n floats); the backward is one recomputing launch (dlogits), one vq3d_rows_gemm and one
    vq3d_rows_wgrad, the parameter gradients added into their buffers (pixelsnail._direct)."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, target_a, target_b, lam):
        from . import pixelsnail as PS
        k = weight.shape[0]
        w16 = PS._w16(weight, hidden.dtype).reshape(k, -1)
        if not _rows(w16):
            w16 = w16.contiguous()
        b32 = bias.detach()
        loss, pred, lse = _fwd(hidden, w16, b32, target_a, target_b, lam)
        ctx.save_for_backward(hidden, w16, b32, target_a, target_b, lam, lse)
        ctx.prm = (weight, bias)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, gloss, _gpred):
        from . import pixelsnail as PS
        hidden, w16, b32, target_a, target_b, lam, lse = ctx.saved_tensors
        weight, bias = ctx.prm
        gloss = gloss.float().contiguous()
        dlogits = _bwd(gloss, hidden, w16, b32, target_a, target_b, lam, lse)
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or PS._direct(weight) or PS._direct(bias)
        dw = db = None
        if need_w:
            dw = PS._param_grad(weight)
            db = PS._param_grad(bias)
        gx = head_grads(dlogits, hidden, w16, None if dw is None else dw.view(w16.shape[0], -1), db,
                        ctx.needs_input_grad[0])
        return (gx, None if dw is None or PS._direct(weight) else dw, None if db is None or PS._direct(bias) else db,
                None, None, None)


def _check(hidden, weight, bias, target_a, target_b, lam):
    if hidden.dim() != 2:
        raise ValueError(f"hidden must be (rows, channels), got {tuple(hidden.shape)}")
    n, c = hidden.shape
    k = weight.shape[0]
    if weight.numel() != k * c or bias.numel() != k:
        raise ValueError("hidden, weight and bias do not fit together")
    for t in (target_a, target_b):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (n,)):
            raise ValueError("targets must be int64 (rows,) tensors")
    if torch.is_tensor(lam) and lam.numel() != 1:
        raise ValueError("lam must hold one value")


def head_loss(hidden, weight, bias, target_a, target_b=None, lam=None):
    """(loss_rows fp32 (n,), pred int64 (n,)) of hidden rows (n, c): see the module doc.  lam: None, a
    float, or a one-element fp32 tensor on the rows' device (read at run time on the GPU path: a captured
    graph replays with the value then in it).  Differentiable in hidden, weight and bias."""
    _check(hidden, weight, bias, target_a, target_b, lam)
    if not hidden.is_cuda or hidden.dtype not in (torch.bfloat16, torch.float16):
        loss, pred = head_loss_reference(hidden, weight, bias, target_a, target_b, lam)
        return loss.float() if loss.dtype != torch.float64 else loss, pred
    n, c = hidden.shape
    k = weight.shape[0]
    if not (K_MIN <= k <= K_MAX and k % 8 == 0):
        raise ValueError(f"{K_MIN} <= K <= {K_MAX} and K % 8 == 0, got {k}")
    if c % 8 or not 0 < c <= C_MAX:
        raise ValueError(f"the hidden width must be a multiple of 8, at most {C_MAX}, got {c}")
    if not _rows(hidden):
        hidden = hidden.contiguous()
    if target_b is None:
        lam = None
    elif lam is None:
        target_b = None
    elif not torch.is_tensor(lam):
        lam = torch.tensor(float(lam), dtype=torch.float32, device=hidden.device)
    elif lam.dtype != torch.float32 or lam.device != hidden.device:
        raise TypeError("lam must be an fp32 tensor on the rows' device")
    target_a = target_a.contiguous()
    target_b = None if target_b is None else target_b.contiguous()
    loss, pred = HeadLossFn.apply(hidden, weight, bias, target_a, target_b, lam)
    return loss, pred.long()
