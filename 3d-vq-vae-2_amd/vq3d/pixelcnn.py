"""PixelCNN prior over VQ-VAE codes (reference pixel_model/pixelcnn.py + pixel_model/layers.py), module
API, argument parsing, init and state_dict of the reference, GPU path through libvq3d.  The published mid
and bottom priors of a VQ-VAE-2 hierarchy are this model conditioned on the level above
(train_pixelcnn_mid.job / train_pixelcnn_bottom.job: --use-conditioning True --use-pre-activation True); the
top prior is the unconditioned one.

A pre-activation PixelCNN is parse_input, num_resblocks + 1 PreActFixupCausalResBlocks (the first with mask
'A') and parse_output: the blocks are vq3d.pixelsnail's, on the same conv engines, lanes and glue kernels.
There is no attention.  Conditioning (pixelcnn.py:113-128, :289-313; layers.py:444-461):

* e = embed_condition(interpolate(one_hot(condition codes), size=data grid, mode='trilinear')) with mixup's
  blend of the interpolated one-hot is vq3d.cond_embed (csrc/cond_embed.hip): a trilinear blend of columns of
  the embedding weight, nothing of the chain in memory, a deterministic backward;
* per layer p = layer.condition(e), a 1x1x1 conv on vq3d_rows_gemm, is added to all three stack streams
  after branch_conv2 and dropout, fused with the pre-activation in front of branch_conv3
  (pixelsnail.PreActAddFn);
* e and every p are made on lane 0 and reach lanes 1 and 2 through pixelsnail._take, so their gradients
  collect on lane 0 only (the cross-lane rules at the top of vq3d/pixelsnail.py);
* for a slab prefix (the sampler's input) p is the crop of the full-grid p, never an interpolation to the
  smaller grid (layers.py:452).

Refused, as the reference cannot run them either: use_pre_activation=False (FixupCausalResBlock.forward
returns a tuple, pixel_model/layers.py:610, which breaks the model's own loop over the layers),
use_concat_activation (the block says why); use_gated_block is forced to False by the reference itself.
"""
from argparse import ArgumentParser, Namespace
from collections import deque

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import pixelsnail as PS
from .cond_embed import cond_embed
from .pixelsnail import PreActFixupCausalResBlock, cl, mixup_draw, pointwise


class PixelCNN(nn.Module):
    """pixel_model/pixelcnn.py:27-316"""

    def __init__(self, args, compute_dtype="bf16"):
        super().__init__()
        self.hparams = {"args": args}  # what checkpoint.save_checkpoint stores (PL's save_hyperparameters)
        self._parse_input_args(args)
        self.compute_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(compute_dtype, torch.float32)
        self.parse_input = nn.Conv3d(in_channels=self.input_dim, out_channels=self.model_dim, kernel_size=1)
        condition_dim = self.model_dim if self.use_conditioning else 0
        self.embed_condition = nn.Conv3d(in_channels=self.condition_dim, out_channels=condition_dim,
                                         kernel_size=1) if self.use_conditioning else None
        self.layers = nn.ModuleList([
            PreActFixupCausalResBlock(in_channels=self.model_dim, out_channels=self.model_dim,
                                      kernel_size=self.kernel_size, mask="A" if i == 0 else "B",
                                      dropout_prob=self.dropout_prob, condition_dim=condition_dim,
                                      condition_kernel_size=1, bottleneck_divisor=self.bottleneck_divisor,
                                      concat_activation=self.use_concat_activation)
            for i in range(self.num_resblocks + 1)])
        self.parse_output = nn.Conv3d(in_channels=self.model_dim, out_channels=self.input_dim, kernel_size=1)
        num_layers = self.num_resblocks + 1  # plus input / output resblocks
        self.apply(lambda layer: layer.initialize_weights(num_layers=num_layers)
                   if isinstance(layer, PreActFixupCausalResBlock) else None)

    def _parse_input_args(self, args: Namespace):
        args.use_gated_block = False
        self.input_dim, self.condition_dim = args.num_embeddings
        if not args.use_conditioning:
            self.condition_dim = 0
        for name in ("model_dim", "kernel_size", "num_resblocks", "dropout_prob", "use_gated_block",
                     "use_conditioning", "use_concat_activation", "bottleneck_divisor", "mixup_alpha",
                     "use_mixup_batch_hack"):
            setattr(self, name, getattr(args, name))
        if not args.use_pre_activation:
            raise NotImplementedError("use_pre_activation=False: the reference's FixupCausalResBlock.forward returns "
                                      "a tuple (pixel_model/layers.py:610), which its own model loop cannot feed to "
                                      "the next layer; pass --use-pre-activation True (the published priors do)")
        if args.metric != "cross_entropy":
            raise ValueError
        self.lr = args.lr

    @classmethod
    def add_model_specific_args(cls, parent_parser):
        """pixelcnn.py:185-211"""
        from .utils import booltype
        parser = ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument("--model-dim", default=32, type=int)
        parser.add_argument("--kernel-size", default=3, type=int)
        parser.add_argument("--num-resblocks", default=18, type=int)
        parser.add_argument("--dropout-prob", default=0.5, type=float, help="Set to 0 to disable dropout.")
        parser.add_argument("--use-pre-activation", default=False, type=booltype)
        parser.add_argument("--use-gated-block", default=False, type=booltype)
        parser.add_argument("--bottleneck-divisor", default=4, type=int,
                            help="Ignored if `--use-pre-activation False` is passed. Set to 1 to disable bottlenecking")
        parser.add_argument("--use-conditioning", default=False, type=booltype)
        parser.add_argument("--use-concat-activation", default=False, type=booltype)
        parser.add_argument("--mixup-alpha", default=1, type=float, help="Set to 0 to disable mixup")
        parser.add_argument("--use-mixup-batch-hack", default=False, type=booltype,
                            help="Will double the batch size in the dataloader, for but only for mixing")
        parser.add_argument("--metric", choices=["cross_entropy"])
        parser.add_argument("--lr", default=1e-5, type=float)
        return parser

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=self.lr, amsgrad=True)

    # ------------------------------------------------------------------ conditioning
    def _condition_codes(self, condition):
        if not self.use_conditioning:
            raise ValueError("this PixelCNN was built without conditioning (use_conditioning=False)")
        if not torch.is_tensor(condition) or condition.dtype != torch.int64:
            raise TypeError("the condition is the upper level's codes: an int64 (b, cd, ch, cw) tensor")
        if condition.dim() == 5 and condition.shape[1] == 1:
            condition = condition.squeeze(1)
        return condition

    def embed(self, condition, full_dims, d_out=None, mix=None):
        """e: embed_condition of the condition codes interpolated to the (D, H, W) grid full_dims, its first
        d_out slabs, in the compute dtype; mix = (lam_t, index_t) device tensors"""
        lam_t, index_t = (None, None) if mix is None else mix
        return cond_embed(self._condition_codes(condition), self.embed_condition.weight, self.embed_condition.bias,
                          full_dims, lam_t, index_t, d_out, self.compute_dtype)

    @torch.no_grad()
    def condition_cache(self, cond_codes, dims):
        """the full-grid condition projection of every layer (the reference's _generate_condition_cache,
        pixelcnn.py:289-295) for condition codes on the (D, H, W) grid dims: what `hidden` takes as
        condition_cache for every prefix of one sampling run"""
        PS.begin_forward(self)
        e = self.embed(cond_codes, dims)
        return deque(layer.project_condition(e, dims) for layer in self.layers)

    # ------------------------------------------------------------------ forward
    def hidden(self, onehot, full_dims=None, condition=None, condition_cache=None, mix=None):
        """the forward up to parse_output: the (b, model_dim, d, h, w) channels-last input of the output
        head, in the compute dtype.  full_dims = (D, h, w): onehot holds the first onehot.shape[2] slabs of
        a D-slab grid (the sampler's causally complete prefix) and the condition is that of the full grid,
        cropped.  condition: int64 (b, cd, ch, cw) codes of the level above; condition_cache: the
        full-grid projections of `condition_cache`, preferred; mix = (lam_t, index_t): mixup's blend of
        the condition (the caller blends onehot)."""
        dims = tuple(onehot.shape[2:])
        fd = dims if full_dims is None else tuple(int(v) for v in full_dims)
        if fd[1:] != dims[1:] or dims[0] > fd[0]:
            raise ValueError(f"a {dims} input is no slab prefix of a {fd} grid")
        if self.use_conditioning and condition is None and condition_cache is None:
            raise ValueError("a conditioned PixelCNN needs `condition` (or `condition_cache`)")
        if not self.use_conditioning and (condition is not None or condition_cache is not None):
            raise ValueError("this PixelCNN was built without conditioning (use_conditioning=False)")
        if condition is not None and condition_cache is None:
            condition = self._condition_codes(condition)
        x = cl(onehot.to(self.compute_dtype))
        PS.begin_forward(self)
        x = cl(pointwise(x, self.parse_input.weight, self.parse_input.bias))
        with PS.forward_lanes(self, x):
            cache = e = None
            if condition_cache is not None:
                cache = list(condition_cache)
                if len(cache) != len(self.layers):
                    raise ValueError(f"the condition cache holds {len(cache)} projections for {len(self.layers)} layers")
            elif condition is not None:
                e = self.embed(condition, fd, dims[0], mix)  # on lane 0, as every projection below
            stack = [x] + [PS._take(i, 0, x) for i in (1, 2)]
            for j, layer in enumerate(self.layers):
                p = None
                if cache is not None:
                    p = PS.crop_condition(cache[j], dims)
                elif e is not None:
                    p = layer.project_condition(e, dims)
                stack = layer.run(stack, cond=p)
            stack = [stack[0]] + [PS._take(0, i, stack[i]) for i in (1, 2)]
        return PS._operand(stack[0] + stack[1] + stack[2])

    def logits(self, onehot, condition=None, condition_cache=None, mix=None, full_dims=None):
        """forward (pixelcnn.py:298-315) of a one-hot (b, K, d, h, w) input; fp32 logits."""
        hid = self.hidden(onehot, full_dims, condition, condition_cache, mix)
        return pointwise(hid, self.parse_output.weight, self.parse_output.bias).float()

    def forward(self, data, condition=None, condition_cache=None):
        return self.logits(data, condition, condition_cache)

    def _split(self, batch):
        """(codes (b, d, h, w), condition codes or None) of a batch (pixelcnn.py:106-121)"""
        if len(batch) == 1 or not self.use_conditioning:
            return batch[0].squeeze(1), None
        return batch[0].squeeze(1), batch[1].squeeze(1)

    def cross_entropy(self, batch, batch_idx=0, metrics=None, mode="train"):
        """pixelcnn.py:102-148: mean cross-entropy of the logits over every code position, with mixup in
        training whenever mixup_alpha != 0 (the reference's default 1 is on), plus bits_per_dim."""
        codes, condition = self._split(batch)
        onehot = F.one_hot(codes, num_classes=self.input_dim).permute(0, 4, 1, 2, 3).float()
        mix = mixup_draw(codes.shape[0], self.mixup_alpha) if (self.mixup_alpha != 0 and mode == "train") else None
        return self.cross_entropy_onehot(onehot, codes, mix, condition)

    def cross_entropy_onehot(self, onehot, codes, mix=None, condition=None):
        """the loss from a prepared one-hot input; mix = (lam, index) from mixup_draw (host values)"""
        if mix is None:
            logits = self.logits(onehot, condition)
            unreduced = F.cross_entropy(logits, codes, reduction="none")
        else:
            lam, index = mix
            idx = index.to(onehot.device).long()
            x = onehot.float()
            lam_t = torch.tensor(float(lam), dtype=torch.float32, device=onehot.device)
            logits = self.logits(lam * x + (1 - lam) * x[idx], condition, mix=(lam_t, idx))
            unreduced = (lam * F.cross_entropy(logits, codes, reduction="none")
                         + (1 - lam) * F.cross_entropy(logits, codes[idx], reduction="none"))
        loss = unreduced.mean()
        return loss, {"bits_per_dim": loss.detach() / np.log(2)}

    def loss_rows(self, onehot, codes, mix=None, condition=None):
        """The per-position loss and prediction of a prepared one-hot (b, K, d, h, w) input: `hidden` followed
        by the fused output head (vq3d.head_loss).  Returns (loss (b, d, h, w) fp32, pred (b, d, h, w) int64).
        mix = (lam_t, index_t), DEVICE tensors -- fp32 0-d lam_t, int64 (b,) index_t: input and interpolated
        condition are lam x + (1 - lam) x[index] and the loss lam CE(y) + (1 - lam) CE(y[index])
        (train_helpers.py:20-63), all read from the tensors when the kernels run, so a captured step replays
        with new draws copied into them."""
        from .head_loss import head_loss
        tb = lam_t = None
        x = onehot
        if mix is not None:
            lam_t, index_t = mix
            x = onehot.float()
            x = lam_t * x + (1 - lam_t) * x[index_t]
            tb = codes[index_t].reshape(-1)
        hid = self.hidden(x, condition=condition, mix=mix)
        rows = hid.permute(0, 2, 3, 4, 1).reshape(-1, hid.shape[1])
        loss, pred = head_loss(rows, self.parse_output.weight, self.parse_output.bias, codes.reshape(-1), tb, lam_t)
        return loss.view(codes.shape), pred.view(codes.shape)

    def training_step(self, batch, batch_idx):
        return self.cross_entropy(batch, batch_idx, mode="train")[0]


def default_args(**kw):
    """the reference's argparse defaults (pixelcnn.py:190-210) as a Namespace."""
    a = Namespace(num_embeddings=[512, 0], model_dim=32, kernel_size=3, num_resblocks=18, dropout_prob=0.5,
                  use_pre_activation=False, use_gated_block=False, bottleneck_divisor=4, use_conditioning=False,
                  use_concat_activation=False, mixup_alpha=1.0, use_mixup_batch_hack=False, metric="cross_entropy",
                  lr=1e-5)
    for k, v in kw.items():
        setattr(a, k, v)
    return a
