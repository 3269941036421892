"""vq3d — MI355X-native 3D VQ-VAE-2 training path (module API of sara-nl/3D-VQ-VAE-2's
vqvae package; kernels in libvq3d.so, C-ABI in include/vq3d.h)."""
from . import _lib  # noqa: F401
from .layers import (Conv3d, Decoder, DownBlock, Encoder2, EvonormResBlock, FixupResBlock,  # noqa: F401
                     PreActFixupResBlock, PreQuantizationConditioning, Quantizer, ResizeConv3D, UpBlock)
from .evonorm import EvoNorm3DS0  # noqa: F401
from .model import VQVAE, default_args  # noqa: F401
from .metrics import SSIM3DSlices, SliceMetrics, nmse, psnr, slice_metrics  # noqa: F401

__all__ = ["VQVAE", "default_args", "Encoder2", "Decoder", "PreActFixupResBlock", "FixupResBlock",
           "EvonormResBlock", "Quantizer", "ResizeConv3D", "EvoNorm3DS0", "DownBlock", "UpBlock",
           "PreQuantizationConditioning", "Conv3d", "slice_metrics", "SliceMetrics", "SSIM3DSlices", "nmse", "psnr",
           "sample_codes", "PixelCNN", "cond_embed_reference"]


def __getattr__(name):
    # vq3d.sample is also the `python -m vq3d.sample` program: importing it here, ahead of its run as
    # __main__, would execute the module twice (runpy warns), so sample_codes resolves on first use
    if name == "sample_codes":
        from .sample import sample_codes
        return sample_codes
    if name == "PixelCNN":  # the priors load on first use (vq3d.pixelcnn pulls in the PixelSNAIL layers)
        from .pixelcnn import PixelCNN
        return PixelCNN
    if name == "cond_embed_reference":  # (vq3d.cond_embed is the module; its function vq3d.cond_embed.cond_embed)
        from .cond_embed import cond_embed_reference
        return cond_embed_reference
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
