"""Training entry for the PixelCNN priors over extracted codes -- the conditioned mid / bottom priors of a
VQ-VAE-2 hierarchy and the unconditioned top one (reference pixel_model/train.py with --use-model pixelcnn,
slurm-jobs/train_pixelcnn_*.job):

    python -m vq3d.train_pixelcnn CODES LEVEL --metric cross_entropy --use-pre-activation True
        [--use-conditioning True] [flags of PixelCNN.add_model_specific_args] [--batch-size B]
        [--compute-dtype bf16|fp16|fp32] [--max_epochs N] [--max_steps N] [--default_root_dir DIR]
        [--resume_from_checkpoint last.ckpt]

CODES is a `vq3d.extract.CodeStore` directory, LEVEL the hierarchy level to model (0 = bottom).  Everything
but the model is vq3d.train_prior's: its CodesDataModule, metrics, validation, checkpointing and fit loop.
With --use-conditioning True the batch's second tensor -- level LEVEL + 1, which CodesDataset returns next to
LEVEL -- is the condition, the store's num_embeddings pair gives [K, Kc], and the condition enters the
captured step as a second static input of the StepGraph; mixup's lam and permutation stay device tensors
the kernels (the input blend, vq3d.cond_embed, vq3d.head_loss) read at replay.  Mixup runs whenever
--mixup-alpha != 0, and the reference's default is 1: on.  --use-mixup-batch-hack is parsed and has no
effect, as in vq3d.train_prior.  The checkpoints are what `vq3d.sample --use-model pixelcnn` reads.

`python -m vq3d.train_prior --use-model pixelcnn` keeps refusing: this is the PixelCNN's entry.
"""
from argparse import ArgumentParser
from pathlib import Path

from . import train as T
from . import train_prior as TP
from .pixelcnn import PixelCNN


def build_parser():
    parser = ArgumentParser()
    parser = PixelCNN.add_model_specific_args(parser)
    parser = T.add_trainer_args(parser)
    parser.add_argument("dataset_path", type=Path)
    parser.add_argument("level", type=int, help="which hierarchy level to train the prior of (0: bottom)")
    parser.add_argument("--batch-size", type=int)
    parser.add_argument("--compute-dtype", choices=TP.DTYPES, default="bf16",
                        help="activation / GEMM operand dtype of the prior (parameters are fp32 masters)")
    parser.set_defaults(gpus="-1", accelerator="ddp", benchmark=True, num_sanity_val_steps=0, precision=16,
                        log_every_n_steps=50, val_check_interval=0.5, flush_logs_every_n_steps=100,
                        weights_summary="full", max_epochs=int(5e4))
    return parser


def parse_arguments(argv=None):
    args = build_parser().parse_args(argv)
    args.use_model = "pixelcnn"
    args.dataset_path = str(args.dataset_path.resolve())
    return args


def main(args, datamodule=None):
    return TP.main(args, datamodule, PixelCNN)


def cli(argv=None, datamodule=None):
    """The command: the ranks' exit code when it started them (--gpus > 1), else main's
    (model, optimizer, log history, checkpointer) of the run in this process."""
    return TP.cli(argv, datamodule, parse=parse_arguments, module="vq3d.train_pixelcnn", model_cls=PixelCNN)


if __name__ == "__main__":
    _rc = cli()
    raise SystemExit(_rc if isinstance(_rc, int) else 0)
