"""Score a checkpoint's reconstructions, the counterpart of the reference's
vqvae/calc_ssim_from_checkpoint.py.

    python -m vq3d.evaluate DATASET CKPT [--split val|train|both] [--batch-size N] [--out FILE.json]

As that script does: seed 42 (so the train / validation split is the training run's), CTDataModule,
the model in eval mode, SSIM over F.elu(decoder output) against the input volume with
data_range = 4 - (-0.24), no slice masking.  Where the reference collects one SSIM per batch and
stops in `breakpoint()`, this writes a JSON report: for every volume its SSIM, the SSIM of each of
its slices, nmse and psnr (psnr range 4, model.py:25), and per split the means over the volumes.
Every volume of a split is scored once, in dataset order (the reference's train loader shuffles and
drops the last partial batch).  All figures come from vq3d.metrics.slice_metrics, one fused kernel
pass per volume.
"""
import json
import sys
from argparse import ArgumentParser, Namespace
from pathlib import Path

import torch

from .metrics import slice_metrics

DATA_MIN, DATA_MAX = -0.24, 4.0
DATA_RANGE = DATA_MAX - DATA_MIN
PSNR_RANGE = 4.0
SCALARS = ("ssim", "nmse", "psnr")


def build_parser():
    parser = ArgumentParser(description="SSIM / nmse / psnr of a VQ-VAE checkpoint over a CT dataset")
    parser.add_argument("dataset_path", type=Path)
    parser.add_argument("ckpt_path", type=Path)
    parser.add_argument("--split", choices=("val", "train", "both"), default="val")
    parser.add_argument("--batch-size", type=int, default=5)
    parser.add_argument("--out", type=Path, default=None, help="JSON report (default: standard output)")
    return parser


def parse_arguments(argv=None):
    return build_parser().parse_args(argv)


def splits_of(name):
    """The splits `--split` names, validation first (the reference's order)."""
    if name not in ("val", "train", "both"):
        raise ValueError(f"split must be val, train or both, not {name!r}")
    return ["val", "train"] if name == "both" else [name]


def volume_record(index, q):
    """One volume's entry from its SliceMetrics (a batch of one)."""
    return {"index": int(index), "ssim": float(q.ssim), "nmse": float(q.nmse), "psnr": float(q.psnr),
            "ssim_per_slice": [float(v) for v in q.ssim_per_slice.reshape(-1).tolist()]}


def summarise(records):
    """A split's report: its volume records and the mean of every scalar over them."""
    n = len(records)
    mean = {k: (sum(r[k] for r in records) / n if n else None) for k in SCALARS}
    return {"count": n, "mean": mean, "volumes": list(records)}


def make_report(args, per_split):
    return {"dataset": str(args.dataset_path), "checkpoint": str(args.ckpt_path), "seed": 42,
            "data_range": DATA_RANGE, "psnr_range": PSNR_RANGE,
            "splits": {name: summarise(recs) for name, recs in per_split.items()}}


def write_report(report, out=None):
    text = json.dumps(report, indent=1)
    if out is None:
        sys.stdout.write(text + "\n")
    else:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text + "\n")
    return text


def score_split(model, dataset, batch_size, num_workers, dev):
    """The volume records of one split: one forward per batch, one metrics pass per volume."""
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                         drop_last=False)
    records = []
    with torch.no_grad():
        for batch, _ in loader:
            x = batch.to(dev).float()
            out, *_ = model(x)
            for i in range(x.shape[0]):
                q = slice_metrics(out[i:i + 1], x[i:i + 1], activation="elu", data_range=DATA_RANGE,
                                  psnr_range=PSNR_RANGE)
                records.append(volume_record(len(records), q))
    return records


def main(args: Namespace, datamodule=None):
    if not torch.cuda.is_available():
        raise RuntimeError("vq3d.evaluate runs the model on the HIP path: a GPU is required")
    from .data import CTDataModule
    from .model import VQVAE
    from .train import seed_everything
    dev = torch.device("cuda", torch.cuda.current_device())
    seed_everything(42)  # the training run's seed: the same train / validation split
    if datamodule is None:
        datamodule = CTDataModule(path=args.dataset_path, batch_size=args.batch_size, num_workers=5)
    datamodule.setup()
    model = VQVAE.load_from_checkpoint(str(args.ckpt_path)).to(dev)
    model.eval()
    datasets = {"val": datamodule.val_dataset, "train": datamodule.train_dataset}
    per_split = {name: score_split(model, datasets[name], args.batch_size, datamodule.num_workers, dev)
                 for name in splits_of(args.split)}
    report = make_report(args, per_split)
    write_report(report, args.out)
    return report


def cli(argv=None):
    main(parse_arguments(argv))
    return 0


if __name__ == "__main__":
    raise SystemExit(cli())
