"""Training entry for the PixelSNAIL priors over extracted codes (vq3d.train_pixelcnn drives the same
datamodule, metrics, validation, checkpointing and fit loop for the PixelCNN priors), mirroring the reference's
pixel_model/train.py + utils/load_lmdb_dataset.py:12-50 + PixelSNAIL.shared_step on the vq3d path:

    python -m vq3d.train_prior CODES LEVEL --use-model pixelsnail --metric cross_entropy
        [--batch-size B] [flags of PixelSNAIL.add_model_specific_args] [--compute-dtype bf16|fp16|fp32]
        [--max_epochs N] [--max_steps N] [--default_root_dir DIR] [--resume_from_checkpoint last.ckpt]

CODES is a `vq3d.extract.CodeStore` directory (what `vq3d.extract` writes), LEVEL the hierarchy level
to model (0 = bottom).  The checkpoints (PL 1.2 layout, vq3d.checkpoint) are what `vq3d.sample` reads.

What the reference gets from PyTorch-Lightning, restated as in vq3d.train (whose seed_everything,
Checkpointer, resume_counters and launch_ranks are reused):
  * arguments: --use-model, the model's flags, the Trainer flags with the reference's set_defaults
    (train.py:28-44), dataset_path, level, --batch-size;
  * seed_everything(42); CodesDataModule(path, embedding_id=level, batch_size, num_workers=5): a
    random_split into int(0.95 len) / rest, train loader shuffled with drop_last, validation loader
    drop_last without shuffling; args.num_embeddings from the data; only batch[0] is used
    (conditioning off, as in the published jobs);
  * the step: one-hot on the device (scatter_, no host validation), mixup draws on the host every
    step (mixup_draw) copied into static device tensors, PixelSNAIL.loss_rows(...).mean() through the
    fused output head, GradScaler, the gradient all-reduce, FusedAdam over FlatParams -- captured as
    one HIP graph per batch shape (StepGraph): lam and the permutation are device tensors, so every
    replay sees its own draws.  The prior's autograd Functions do not report their parameters to
    parallel.grads_ready, so every all-reduce bucket is issued after the backward (no overlap);
  * logs every log_every_n_steps: train_loss_{min,max,mean,median,std} (sub_metric_log_dict:
    torch.median is the lower median, torch.std unbiased) and train_bits_per_dim = mean / ln 2, from
    the loss rows the step produced;
  * validation every val_check_interval (eval mode, no mixup): the five val_loss_*,
    val_bits_per_dim and val_accuracy = mean(pred == codes) per batch, averaged over the batches of
    every rank (model.val_metrics);
  * ModelCheckpoint(save_top_k=1, save_last=True, monitor='val_loss_mean').
"""
import math
from argparse import ArgumentParser, Namespace
from pathlib import Path

import torch

from . import parallel
from . import train as T
from .checkpoint import load_checkpoint
from .extract import CodesDataset
from .flat import FlatParams
from .graph import StepGraph
from .optim import FusedAdam, GradScaler
from .pixelsnail import PixelSNAIL, mixup_draw

CL = torch.channels_last_3d
DTYPES = ("bf16", "fp16", "fp32")
LOSS_STATS = ("min", "max", "mean", "median", "std")
VAL_KEYS = tuple(f"val_loss_{s}" for s in LOSS_STATS) + ("val_bits_per_dim", "val_accuracy")


# ------------------------------------------------------------------ arguments
def build_parser(argv=None):
    parser = ArgumentParser()
    parser.add_argument("--use-model", type=str, choices=["pixelcnn", "pixelsnail"], default="pixelcnn")
    use_model = parser.parse_known_args(argv)[0].use_model
    if use_model == "pixelcnn":
        raise NotImplementedError("--use-model pixelcnn: this entry trains PixelSNAIL priors only (DESIGN.md §8); the "
                                  "PixelCNN prior has its own, python -m vq3d.train_pixelcnn -- or pass "
                                  "--use-model pixelsnail")
    parser = PixelSNAIL.add_model_specific_args(parser)
    parser = T.add_trainer_args(parser)
    parser.add_argument("dataset_path", type=Path)
    parser.add_argument("level", type=int, help="which hierarchy level to train the prior of (0: bottom)")
    parser.add_argument("--batch-size", type=int)
    parser.add_argument("--compute-dtype", choices=DTYPES, default="bf16",
                        help="activation / GEMM operand dtype of the prior (parameters are fp32 masters)")
    parser.set_defaults(gpus="-1", accelerator="ddp", benchmark=True, num_sanity_val_steps=0, precision=16,
                        log_every_n_steps=50, val_check_interval=0.5, flush_logs_every_n_steps=100,
                        weights_summary="full", max_epochs=int(5e4))
    return parser, use_model


def parse_arguments(argv=None):
    parser, use_model = build_parser(argv)
    args = parser.parse_args(argv)
    args.use_model = use_model
    args.dataset_path = str(args.dataset_path.resolve())
    return args


# ------------------------------------------------------------------ data
class CodesDataModule:
    """LMDBDataModule (load_lmdb_dataset.py:12-50) over a CodeStore directory."""

    def __init__(self, path, embedding_id, batch_size=16, train_frac=0.95, num_workers=6):
        assert 0 <= train_frac <= 1
        self.path, self.embedding_id, self.batch_size = str(path), embedding_id, batch_size
        self.train_frac, self.num_workers = train_frac, num_workers

    def setup(self, stage=None):
        dataset = CodesDataset(self.path, self.embedding_id, transform=None)
        self.n_enc = dataset.n_enc
        self.num_embeddings = dataset.num_embeddings
        self.train_len = int(len(dataset) * self.train_frac)
        self.val_len = len(dataset) - self.train_len
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(dataset, [self.train_len, self.val_len])

    def _loader(self, ds, shuffle, sampler=None):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, num_workers=self.num_workers,
                                           pin_memory=True, shuffle=shuffle and sampler is None, sampler=sampler,
                                           drop_last=True, persistent_workers=self.num_workers > 0)

    def train_dataloader(self, sampler=None):
        return self._loader(self.train_dataset, True, sampler)

    def val_dataloader(self, sampler=None):
        return self._loader(self.val_dataset, False, sampler)


# ------------------------------------------------------------------ metrics
def loss_metrics(rows, mode):
    """sub_metric_log_dict('loss', rows) + bits_per_dim of a loss tensor (logging_helpers.py:5-15,
    pixelsnail.py:150-154) as 0-d float64 tensors keyed `{mode}_...`: torch.median is the lower
    median, torch.std the unbiased one; bits_per_dim = mean / ln 2."""
    r = rows.detach().reshape(-1).float()
    out = {f"{mode}_loss_{name}": fn(r).double()
           for name, fn in zip(LOSS_STATS, (torch.min, torch.max, torch.mean, torch.median, torch.std))}
    out[f"{mode}_bits_per_dim"] = out[f"{mode}_loss_mean"] / math.log(2)
    return out


def onehot_codes(codes, k, dtype=torch.float32):
    """the (b, K, d, h, w) channels-last one-hot of int64 (b, d, h, w) codes on their device, by
    scatter_ (F.one_hot validates its input on the host, which a captured graph cannot do)"""
    b = codes.shape[0]
    x = torch.empty((b, k) + tuple(codes.shape[1:]), dtype=dtype, device=codes.device, memory_format=CL).zero_()
    return x.scatter_(1, codes.unsqueeze(1), 1.0)


def _codes(batch, dev):
    return torch.as_tensor(batch[0]).squeeze(1).to(dev, non_blocking=True).long()


def _condition(batch, dev, model):
    """the batch's second tensor -- the level above -- as int64 (b, cd, ch, cw) condition codes when the
    model is conditioned (pixelcnn.py:106-113), else None"""
    if len(batch) == 1 or not getattr(model, "use_conditioning", False):
        return None
    return torch.as_tensor(batch[1]).squeeze(1).to(dev, non_blocking=True).long()


def _cond_kw(cond):
    return {} if cond is None else {"condition": cond}


def validate(model, loader, dev):
    """The mean of every VAL_KEYS value over the validation batches of all ranks (as train.validate):
    returns val_loss_mean (None without batches), all seven in model.val_metrics."""
    model.eval()
    tot, n = torch.zeros(len(VAL_KEYS), dtype=torch.float64, device=dev), 0
    with torch.no_grad():
        for batch in loader:
            codes = _codes(batch, dev)
            rows, pred = model.loss_rows(onehot_codes(codes, model.input_dim), codes,
                                         **_cond_kw(_condition(batch, dev, model)))
            m = loss_metrics(rows, "val")
            m["val_accuracy"] = (pred == codes).double().mean()
            tot += torch.stack([m[k] for k in VAL_KEYS])
            n += 1
    model.train()
    t = torch.cat([tot, torch.tensor([float(n)], dtype=torch.float64, device=dev)])
    if torch.distributed.is_initialized():
        torch.distributed.all_reduce(t)
    t = t.tolist()
    n = int(t[-1])
    model.val_metrics = {k: v / n for k, v in zip(VAL_KEYS, t)} if n else {}
    return model.val_metrics.get("val_loss_mean")


# ------------------------------------------------------------------ training
def main(args: Namespace, datamodule=None, model_cls=PixelSNAIL):
    """pixel_model/train.py:55-77.  model_cls: PixelSNAIL, or vq3d.pixelcnn.PixelCNN (vq3d.train_pixelcnn),
    whose conditioned form takes the batch's second tensor as its condition."""
    rank, world, _, dev = parallel.init_from_env()
    if dev.type != "cuda":
        raise RuntimeError("the priors train on the HIP path: a GPU is required")
    if model_cls is PixelSNAIL and getattr(args, "use_conditioning", False):
        raise NotImplementedError("conditioning (use_conditioning) is not implemented for PixelSNAIL")
    T.seed_everything(42)
    if datamodule is None:
        datamodule = CodesDataModule(path=args.dataset_path, embedding_id=args.level, batch_size=args.batch_size,
                                     num_workers=5)
    datamodule.setup()
    args.num_embeddings = [int(k) for k in datamodule.num_embeddings]
    if getattr(args, "use_conditioning", False) and not args.num_embeddings[1]:
        raise ValueError(f"level {args.level} is the top of its store: there is no level above to condition on")
    model = model_cls(args, compute_dtype=getattr(args, "compute_dtype", "bf16")).to(dev)
    model.train()
    model.flat = FlatParams(model.parameters(), dev)  # what parallel.GradientAllReduce averages
    opt = FusedAdam(model.parameters(), model.flat, lr=model.lr, amsgrad=True)
    scaler = GradScaler(dev, enabled=model.compute_dtype == torch.float16)
    ckpt = T.Checkpointer(Path(args.default_root_dir) / "checkpoints", monitor="val_loss_mean")
    epoch0, step = 0, 0
    if args.resume_from_checkpoint:
        ck = load_checkpoint(args.resume_from_checkpoint)
        model.load_state_dict(ck["state_dict"])
        if ck.get("optimizer_states"):
            opt.load_state_dict(ck["optimizer_states"][0])
        scaler.load_state_dict(ck.get("native_amp_scaling_state"))
        epoch0, step = T.resume_counters(ck)
        st = ck.get("callbacks", {}).get("ModelCheckpoint") or {}
        ckpt.best_score, ckpt.best_path = st.get("best_model_score"), st.get("best_model_path")
    # built after any resume (the replicas start from the restored state); the prior's autograd
    # Functions report nothing to grads_ready: every bucket goes out in reducer(), after the backward
    reducer = parallel.GradientAllReduce(model, overlap=False)
    try:
        return _fit(args, model, opt, reducer, ckpt, datamodule, rank, world, dev, epoch0, step, scaler)
    finally:
        reducer.close()


def _fit(args, model, opt, reducer, ckpt, datamodule, rank, world, dev, epoch0, step, scaler):
    train_ds, val_ds = datamodule.train_dataset, datamodule.val_dataset
    DS = torch.utils.data.distributed.DistributedSampler
    sampler = DS(train_ds, world, rank, shuffle=True, seed=42, drop_last=True) if world > 1 else None
    loader = datamodule.train_dataloader(sampler)
    vloader = datamodule.val_dataloader(DS(val_ds, world, rank, shuffle=False) if world > 1 else None)
    n_batches = len(loader)
    bsz, k = datamodule.batch_size, model.input_dim
    mixup = model.mixup_alpha != 0
    # the step's mixup draws: static device tensors the (captured) step reads, rewritten before every step
    lam_t = torch.ones((), dtype=torch.float32, device=dev)
    index_t = torch.arange(bsz, dtype=torch.int64, device=dev)
    last = {}

    def train_step(codes, cond=None):  # cond: the captured step's second static input
        opt.zero_grad()
        rows, _ = model.loss_rows(onehot_codes(codes, k), codes, (lam_t, index_t) if mixup else None, **_cond_kw(cond))
        loss = rows.mean()
        scaler.scale(loss).backward()
        reducer()
        scaler.step(opt)
        scaler.update()
        last["rows"] = rows.detach()  # a captured step's tensor: every replay rewrites it in place
        return loss
    use_graph = bool(getattr(args, "hip_graph", 1)) and (
        world == 1 or (torch.distributed.get_backend() == "nccl" and parallel.graph_collectives_ok(dev)))
    runner = StepGraph(train_step, warmup=2, enabled=use_graph)
    val_every = max(1, int(n_batches * args.val_check_interval)) if args.val_check_interval <= 1 else \
        int(args.val_check_interval)
    history = []
    epoch = epoch0
    for epoch in range(epoch0, args.max_epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        for i, batch in enumerate(loader):
            codes, cond = _codes(batch, dev), _condition(batch, dev, model)
            if mixup:
                lam, index = mixup_draw(bsz, model.mixup_alpha)
                lam_t.copy_(torch.tensor(lam, dtype=torch.float32), non_blocking=True)
                index_t.copy_(index.to(torch.int64), non_blocking=True)
            runner(*((codes,) if cond is None else (codes, cond)))
            step += 1
            if step % args.log_every_n_steps == 0 or step == 1:
                log = {name: float(v) for name, v in loss_metrics(last["rows"], "train").items()}
                history.append((step, log))
                if rank == 0:
                    print(f"epoch {epoch} step {step} " + " ".join(f"{n} {v:.6f}" for n, v in log.items()), flush=True)
            if (i + 1) % val_every == 0 or (i + 1) == n_batches:
                score = validate(model, vloader, dev) if len(vloader) else None
                if rank == 0 and score is not None:
                    vals = " ".join(f"{n} {v:.6f}" for n, v in model.val_metrics.items())
                    print(f"epoch {epoch} step {step} {vals}", flush=True)
                if rank == 0:  # PL's global_step is still this batch's 0-based index here
                    ckpt(model, opt, epoch, step - 1, score, args.max_steps, scaler)
            if args.max_steps is not None and step >= args.max_steps:
                break
        if args.max_steps is not None and step >= args.max_steps:
            break
    if rank == 0 and step > 0:  # training ended (max_steps / max_epochs): last.ckpt holds the final state
        ckpt(model, opt, epoch, step - 1, None, args.max_steps, scaler)
    return model, opt, history, ckpt


def cli(argv=None, datamodule=None, parse=None, module="vq3d.train_prior", model_cls=PixelSNAIL):
    """The command: the ranks' exit code when it started them (--gpus > 1), else main's
    (model, optimizer, log history, checkpointer) of the run in this process."""
    import sys
    argv = sys.argv[1:] if argv is None else argv
    args = (parse or parse_arguments)(argv)
    rc = T.launch_ranks(args, argv, module=module)
    if rc is not None:
        return rc
    return main(args, datamodule, model_cls)


if __name__ == "__main__":
    _rc = cli()
    raise SystemExit(_rc if isinstance(_rc, int) else 0)
