#!/usr/bin/env python3
"""One training step of the published mid-level conditioned PixelCNN prior (slurm-jobs/train_pixelcnn_mid.job:
45 resblocks, model-dim 256, dropout 0.5, mixup alpha 1 (the default), batch 2; codes 32x32x8 conditioned on
8x8x2, K = Kc = 512) as vq3d.train_pixelcnn runs it: device-side mixup draws, loss_rows through the fused head,
FusedAdam over FlatParams, captured as one HIP graph.  Reports ms per step and peak memory.

    python tools/pixelcnn_step.py [--out profiles/pixelcnn_mid_step.json] [--steps 10] [--rounds 5] [--dtype bf16]

A window is `steps` replays between two device events; the median and spread of `rounds` windows are reported.
Peak memory is torch.cuda.max_memory_allocated over the eager warm-up steps and the capture.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-vq-vae-2_amd"))

CFG = dict(num_embeddings=[512, 512], model_dim=256, num_resblocks=45, dropout_prob=0.5, use_pre_activation=True,
           use_conditioning=True, bottleneck_divisor=4, mixup_alpha=1.0, lr=1e-4)
DIMS, CDIMS, BATCH = (32, 32, 8), (8, 8, 2), 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixelcnn_mid_step.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pixelcnn_step needs the GPU")
    from vq3d import pixelcnn as PC
    from vq3d.flat import FlatParams
    from vq3d.graph import StepGraph
    from vq3d.optim import FusedAdam, GradScaler
    from vq3d.pixelsnail import mixup_draw
    from vq3d.train_prior import onehot_codes
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    model = PC.PixelCNN(PC.default_args(**CFG), compute_dtype=a.dtype).to(dev)
    model.train()
    flat = FlatParams(model.parameters(), dev)
    opt = FusedAdam(model.parameters(), flat, lr=CFG["lr"], amsgrad=True)
    scaler = GradScaler(dev, enabled=a.dtype == "fp16")
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, CFG["num_embeddings"][0], (BATCH,) + DIMS, generator=g).to(dev)
    cond = torch.randint(0, CFG["num_embeddings"][1], (BATCH,) + CDIMS, generator=g).to(dev)
    lam_t = torch.ones((), dtype=torch.float32, device=dev)
    index_t = torch.arange(BATCH, dtype=torch.int64, device=dev)

    def train_step(codes, cond):
        opt.zero_grad()
        rows, _ = model.loss_rows(onehot_codes(codes, model.input_dim), codes, (lam_t, index_t), condition=cond)
        loss = rows.mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss
    runner = StepGraph(train_step, warmup=2)

    def one():
        lam, index = mixup_draw(BATCH, CFG["mixup_alpha"])
        lam_t.copy_(torch.tensor(lam, dtype=torch.float32), non_blocking=True)
        index_t.copy_(index.to(torch.int64), non_blocking=True)
        return runner(codes, cond)
    torch.cuda.reset_peak_memory_stats()
    for _ in range(4):  # two eager steps, the capture, one replay
        loss = one()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated())
    wins = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            loss = one()
        e1.record()
        e1.synchronize()
        wins.append(e0.elapsed_time(e1) / a.steps)
    res = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "config": {**CFG, "codes": list(DIMS),
                                                                                 "condition": list(CDIMS), "batch": BATCH},
           "parameters": int(sum(p.numel() for p in model.parameters())), "launch": "hip_graph",
           "ms_per_step_median": statistics.median(wins), "ms_per_step_min": min(wins), "ms_per_step_max": max(wins),
           "steps_per_window": a.steps, "rounds": a.rounds, "peak_bytes": peak, "final_loss": float(loss)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
