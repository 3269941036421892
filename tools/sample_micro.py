#!/usr/bin/env python3
"""Time prior sampling (vq3d.sample.sample_codes) at the published mid prior: model_dim 256, 8 blocks
x 5 layers, K = 256 (bench.py's PRIOR), bf16, batch 1, freshly initialised and perturbed weights.

    python3 tools/sample_micro.py [--size D H W]... [--variants naive eager graphs] [--out FILE.json]

Seconds per sample batch (one volume of D x H x W codes) of three forms:
  naive   the reference's shape of the loop: one full-grid forward with full logits per position, the
          row picked out and drawn with F.gumbel_softmax(hard=True).  Every position costs the same,
          so NAIVE_POSITIONS positions are timed and scaled by (D H W) / NAIVE_POSITIONS;
  eager   sample_codes: slab-prefix forward + the fused head-and-draw kernel per position;
  graphs  sample_codes(graphs=True): the same, one captured HIP graph per slab count; the captures'
          time (warm-up included) is reported apart and is part of the total.
A host clock around each whole run, device-synchronised at both ends, after a warm-up run of the same
form on the grid's first two slabs.  eager and graphs are whole runs and must give the same codes.
With --out the document is written there; an existing document keeps its other sizes.
Fails without a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-vq-vae-2_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PRIOR = dict(num_embeddings=[256, 0], model_dim=256, num_blocks=8, num_layers_per_block=5, bottleneck_divisor=4)
NAIVE_POSITIONS = 64
CL = torch.channels_last_3d


def make_model(dev):
    from vq3d import pixelsnail as PS
    torch.manual_seed(0)
    m = PS.PixelSNAIL(PS.default_args(**PRIOR), compute_dtype="bf16")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # branch_conv3 is zero at initialisation: perturb, so the logits depend on the input
        for _, p in sorted(m.named_parameters()):
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    return m.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


@torch.no_grad()
def naive_positions(m, size, npositions):
    """the first npositions positions of the naive loop (full forward + full logits each)"""
    d, h, w = size
    k = m.input_dim
    x = torch.zeros((1, k, d, h, w), dtype=m.compute_dtype, device="cuda").contiguous(memory_format=CL)
    flat = x.permute(0, 2, 3, 4, 1).reshape(1, d * h * w, k)
    for p in range(npositions):
        row = m.logits(x).permute(0, 2, 3, 4, 1).reshape(1, d * h * w, k)[:, p]
        flat[:, p] = F.gumbel_softmax(row, tau=1.0, hard=True, dim=1).to(x.dtype)
    return flat[:, :npositions].argmax(-1)


def bench_size(m, size, variants):
    from vq3d import sample as S
    d, h, w = size
    npos = d * h * w
    warm = (min(d, 2), h, w)
    out = {"size": list(size), "positions": npos, "batch": 1, "dtype": "bf16"}
    codes = {}
    if "naive" in variants:
        naive_positions(m, size, 2)
        t, _ = timed(lambda: naive_positions(m, size, NAIVE_POSITIONS))
        out["naive"] = {"timed_positions": NAIVE_POSITIONS, "timed_s": t, "ms_per_position": 1e3 * t / NAIVE_POSITIONS,
                        "seconds_per_sample_batch_scaled": t * npos / NAIVE_POSITIONS}
    if "eager" in variants:
        S.sample_codes(m, warm, seed=1)
        t, codes["eager"] = timed(lambda: S.sample_codes(m, size, seed=1))
        out["eager"] = {"seconds_per_sample_batch": t, "ms_per_position": 1e3 * t / npos}
    if "graphs" in variants:
        capture, spent = S._capture, []

        def timed_capture(*a):
            t, r = timed(lambda: capture(*a))
            spent.append(t)
            return r
        S._capture = timed_capture
        try:
            S.sample_codes(m, warm, seed=1, graphs=True)
            spent.clear()
            t, codes["graphs"] = timed(lambda: S.sample_codes(m, size, seed=1, graphs=True))
        finally:
            S._capture = capture
        out["graphs"] = {"seconds_per_sample_batch": t, "of_which_capture_s": spent[0], "graphs": d,
                         "ms_per_position_replay": 1e3 * (t - spent[0]) / npos}
    for name in variants:  # progress, one line per form
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    if len(codes) == 2:
        out["graphs_equal_eager"] = bool(torch.equal(codes["eager"], codes["graphs"]))
    if codes:
        c = next(iter(codes.values()))
        out["distinct_codes"] = int(torch.unique(c).numel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, action="append", metavar=("D", "H", "W"))
    ap.add_argument("--variants", nargs="+", default=["naive", "eager", "graphs"], choices=["naive", "eager", "graphs"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_micro: needs a GPU (nothing is measured without one)")
    sizes = [tuple(s) for s in (a.size or [[16, 16, 8], [32, 32, 8]])]
    m = make_model(torch.device("cuda:0"))
    doc = {"device": torch.cuda.get_device_name(0), "model": PRIOR, "sizes": {}}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc["sizes"] = json.load(f).get("sizes", {})
    for s in sizes:
        key = "x".join(str(v) for v in s)
        doc["sizes"][key] = {**doc["sizes"].get(key, {}), **bench_size(m, s, a.variants)}
        text = json.dumps(doc, indent=1)
        if a.out:  # after every size: a later size that runs out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
