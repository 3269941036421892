#!/usr/bin/env python3
"""Time the fused validation-metrics kernel (vq3d.metrics.slice_metrics, csrc/metrics.hip) against a
torch-on-GPU formulation of the same definition (rearrange to (B D, 1, H, W) + F.conv2d).

    python3 tools/metrics_micro.py [--rounds N] [--step] [--out FILE.json]

Sizes: 512 x 512 x 128 at batch 1 and 256 x 256 x 128 at batch 2, bf16 decoder output, fp32 target.
Both forms are warmed at every size, then timed alternately in one process with device events
(`rounds` windows each; a window is many back-to-back calls, the kernel's replayed from a HIP graph
so that its host side is not what is timed); the median window is reported.  Prints
one JSON document: per size the kernel time with an explicit data range (the fused pass alone) and
with a computed one (plus the min / max pass), the torch time, the kernel's algorithmic bytes
B H W D (sizeof(pred) + 4) and bytes / s as a share of the measured 6.29 TB/s copy rate.
--step also times one validation_step of the benchmark's flagship model at 512 x 512 x 128 with the
metrics and with the metrics pass bypassed (the step the model ran before it logged them).
Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-vq-vae-2_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, the measured device copy rate
SIZES = [(1, 512, 512, 128), (2, 256, 256, 128)]


def make_inputs(shape, dev, seed=0):
    b, h, w, d = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    field = torch.rand((b, 1, h // 8 + 1, w // 8 + 1, d // 8 + 1), generator=g, device=dev) * 4.5 - 0.5
    x = F.interpolate(field, size=(h, w, d), mode="trilinear", align_corners=True).contiguous()
    pred = (x + 0.1 * torch.randn(x.shape, generator=g, device=dev)).to(torch.bfloat16)
    nvs = torch.full((b,), d - 3, dtype=torch.int64, device=dev)
    return pred, x, nvs


def torch_metrics(pred, x, nvs, data_range, window):
    """The same figures in torch ops: {ssim, mse, nmse, psnr} as a 4-vector."""
    b, _, h, w, d = pred.shape
    p = F.elu(pred.float())
    p = p * (torch.arange(d, device=p.device).view(1, 1, 1, 1, d) < nvs.view(b, 1, 1, 1, 1))
    rng = torch.maximum(p.max() - p.min(), x.max() - x.min()) if data_range is None else \
        torch.tensor(data_range, device=p.device)
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    ps, ts = (v.permute(0, 4, 1, 2, 3).reshape(b * d, 1, h, w) for v in (p, x))
    q = F.conv2d(torch.cat([ps, ts, ps * ps, ts * ts, ps * ts], dim=1), window, groups=5)
    mp, mt, epp, ett, ept = q.unbind(1)
    smap = ((2 * mp * mt + c1) * (2 * (ept - mp * mt) + c2)) / \
        ((mp * mp + mt * mt + c1) * ((epp - mp * mp) + (ett - mt * mt) + c2))
    sse, st2 = ((p - x) ** 2).sum(), (x * x).sum()
    mse = sse / p.numel()
    return torch.stack([smap.mean(dim=(1, 2)).mean(), mse, sse / st2, 10 * torch.log10(16.0 / mse)])


def window_ms(fn, reps):
    """milliseconds per call over one window of `reps` back-to-back calls (device events)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def graphed(fn, calls):
    """`calls` back-to-back launches of fn as one HIP graph, so the host side (Python, ctypes) of a
    sub-millisecond call is not what the window measures: (replay, calls)"""
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    return graph.replay, calls


def alternate(forms, rounds):
    """forms: {name: (fn, calls per fn, fn calls per window)}; every round times each form once, in turn"""
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, (fn, calls, reps) in forms.items():
            times[k].append(window_ms(fn, reps) / calls)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v),
                "calls_per_window": forms[k][1] * forms[k][2]} for k, v in times.items()}


def bench_size(shape, dev, rounds):
    from vq3d.metrics import gaussian_window, slice_metrics
    pred, x, nvs = make_inputs(shape, dev)
    g = gaussian_window(device=dev)
    window = (g.view(-1, 1) * g.view(1, -1)).view(1, 1, 11, 11).repeat(5, 1, 1, 1)
    forms = {
        "kernel_explicit_range": (lambda: slice_metrics(pred, x, nvs, activation="elu", data_range=4.24), 1, 1),
        "kernel_computed_range": (lambda: slice_metrics(pred, x, nvs, activation="elu"), 1, 1),
        "torch_explicit_range": (lambda: torch_metrics(pred, x, nvs, 4.24, window), 1, 10),
        "torch_computed_range": (lambda: torch_metrics(pred, x, nvs, None, window), 1, 10),
    }
    for fn, _, _ in forms.values():  # warm every form at this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for k in ("kernel_explicit_range", "kernel_computed_range"):
        forms[k] = graphed(forms[k][0], 50) + (8,)
    q = slice_metrics(pred, x, nvs, activation="elu")
    t = torch_metrics(pred, x, nvs, None, window)
    res = alternate(forms, rounds)
    nbytes = pred.numel() * (pred.element_size() + 4)
    out = {"shape": list(shape), "pred_dtype": "bf16", "algorithmic_bytes": nbytes, "times": res,
           "kernel_values": [float(v) for v in (q.ssim, q.mse, q.nmse, q.psnr)], "torch_values": t.tolist()}
    for k in ("kernel_explicit_range", "kernel_computed_range"):
        rate = nbytes / (res[k]["median_ms"] * 1e-3)
        out[k + "_bytes_per_s"] = rate
        out[k + "_share_of_copy_rate"] = rate / COPY_RATE
    out["speedup_explicit"] = res["torch_explicit_range"]["median_ms"] / res["kernel_explicit_range"]["median_ms"]
    out["speedup_computed"] = res["torch_computed_range"]["median_ms"] / res["kernel_computed_range"]["median_ms"]
    return out


def bench_step(dev, rounds):
    import vq3d
    from bench import CONFIGS
    from vq3d.utils import synthetic_volume
    mkw, size, batch, _ = CONFIGS["3l_pub"]
    torch.manual_seed(0)
    m = vq3d.VQVAE(vq3d.default_args(compute_dtype="bf16", **mkw)).to(dev).eval()
    x = torch.cat([synthetic_volume((1, 1) + size, i) for i in range(batch)]).to(dev)
    nvs = torch.full((batch,), size[2], dtype=torch.int64, device=dev)

    def step(quality):
        with torch.no_grad():
            m.recon_loss_f((x, nvs), 0, quality=quality)
    forms = {"validation_step_with_metrics": (lambda: step(True), 1, 3),
             "validation_step_metrics_bypassed": (lambda: step(False), 1, 3)}
    for fn, _, _ in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    return {"config": "3l_pub", "shape": [batch, *size], "dtype": "bf16", "times": alternate(forms, rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_micro: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE,
           "sizes": [bench_size(s, dev, a.rounds) for s in SIZES]}
    if a.step:
        doc["validation_step"] = bench_step(dev, max(3, a.rounds // 2))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
