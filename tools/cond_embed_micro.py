#!/usr/bin/env python3
"""Time the conditioned PixelCNN's fused condition embedding (vq3d.cond_embed, forward + backward) against the
unfused chain on the same operands -- one-hot of the condition codes -> F.interpolate(trilinear) [-> mixup's
blend] -> pixelsnail.pointwise (embed_condition) and its autograd backward, as the reference's
PixelCNN.cross_entropy + forward run it -- and record each one's peak memory.

    python tools/cond_embed_micro.py [--out profiles/cond_embed_micro.json] [--calls 20] [--rounds 10]

Shapes (bf16, batch 2): the published mid level (codes 32x32x8 conditioned on 8x8x2, Kc 512, M 256) and a
bottom-like one (64x64x16 on 16x16x4, Kc 256, M 512), each without and with mixup.  Every variant is captured
once as a HIP graph (forward, a weighted sum, backward to the weight and bias) so the host's launch cost is
out of the window; a window is `calls` replays between two device events, the variants' windows alternate
`rounds` times in one process, and the medians and the spread (min, max) of the windows are reported.  Peak
memory is torch.cuda.max_memory_allocated over one eager call, above what was allocated before it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-vq-vae-2_amd"))

# name: (data grid, condition grid, Kc, M)
SHAPES = {"mid": ((32, 32, 8), (8, 8, 2), 512, 256), "bottom_like": ((64, 64, 16), (16, 16, 4), 256, 512)}
BATCH, LAM = 2, 0.3


def variants(dims, cdims, kc, m, mix, dev):
    import torch
    import torch.nn.functional as F

    from vq3d import pixelsnail as PS
    from vq3d.cond_embed import cond_embed
    PS._compute[0] = torch.bfloat16
    g = torch.Generator().manual_seed(kc + m)
    codes = torch.randint(0, kc, (BATCH,) + cdims, generator=g).to(dev)
    w = (torch.randn((m, kc, 1, 1, 1), generator=g) * 0.5).to(dev).requires_grad_(True)
    b = torch.randn(m, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn((BATCH, m) + dims, generator=g).to(torch.bfloat16).to(dev).contiguous(
        memory_format=torch.channels_last_3d)
    lam_t = torch.tensor(LAM, dtype=torch.float32, device=dev)
    index_t = torch.tensor([1, 0], dtype=torch.int64, device=dev)

    def fused():
        e = cond_embed(codes, w, b, dims, lam_t if mix else None, index_t if mix else None, dtype=torch.bfloat16)
        return (e,) + torch.autograd.grad(e, (w, b), gy)

    def chain():
        oh = torch.zeros((BATCH, kc) + cdims, dtype=torch.float32, device=dev).scatter_(1, codes.unsqueeze(1), 1.0)
        it = F.interpolate(oh, size=dims, mode="trilinear")
        if mix:
            it = lam_t * it + (1 - lam_t) * it[index_t]
        e = PS.pointwise(PS.cl(it.to(torch.bfloat16)), w, b)
        return (e,) + torch.autograd.grad(e, (w, b), gy)
    return {"fused": fused, "chain": chain}


def capture(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def window(graph, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_embed_micro.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cond_embed_micro needs the GPU: there is no CPU timing of these kernels")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "batch": BATCH, "calls_per_window": a.calls,
           "rounds": a.rounds, "unit": "microseconds per forward + backward (graph replay, device events)", "cases": []}
    for name, (dims, cdims, kc, m) in SHAPES.items():
        for mix in (False, True):
            fns = variants(dims, cdims, kc, m, mix, dev)
            peaks = {v: peak_bytes(f) for v, f in fns.items()}
            graphs = {v: capture(f) for v, f in fns.items()}
            for g, _ in graphs.values():  # warm the replays (a capture computes nothing: the outputs exist from here)
                window(g, 3)
            diff = [float((graphs["fused"][1][i].float() - graphs["chain"][1][i].float()).abs().max()) for i in range(3)]
            wins = {v: [] for v in fns}
            for _ in range(a.rounds):
                for v in fns:
                    wins[v].append(window(graphs[v][0], a.calls))
            case = {"shape": name, "grid": list(dims), "condition_grid": list(cdims), "kc": kc, "m": m, "mixup": mix,
                    "max_abs_difference": dict(zip(("e", "dweight", "dbias"), diff))}
            for v in fns:
                case[v] = {"median_us": statistics.median(wins[v]), "min_us": min(wins[v]), "max_us": max(wins[v]),
                           "peak_bytes": peaks[v]}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
            del graphs, fns
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
