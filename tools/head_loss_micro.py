#!/usr/bin/env python3
"""Time the prior's fused output head + loss (vq3d.head_loss, forward + backward) against today's chain
on the same operands -- pixelsnail.pointwise -> .float() -> F.cross_entropy and its autograd backward,
as PixelSNAIL.cross_entropy_onehot runs it -- and record each one's peak memory.

    python tools/head_loss_micro.py [--out profiles/head_loss_micro.json] [--calls 50] [--rounds 10]

Shapes (bf16): the published mid level (8,192 rows, c 256, K 256) and a bottom-like one (65,536 rows,
c 256, K 512), each with one target and with mixup's two.  Every variant is captured once as a HIP graph
(forward, mean, backward to the rows, weight and bias) so the host's launch cost is out of the window; a
window is `calls` replays between two device events, the variants' windows alternate `rounds` times
in one process, and the medians and the spread (min, max) of the windows are reported.  Peak memory is
torch.cuda.max_memory_allocated over one eager call, above what was allocated before it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-vq-vae-2_amd"))

SHAPES = {"mid": (8192, 256, 256), "bottom_like": (65536, 256, 512)}
LAM = 0.3


def operands(n, c, k, dev):
    import torch
    g = torch.Generator().manual_seed(1000 * k + c)
    h = torch.randn((n, c), generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    w = (torch.randn((k, c), generator=g) * (4.0 / c ** 0.5)).to(dev).requires_grad_(True)
    b = torch.randn(k, generator=g).to(dev).requires_grad_(True)
    ta = torch.randint(0, k, (n,), generator=g).to(dev)
    tb = torch.randint(0, k, (n,), generator=g).to(dev)
    return h, w, b, ta, tb


def variants(n, c, k, two, dev):
    import torch
    import torch.nn.functional as F

    from vq3d import pixelsnail as PS
    from vq3d.head_loss import head_loss
    h, w, b, ta, tb = operands(n, c, k, dev)
    lam_t = torch.tensor(LAM, dtype=torch.float32, device=dev)

    def fused():
        loss, _ = head_loss(h, w, b, ta, tb if two else None, lam_t if two else None)
        m = loss.mean()
        return (m,) + torch.autograd.grad(m, (h, w, b))

    def chain(rows_form=False):
        x5 = h.view(1, n, 1, 1, c).permute(0, 4, 1, 2, 3)
        logits = PS.pointwise(x5, w, b).float()  # (1, K, n, 1, 1): the class axis is dim 1, as in the model
        t1, t2 = ta.view(1, n, 1, 1), tb.view(1, n, 1, 1)
        if rows_form:
            logits, t1, t2 = logits.permute(0, 2, 3, 4, 1).reshape(n, k), ta, tb
        rows = F.cross_entropy(logits, t1, reduction="none")
        if two:
            rows = LAM * rows + (1 - LAM) * F.cross_entropy(logits, t2, reduction="none")
        m = rows.mean()
        return (m,) + torch.autograd.grad(m, (h, w, b))
    # chain: what PixelSNAIL.cross_entropy_onehot runs today; chain_rows: the same ops on (n, K) logits, for
    # information (torch's row softmax instead of its spatial one)
    return {"fused": fused, "chain": chain, "chain_rows": lambda: chain(True)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_loss_micro.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("head_loss_micro needs the GPU: there is no CPU timing of these kernels")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "calls_per_window": a.calls, "rounds": a.rounds,
           "unit": "microseconds per forward + backward (graph replay, device events)", "cases": []}
    for name, (n, c, k) in SHAPES.items():
        for two in (False, True):
            fns = variants(n, c, k, two, dev)
            peaks = {v: peak_bytes(f) for v, f in fns.items()}
            graphs = {v: capture(f) for v, f in fns.items()}
            for g, _ in graphs.values():  # warm the replays (a capture computes nothing: the outputs exist from here)
                window(g, 5)
            diff = {i: float((graphs["fused"][1][i].float() - graphs["chain"][1][i].float()).abs().max())
                    for i in range(4)}
            wins = {v: [] for v in fns}
            for _ in range(a.rounds):
                for v in fns:
                    wins[v].append(window(graphs[v][0], a.calls))
            case = {"shape": name, "nrows": n, "c": c, "k": k, "targets": 2 if two else 1,
                    "max_abs_difference": dict(zip(("loss_mean", "dhidden", "dweight", "dbias"), diff.values()))}
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
