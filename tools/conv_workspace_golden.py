#!/usr/bin/env python3
"""Record vq3d_conv3d_workspace_size (forward, backward-data, weight pass) of the built library
for every conv descriptor of one training step of the published 3-level model (3l_pub, 512 x 512
x 128) and of the 2-layer default (32^3), in bf16, fp16 and fp32, plus the engine table of
tests/test_conv_routes_cpu.py, into tests/golden/conv_workspace_parent.json.  No GPU: the host
path runs on CPU tensors with the C-ABI calls recorded instead of executed (as
tools/layer_inventory.py does); the size query is host planning.

Run it BEFORE a change to the conv routing; tests/test_conv_routes_cpu.py then holds the changed
library to the recorded sizes.

    python3 tools/conv_workspace_golden.py"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-vq-vae-2_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from test_conv_routes_cpu import FIELDS, table_descs  # noqa: E402
from vq3d import _lib as L  # noqa: E402

descs = {}  # descriptor fields -> name


def name_of(f):
    d = dict(zip(FIELDS, f))
    return (f"{('f32', 'bf16', 'f16')[d['dtype']]} b{d['batch']} {d['cin']}+{d['cin2']}->{d['cout']} k{d['kernel']} "
            f"s{d['stride']} p{d['pad']} {'circ' if d['pad_mode'] else 'zero'} @{d['in_h']}x{d['in_w']}x{d['in_d']} "
            f"pro{d['pro_kind']} taps{d['tap_mask']}")


def fake_call(name, *args):
    if name.startswith("vq3d_conv3d"):
        f = tuple(int(getattr(args[0]._obj, n)) for n in FIELDS)
        descs.setdefault(f, name_of(f))
    return 0


def main():
    import vq3d
    from vq3d import functional as F
    real_call = L.call
    L.call, L.ptr, L.stream = fake_call, (lambda t: t.data_ptr()), (lambda: None)
    F.grad_buf = lambda p: torch.zeros_like(p) if p is not None else None
    runs = [(bench.CONFIGS["3l_pub"][0], bench.CONFIGS["3l_pub"][1]), (dict(n_bottleneck_blocks=2), (32, 32, 32))]
    for mkw, size in runs:
        for dt in ("bf16", "fp16", "fp32"):
            model = vq3d.VQVAE(vq3d.default_args(compute_dtype=dt, **mkw))
            x = torch.rand((1, 1) + tuple(size)) * 4.5 - 0.5
            loss = model.training_step((x, torch.full((1,), size[2], dtype=torch.int64)), 0)
            loss.backward()
    L.call = real_call
    entries = [(n, f) for f, n in sorted(descs.items(), key=lambda kv: kv[1])]
    entries += [("table: " + n, tuple(int(getattr(d, k)) for k in FIELDS)) for n, d, _ in table_descs()]
    out = []
    for n, f in entries:
        d = L.ConvDesc(**dict(zip(FIELDS, f)))
        out.append({"name": n, "desc": list(f),
                    "bytes": [int(L.query("vq3d_conv3d_workspace_size", ctypes.byref(d), p)) for p in (0, 1, 2)]})
    path = os.path.join(ROOT, "tests", "golden", "conv_workspace_parent.json")
    with open(path, "w") as fh:
        fh.write('{"fields": %s,\n "entries": [\n' % json.dumps(list(FIELDS)))
        fh.write(",\n".join("  " + json.dumps(e) for e in out))
        fh.write("\n]}\n")
    print(f"{len(out)} entries -> {path}")


if __name__ == "__main__":
    main()
