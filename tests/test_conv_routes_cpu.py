"""CPU: the conv route (csrc/conv3d.hip `route`): which engine a descriptor reaches, as
vq3d_conv3d_engine reports it, and that vq3d_conv3d_workspace_size still answers what it answered
before the route existed (tests/golden/conv_workspace_parent.json, recorded with the library of
the commit before: every conv descriptor of one training step of the published 3-level model and
of the 2-layer default, in bf16, fp16 and fp32, plus the table below;
tools/conv_workspace_golden.py rewrites it).  Host planning only: no GPU is touched."""
import ctypes
import json
import os

import pytest

from conftest import GOLDEN

FWD, DGRAD, WGRAD = 0, 1, 2
F32, BF16, F16 = 0, 1, 2
HALF = (BF16, F16)
FIELDS = ("dtype", "batch", "cin", "cin2", "cout", "in_h", "in_w", "in_d", "out_h", "out_w", "out_d", "kernel",
          "stride", "pad", "pad_mode", "pro_kind", "tap_mask")

# (name, dtypes, cin, cout, input (h, w, d), k, s, p, circular, {pass: engine}): for every engine the
# smallest descriptor found that reaches it (batch 1, no second input, no prologue)
ENGINE_TABLE = [
    ("2->2 k3 circ @8x8x32", HALF + (F32,), 2, 2, (8, 8, 32), 3, 1, 1, True, {FWD: "tc", DGRAD: "tc", WGRAD: "tc_wgrad"}),
    # no 8 x 8 x 32 brick: the lines engine
    ("2->2 k3 circ @8x8x16", HALF, 2, 2, (8, 8, 16), 3, 1, 1, True, {FWD: "lines", DGRAD: "lines"}),
    ("4->4 k3 circ @8x8x64", HALF, 4, 4, (8, 8, 64), 3, 1, 1, True, {FWD: "lines", DGRAD: "lines", WGRAD: "gen_mfma"}),
    ("4->4 k3 circ @8x8x64", (F32,), 4, 4, (8, 8, 64), 3, 1, 1, True, {FWD: "valu", DGRAD: "valu", WGRAD: "valu_wgrad"}),
    ("9->9 k3 circ @16x16x16", HALF, 9, 9, (16, 16, 16), 3, 1, 1, True, {WGRAD: "mid_w2grad"}),
    ("36->36 k3 circ @32x32x8", HALF, 36, 36, (32, 32, 8), 3, 1, 1, True, {FWD: "lines", WGRAD: "lines_wgrad"}),
    ("128->128 k3 circ @8x8x2", HALF, 128, 128, (8, 8, 2), 3, 1, 1, True,
     {FWD: "small", DGRAD: "small", WGRAD: "gen_tiled"}),
    ("128->128 k3 circ @8x8x2", (F32,), 128, 128, (8, 8, 2), 3, 1, 1, True,
     {FWD: "small", DGRAD: "small", WGRAD: "valu_wgrad"}),
    ("32->32 k4 s2 circ @8x8x2", HALF, 32, 32, (8, 8, 2), 4, 2, 1, True, {DGRAD: "small"}),
    # more than 512 input voxels: the parity-tap engine, both storage types
    ("16->16 k4 s2 circ @16x16x4", HALF + (F32,), 16, 16, (16, 16, 4), 4, 2, 1, True, {DGRAD: "s2"}),
    # wgrad_ds has an instance for 4 -> 4 k4 s2 at output depth 64 only
    ("4->4 k4 s2 circ @8x8x128", HALF, 4, 4, (8, 8, 128), 4, 2, 1, True, {WGRAD: "wgrad_ds"}),
    ("4->4 k4 s2 circ @64x64x16", HALF, 4, 4, (64, 64, 16), 4, 2, 1, True, {WGRAD: "gen_mfma"}),
    ("18->9 k1 @16x16x16", HALF + (F32,), 18, 9, (16, 16, 16), 1, 1, 0, False,
     {FWD: "pointwise", DGRAD: "pointwise", WGRAD: "pw_wgrad"}),
    # too few voxels x outputs for the small-grid engine and, from 161 reduction channels on at 2x2x2,
    # too many channels for the lines planner: the direct MFMA engine
    ("161->4 k3 zero @2x2x2", HALF, 161, 4, (2, 2, 2), 3, 1, 1, False, {FWD: "mfma"}),
    ("4->161 k3 zero @2x2x2", HALF, 4, 161, (2, 2, 2), 3, 1, 1, False, {DGRAD: "mfma"}),
]

# Forward sizes that may exceed the recorded ones: the tc-shaped 16-bit descriptors, whose size now
# also covers the call with an upsampled residual (it runs on the lines engine, which packs
# weights).  A closed set of golden entry names; every other entry must match to the byte.
FWD_GROWTH = {
    "bf16 b1 2+0->2 k3 s1 p1 circ @128x128x32 pro0 taps0",
    "f16 b1 2+0->2 k3 s1 p1 circ @128x128x32 pro0 taps0",
    "table: 2->2 k3 circ @8x8x32 bf16",
    "table: 2->2 k3 circ @8x8x32 f16",
}


def make_desc(dtype, cin, cout, hwd, k, s, p, circ, batch=1):
    from vq3d import _lib as L
    out = [(n + 2 * p - k) // s + 1 for n in hwd]
    return L.ConvDesc(dtype=dtype, batch=batch, cin=cin, cin2=0, cout=cout, in_h=hwd[0], in_w=hwd[1], in_d=hwd[2],
                      out_h=out[0], out_w=out[1], out_d=out[2], kernel=k, stride=s, pad=p, pad_mode=int(circ),
                      pro_kind=0, tap_mask=0)


def engine(desc, pass_):
    from vq3d import _lib as L
    return L.query("vq3d_conv3d_engine", ctypes.byref(desc), pass_).decode()


def table_descs():
    """(name with dtype, descriptor, expectations) of every table row and dtype"""
    for name, dtypes, cin, cout, hwd, k, s, p, circ, expect in ENGINE_TABLE:
        for dt in dtypes:
            yield f"{name} {('f32', 'bf16', 'f16')[dt]}", make_desc(dt, cin, cout, hwd, k, s, p, circ), expect


@pytest.mark.parametrize("name,desc,expect", [pytest.param(*t, id=t[0]) for t in table_descs()])
def test_engine_table(name, desc, expect):
    for pass_, want in expect.items():
        assert engine(desc, pass_) == want, (name, pass_)


def test_table_reaches_every_engine():
    seen = {e for _, _, expect in table_descs() for e in expect.values()}
    assert seen == {"pointwise", "tc", "small", "lines", "mfma", "s2", "valu", "pw_wgrad", "tc_wgrad",
                    "mid_w2grad", "wgrad_ds", "lines_wgrad", "gen_mfma", "gen_tiled", "valu_wgrad"}


def test_engine_query_refuses_bad_input():
    d = make_desc(BF16, 4, 4, (8, 8, 8), 3, 1, 1, True)
    assert engine(d, 3) == "" and engine(d, -1) == ""
    d.out_h = 9
    assert engine(d, FWD) == ""


def test_workspace_sizes_match_parent():
    from vq3d import _lib as L
    entries = json.load(open(os.path.join(GOLDEN, "conv_workspace_parent.json")))["entries"]
    assert len(entries) > 100
    assert FWD_GROWTH <= {e["name"] for e in entries}
    bad = []
    for e in entries:
        desc = L.ConvDesc(**dict(zip(FIELDS, e["desc"])))
        got = [int(L.query("vq3d_conv3d_workspace_size", ctypes.byref(desc), p)) for p in (FWD, DGRAD, WGRAD)]
        want = list(e["bytes"])
        if e["name"] in FWD_GROWTH:
            assert engine(desc, FWD) == "tc" and got[0] > want[0], e["name"]
            want[0] = got[0]
        if got != want:
            bad.append((e["name"], want, got))
    assert not bad, bad
