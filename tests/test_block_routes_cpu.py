"""CPU: the fused PreAct route (vq3d.functional.run_route / block_path): which engine a run of identical
blocks and which path a single block reach, as pure functions of (dtype, shape, block) over the library's
host-only *_supported / *_plan queries.  The expectations were recorded with the predicates of the commit
before the route existed (layers.BlockStack's if-chain and _stack_ok, functional.*_eligible, the conditions
of PreActBlockFn.forward), evaluated on the same shapes; a sweep of 85,000 (toggle, dtype, class, mode, grid,
run length, small_only) combinations gave the same answers from both, with the same number of host queries.
Host planning only: no GPU is touched."""
import pytest
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALF = (BF16, F16)
ALL = HALF + (F32,)

# (dtypes, C (branch = C // 2), block kind, grid (h, w, d), run length, small_only, run route, block path):
# kind "same" | "down" | "up" as the block's mode, "skip": mode "same" with a skip conv (C -> 2C); the block
# path (rows of run length 1) is block_path's answer, "small" with the backward it takes ("small+fused":
# the fused kernels, "small+convs": the per-conv backward from the saved t2 / t3); batch 1.
ROUTE_TABLE = [
    # the published 3-level model's classes as runs of 50 blocks, and one block of each
    (ALL, 32, "same", (8, 8, 2), 50, False, "stack", None),
    (HALF, 72, "same", (32, 32, 8), 50, False, "wide", None),
    ((F32,), 72, "same", (32, 32, 8), 50, False, None, None),
    (HALF, 18, "same", (128, 128, 32), 50, False, "mid", None),
    ((F32,), 18, "same", (128, 128, 32), 50, False, None, None),
    (HALF, 8, "same", (32, 32, 8), 50, False, "small", None),
    ((F32,), 8, "same", (32, 32, 8), 50, False, None, None),
    (HALF, 2, "same", (128, 128, 32), 50, False, "small", None),
    ((F32,), 2, "same", (128, 128, 32), 50, False, None, None),
    (HALF, 4, "same", (512, 512, 128), 50, True, "small", None),
    ((F32,), 4, "same", (512, 512, 128), 50, True, None, None),
    (ALL, 32, "same", (8, 8, 2), 1, False, None, "tiny"),
    (HALF, 72, "same", (32, 32, 8), 1, False, "wide", "convs"),  # the wide route takes a single block
    ((F32,), 72, "same", (32, 32, 8), 1, False, None, "convs"),
    (HALF, 18, "same", (128, 128, 32), 1, False, None, "mid"),
    ((F32,), 18, "same", (128, 128, 32), 1, False, None, "convs"),
    (HALF, 8, "same", (32, 32, 8), 1, False, None, "small+fused"),
    ((F32,), 8, "same", (32, 32, 8), 1, False, None, "convs"),
    (HALF, 2, "same", (128, 128, 32), 1, False, None, "small+fused"),
    ((F32,), 2, "same", (128, 128, 32), 1, False, None, "convs"),
    (HALF, 4, "same", (512, 512, 128), 1, True, None, "small+fused"),
    ((F32,), 4, "same", (512, 512, 128), 1, True, None, "convs"),
    # stack: the smallest grid; it comes first, so it also takes a few-channel class on a tiny grid unless
    # the stack fuses few-channel runs only; misses: 256 voxels, C % 4 != 0, small_only
    (ALL, 8, "same", (2, 2, 2), 2, False, "stack", None),
    (ALL, 32, "same", (8, 8, 2), 2, False, "stack", None),
    (ALL, 32, "same", (8, 8, 4), 2, False, None, None),
    (ALL, 6, "same", (4, 4, 4), 2, False, None, None),
    (ALL, 8, "same", (4, 4, 4), 2, False, "stack", None),
    (HALF, 8, "same", (4, 4, 4), 2, True, "small", None),
    ((F32,), 8, "same", (4, 4, 4), 2, True, None, None),
    (ALL, 32, "same", (8, 8, 2), 50, True, None, None),
    # wide: the smallest grid, one block and two; misses: D = 4, D = 12, H = 7, small_only
    (HALF, 72, "same", (8, 8, 8), 1, False, "wide", "convs"),
    ((F32,), 72, "same", (8, 8, 8), 1, False, None, "convs"),
    (HALF, 72, "same", (8, 8, 8), 2, False, "wide", None),
    ((F32,), 72, "same", (8, 8, 8), 2, False, None, None),
    (ALL, 72, "same", (8, 8, 4), 1, False, None, "convs"),
    (ALL, 72, "same", (8, 8, 12), 2, False, None, None),
    (ALL, 72, "same", (7, 8, 16), 2, False, None, None),
    (ALL, 72, "same", (32, 32, 8), 50, True, None, None),
    # mid: the smallest grid (a run of one is not chained); misses: D = 8, H = 7, D = 24, 36 channels
    (HALF, 18, "same", (8, 8, 16), 2, False, "mid", None),
    ((F32,), 18, "same", (8, 8, 16), 2, False, None, None),
    (HALF, 18, "same", (8, 8, 16), 1, False, None, "mid"),
    ((F32,), 18, "same", (8, 8, 16), 1, False, None, "convs"),
    (ALL, 18, "same", (8, 8, 8), 2, False, None, None),
    (ALL, 18, "same", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 18, "same", (7, 8, 16), 2, False, None, None),
    (ALL, 18, "same", (8, 8, 24), 2, False, None, None),
    (ALL, 36, "same", (8, 8, 16), 2, False, None, None),
    # small: the smallest grid; misses: 3 x 3 x 3, D = 5
    (HALF, 2, "same", (2, 2, 2), 2, False, "small", None),
    ((F32,), 2, "same", (2, 2, 2), 2, False, None, None),
    (HALF, 2, "same", (2, 2, 2), 1, False, None, "small+fused"),
    ((F32,), 2, "same", (2, 2, 2), 1, False, None, "convs"),
    (ALL, 2, "same", (3, 3, 3), 2, False, None, None),
    (ALL, 2, "same", (3, 3, 3), 1, False, None, "convs"),
    (HALF, 8, "same", (8, 8, 8), 2, False, "small", None),
    ((F32,), 8, "same", (8, 8, 8), 2, False, None, None),
    (HALF, 8, "same", (8, 8, 8), 1, False, None, "small+fused"),  # 512 voxels: past the tiny kernels
    ((F32,), 8, "same", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 8, "same", (8, 8, 5), 2, False, None, None),
    (ALL, 8, "same", (8, 8, 5), 1, False, None, "convs"),
    # tiny: 256 voxels, up to 32 channels; misses: 512 voxels, 64 channels
    (ALL, 8, "same", (4, 4, 4), 1, False, None, "tiny"),
    (ALL, 8, "same", (8, 8, 4), 1, False, None, "tiny"),
    (ALL, 32, "same", (8, 8, 4), 1, False, None, "tiny"),
    (ALL, 32, "same", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 64, "same", (2, 2, 2), 1, False, None, "convs"),
    # the (8, 4) class around ops._SMALL_BWD_MAX_VOX = 2^19 voxels: at it (brick kernels); above it where
    # the column plan does not apply (D % 16 != 0): the fused forward, the per-conv backward, no run; above
    # it with the column plan; D = 9: no fused kernel at all
    (HALF, 8, "same", (256, 256, 8), 2, False, "small", None),
    ((F32,), 8, "same", (256, 256, 8), 2, False, None, None),
    (HALF, 8, "same", (256, 256, 8), 1, False, None, "small+fused"),
    ((F32,), 8, "same", (256, 256, 8), 1, False, None, "convs"),
    (ALL, 8, "same", (512, 512, 8), 2, False, None, None),
    (HALF, 8, "same", (512, 512, 8), 1, False, None, "small+convs"),
    ((F32,), 8, "same", (512, 512, 8), 1, False, None, "convs"),
    (HALF, 8, "same", (256, 256, 64), 2, False, "small", None),
    ((F32,), 8, "same", (256, 256, 64), 2, False, None, None),
    (HALF, 8, "same", (256, 256, 64), 1, False, None, "small+fused"),
    ((F32,), 8, "same", (256, 256, 64), 1, False, None, "convs"),
    (ALL, 8, "same", (256, 256, 9), 1, False, None, "convs"),
    # a down block, an up block, a block with a skip conv: the per-conv path, never part of a run
    (ALL, 8, "down", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 8, "down", (8, 8, 8), 2, False, None, None),
    (ALL, 8, "up", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 8, "up", (8, 8, 8), 2, False, None, None),
    (ALL, 8, "skip", (8, 8, 8), 1, False, None, "convs"),
    (ALL, 8, "skip", (8, 8, 8), 2, False, None, None),
]

# toggle -> the rows it changes (and one it must leave alone), in ROUTE_TABLE's form
TOGGLED = {
    "tiny": [(HALF, 8, "same", (4, 4, 4), 1, False, None, "small+fused"),  # default: tiny
             ((F32,), 8, "same", (4, 4, 4), 1, False, None, "convs"),
             (ALL, 32, "same", (8, 8, 2), 1, False, None, "convs"),  # default: tiny
             (ALL, 32, "same", (8, 8, 2), 2, False, "stack", None)],  # the stack run does not depend on it
    "mid": [(ALL, 18, "same", (8, 8, 16), 2, False, None, None),  # default (16-bit): mid
            (ALL, 18, "same", (8, 8, 16), 1, False, None, "convs")],  # default (16-bit): mid
    "small_bwd": [(ALL, 8, "same", (8, 8, 8), 2, False, None, None),  # default (16-bit): small
                  (HALF, 8, "same", (8, 8, 8), 1, False, None, "small+convs"),  # default: small+fused
                  ((F32,), 8, "same", (8, 8, 8), 1, False, None, "convs")],
    "wide": [(ALL, 72, "same", (8, 8, 8), 1, False, None, "convs"),  # default (16-bit): wide
             (ALL, 72, "same", (32, 32, 8), 50, False, None, None)],  # default (16-bit): wide
}

_BLOCKS = {}


def _block(c, kind):
    from vq3d import layers as VL
    blk = _BLOCKS.get((c, kind))
    if blk is None:
        out = {"same": c, "down": 2 * c, "up": c // 2, "skip": 2 * c}[kind]
        blk = _BLOCKS[(c, kind)] = VL.PreActFixupResBlock(c, out, "same" if kind == "skip" else kind)
        assert (blk.skip_conv is None) == (kind == "same")
    return blk


def routes(row, dtype):
    """(run route, block path or None) of one table row, from the code under test"""
    from vq3d import functional as Fn
    from vq3d import ops
    _, c, kind, grid, nrun, small_only, _, want_path = row
    blk, shape = _block(c, kind), (1, c) + grid
    path = None
    if nrun == 1:
        path = Fn.block_path(dtype, shape, blk)
        if path == "small":
            path += "+fused" if ops.small_bwd_fused(shape) else "+convs"
    return Fn.run_route(dtype, shape, blk, nrun, small_only), path


def _rows(table):
    for row in table:
        for dt in row[0]:
            yield pytest.param(row, dt, id=f"{str(dt)[6:]}-{row[1]}{row[2]}@{'x'.join(map(str, row[3]))}-"
                                           f"n{row[4]}{'-small_only' if row[5] else ''}")


@pytest.mark.parametrize("row,dtype", list(_rows(ROUTE_TABLE)))
def test_route_table(row, dtype):
    assert routes(row, dtype) == (row[6], row[7])


def test_table_reaches_every_route_and_path():
    assert {r[6] for r in ROUTE_TABLE} == {"stack", "wide", "mid", "small", None}
    assert {r[7] for r in ROUTE_TABLE if r[4] == 1} == {"tiny", "small+fused", "small+convs", "mid", "convs"}


def test_tensor_predicates_follow_the_route():
    """the tensor-taking wrappers: False off the GPU, whatever the shape"""
    from vq3d import functional as Fn
    x = torch.empty((1, 8, 8, 8, 8), dtype=BF16)
    blk = _block(8, "same")
    assert Fn.stack_eligible(blk) and not Fn.stack_eligible(_block(8, "down"))
    assert not (Fn.small_run_eligible(x, blk) or Fn.mid_run_eligible(x, blk) or Fn.wide_eligible(x, blk))


@pytest.mark.parametrize("toggle", sorted(TOGGLED))
def test_toggles_change_their_rows(toggle):
    from vq3d import ops
    off, on = {"tiny": (lambda: ops.set_tiny_blocks(False), lambda: ops.set_tiny_blocks(True)),
               "mid": (lambda: ops.set_mid_blocks(False), lambda: ops.set_mid_blocks(True)),
               "small_bwd": (lambda: ops.set_small_blocks(True, False), lambda: ops.set_small_blocks(True, True)),
               "wide": (lambda: ops.set_wide_blocks(False), lambda: ops.set_wide_blocks(True))}[toggle]
    rows = [(row, dt) for row in TOGGLED[toggle] for dt in row[0]]
    default = [next(r for r in ROUTE_TABLE if r[1:6] == row[1:6] and dt in r[0]) for row, dt in rows]
    off()
    try:
        got = [routes(row, dt) for row, dt in rows]
    finally:
        on()
    assert got == [(row[6], row[7]) for row, _ in rows]
    assert [routes(row, dt) for row, dt in rows] == [(d[6], d[7]) for d in default]  # restored
    assert any((row[6], row[7]) != (d[6], d[7]) for (row, _), d in zip(rows, default))
