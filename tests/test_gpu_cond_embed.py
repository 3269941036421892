"""GPU: the conditioned PixelCNN's condition embedding (csrc/cond_embed.hip, vq3d.cond_embed) and the fused
add-pre-activation glue (vq3d_preact_add_act_*, csrc/misc.hip) against float64.

Forward, against vq3d.cond_embed.cond_embed_reference on the same rounded table: with S = |be| +
sum |lam t E| over the at most 17 terms of an element, fp32 accumulation allows |err| <= 2^-19 S; a 16-bit
output adds its single final rounding u |y|, u = 2^-8 (bf16) / 2^-11 (fp16).

Backward, per element of dWe and dbe: |err| <= N 2^-23 T with N its number of terms (the (destination sample,
fine voxel, corner) triples of non-zero weight whose code is the element's; every fine voxel for dbe) and
T the sum of their magnitudes: any-order fp32 summation, with a factor 2 for the staged rounding (the
workspace, then the per-code sum).

The backward is deterministic: outputs and gradients are bit-identical run to run and across the ctypes and
torch.library bindings, and a captured graph replays with the lam / index then in its device tensors.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last_3d
GRIDS = [((2, 3, 1), (8, 6, 5)), ((1, 1, 1), (2, 3, 4)), ((3, 3, 3), (3, 3, 3)), ((3, 5, 2), (7, 9, 3)),
         ((5, 4, 3), (3, 4, 7))]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
FLOOR = {"bf16": 0.0, "fp16": 2.0 ** -25}  # half the spacing of fp16's subnormals: its rounding below 2^-14


def _case(cin, b, kc, m, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, kc, (b,) + cin, generator=g)
    flat = codes.view(-1)
    if flat.numel() >= 4:  # foreign codes: compared, never used as addresses, contribute nothing
        flat[1] = -1
        flat[flat.numel() - 1] = kc
    w = torch.randn((m, kc), generator=g)
    be = torch.randn((m,), generator=g)
    lam = torch.tensor(0.3, dtype=torch.float32)
    index = torch.tensor([1, 1, 0][:b] if b == 3 else [0] * b)  # not a permutation; batch 1: a fixed point
    return codes, w, be, lam, index


def _term_counts(codes, kc, out, index):
    """N[k]: the number of (destination sample, fine voxel, corner) terms of non-zero weight whose code is k"""
    from vq3d.cond_embed import axis_coefficients
    b, cd, ch, cw = codes.shape
    ax = [axis_coefficients(n, o) for n, o in zip((cd, ch, cw), out)]
    cnt = np.zeros((b, cd, ch, cw), dtype=np.int64)  # terms per coarse voxel of one sample's own e0
    for jz in (0, 1):
        for jy in (0, 1):
            for jx in (0, 1):
                wgt = (ax[0][2 + jz][:, None, None] * ax[1][2 + jy][None, :, None] * ax[2][2 + jx][None, None, :]) != 0
                iz, iy, ix = np.meshgrid(ax[0][jz], ax[1][jy], ax[2][jx], indexing="ij")
                np.add.at(cnt[0], (iz[wgt], iy[wgt], ix[wgt]), 1)
    cnt[:] = cnt[0]
    uses = np.ones(b, dtype=np.int64) if index is None else np.array(
        [1 + sum(int(index[d]) == s for d in range(b)) for s in range(b)])  # lam's term + every 1 - lam term
    cnt = cnt * uses[:, None, None, None]
    n = np.zeros(kc, dtype=np.int64)
    c = codes.numpy()
    ok = (c >= 0) & (c < kc)
    np.add.at(n, c[ok], cnt[ok])
    return n


def _run_case(gpu, cin, out, dname, mix, b, kc, m, seed):
    from vq3d.cond_embed import cond_embed, cond_embed_reference
    dtype = DTYPES[dname]
    codes, w, be, lam, index = _case(cin, b, kc, m, seed)
    lam_i = (lam, index) if mix else (None, None)
    wr = w.to(dtype).double()  # the table the kernel reads
    wg, bg = w.to(gpu).requires_grad_(True), be.to(gpu).requires_grad_(True)
    dev = [None if t is None else t.to(gpu) for t in lam_i]
    e = cond_embed(codes.to(gpu), wg, bg, out, dev[0], dev[1], dtype=dtype)
    assert e.dtype == dtype and tuple(e.shape) == (b, m) + out and e.is_contiguous(memory_format=CL)
    ref = cond_embed_reference(codes, wr, be, out, *lam_i)
    S = cond_embed_reference(codes, wr.abs(), be.abs(), out, *lam_i)
    bound = 2.0 ** -19 * S + U[dname] * ref.abs()
    err = (e.detach().cpu().double() - ref).abs()
    tag = f"{cin}->{out} {dname} mix {mix} b {b} kc {kc} m {m}"
    print(f"{tag}: forward error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), tag
    # a slab prefix is the crop of the full grid's e: the same bits
    d_out = max(1, out[0] - 1)
    with torch.no_grad():
        pre = cond_embed(codes.to(gpu), wg, bg, out, dev[0], dev[1], d_out=d_out, dtype=dtype)
    assert torch.equal(pre, e.detach()[:, :, :d_out]), tag
    # backward
    g = torch.randn(e.shape, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    e.backward(g.to(gpu).contiguous(memory_format=CL))
    w64, b64 = wr.clone().requires_grad_(True), be.double().requires_grad_(True)
    (cond_embed_reference(codes, w64, b64, out, *lam_i) * g.double()).sum().backward()
    wt, bt = wr.clone().requires_grad_(True), be.double().requires_grad_(True)
    (cond_embed_reference(codes, wt, bt, out, *lam_i) * g.double().abs()).sum().backward()  # T: weights are >= 0
    n_k = torch.from_numpy(_term_counts(codes, kc, out, index if mix else None)).double()
    bw = n_k.view(1, kc) * 2.0 ** -23 * wt.grad
    bb = float(b * out[0] * out[1] * out[2]) * 2.0 ** -23 * bt.grad
    ew = (wg.grad.cpu().double() - w64.grad).abs()
    eb = (bg.grad.cpu().double() - b64.grad).abs()
    print(f"{tag}: dWe error / bound {float((ew / bw.clamp_min(1e-300)).max()):.3f}, "
          f"dbe {float((eb / bb.clamp_min(1e-300)).max()):.3f}")
    assert wg.grad.dtype == torch.float32 and tuple(wg.grad.shape) == (m, kc)
    assert bool((ew <= bw).all()), tag
    assert bool((eb <= bb).all()), tag
    assert bool((wg.grad[:, n_k == 0] == 0).all())  # codes nobody names get nothing


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("dname", sorted(DTYPES))
@pytest.mark.parametrize("cin,out", GRIDS)
def test_forward_and_backward_against_float64(gpu, cin, out, dname, mix):
    seed = 0
    for m in (8, 72):
        for kc in (8, 512):
            for b in (1, 3):
                seed += 1
                _run_case(gpu, cin, out, dname, mix, b, kc, m, seed)


def test_two_workgroup_grid_and_wide_embedding(gpu):
    """more than one workgroup in every launch, M = 1024 (four channel steps per thread of the per-code sums)"""
    _run_case(gpu, (3, 2, 2), (6, 5, 7), "bf16", True, 3, 16, 1024, 7)


@pytest.mark.parametrize("dname", sorted(DTYPES))
def test_bitwise_determinism_and_bindings(gpu, dname):
    from vq3d import functional as Fn
    from vq3d.cond_embed import cond_embed
    codes, w, be, lam, index = _case((3, 5, 2), 3, 512, 72, 11)
    out = (7, 9, 3)
    g = torch.randn((3, 72) + out, generator=torch.Generator().manual_seed(2)).to(DTYPES[dname]).to(gpu).contiguous(
        memory_format=CL)

    def run():
        wg, bg = w.to(gpu).requires_grad_(True), be.to(gpu).requires_grad_(True)
        e = cond_embed(codes.to(gpu), wg, bg, out, lam.to(gpu), index.to(gpu), dtype=DTYPES[dname])
        e.backward(g)
        return e.detach(), wg.grad, bg.grad
    first, second = run(), run()
    assert Fn.binding() == "ctypes"
    Fn.set_binding("library")
    try:
        third = run()
    finally:
        Fn.set_binding("ctypes")
    for a, b2, c3 in zip(first, second, third):
        assert torch.equal(a, b2) and torch.equal(a, c3)


def test_parameter_gradients_go_into_their_buffers(gpu):
    """leaf nn.Parameters: the kernel adds into .grad directly (twice: the sum), autograd gets nothing"""
    from vq3d.cond_embed import cond_embed
    codes, w, be, _, _ = _case((2, 3, 1), 2, 8, 16, 3)
    conv = torch.nn.Conv3d(8, 16, 1).to(gpu)
    with torch.no_grad():
        conv.weight.copy_(w.view(16, 8, 1, 1, 1))
        conv.bias.copy_(be)
    g = torch.randn((2, 16, 8, 6, 5), generator=torch.Generator().manual_seed(4)).to(gpu).contiguous(memory_format=CL)
    for _ in range(2):
        cond_embed(codes.to(gpu), conv.weight, conv.bias, (8, 6, 5)).backward(g)
    wg = w.to(gpu).requires_grad_(True)
    bg = be.to(gpu).requires_grad_(True)
    cond_embed(codes.to(gpu), wg, bg, (8, 6, 5)).backward(g)
    assert tuple(conv.weight.grad.shape) == (16, 8, 1, 1, 1)
    assert torch.equal(conv.weight.grad.view(16, 8), wg.grad + wg.grad) and torch.equal(conv.bias.grad, bg.grad + bg.grad)


def test_registered_operator_differentiates(gpu):
    """torch.ops.vq3d.cond_embed called directly under autograd gives CondEmbedFn's gradients (of the table)"""
    import vq3d.library  # noqa: F401
    from vq3d.cond_embed import cond_embed
    codes, w, be, lam, index = _case((2, 3, 1), 3, 8, 16, 5)
    out = (8, 6, 5)
    g = torch.randn((3, 16) + out, generator=torch.Generator().manual_seed(6)).to(gpu).contiguous(memory_format=CL)
    table = w.t().contiguous().to(gpu).requires_grad_(True)
    b1 = be.to(gpu).requires_grad_(True)
    e1 = torch.ops.vq3d.cond_embed(codes.to(gpu), table, b1, list(out), out[0], lam.to(gpu), index.to(gpu))
    e1.backward(g)
    wg, bg = w.to(gpu).requires_grad_(True), be.to(gpu).requires_grad_(True)
    e2 = cond_embed(codes.to(gpu), wg, bg, out, lam.to(gpu), index.to(gpu))
    e2.backward(g)
    assert torch.equal(e1.detach(), e2.detach())
    assert torch.equal(table.grad, wg.grad.t()) and torch.equal(b1.grad, bg.grad)


def test_captured_graph_replays_with_new_draws(gpu):
    from vq3d import ops
    from vq3d.cond_embed import cond_embed_bwd_kernel, cond_embed_fwd_kernel
    codes, w, be, _, _ = _case((3, 5, 2), 3, 8, 72, 13)
    out, kc, m = (7, 9, 3), 8, 72
    codes_g = codes.to(gpu)
    table = w.t().contiguous().to(torch.bfloat16).to(gpu)
    bias = be.to(gpu)
    g = torch.randn((3, m) + out, generator=torch.Generator().manual_seed(14)).to(torch.bfloat16).to(gpu).contiguous(
        memory_format=CL)
    lam_t = torch.tensor(0.3, dtype=torch.float32, device=gpu)
    index_t = torch.tensor([1, 2, 0], dtype=torch.int64, device=gpu)

    def step():
        e = cond_embed_fwd_kernel(codes_g, table, bias, out, out[0], lam_t, index_t)
        dwe = ops.zero_(torch.empty((m, kc), dtype=torch.float32, device=gpu))
        dbe = ops.zero_(torch.empty((m,), dtype=torch.float32, device=gpu))
        cond_embed_bwd_kernel(g, codes_g, kc, lam_t, index_t, dwe, dbe)
        return e, dwe, dbe
    step()  # lazy initialisations stay out of the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        static = step()
    for lam, index in ((0.3, [1, 2, 0]), (0.85, [2, 2, 1]), (0.0, [0, 1, 2])):
        lam_t.copy_(torch.tensor(lam, dtype=torch.float32))
        index_t.copy_(torch.tensor(index, dtype=torch.int64))
        graph.replay()
        replayed = [t.clone() for t in static]
        eager = step()
        for a, b2 in zip(replayed, eager):
            assert torch.equal(a, b2), (lam, index)


# ------------------------------------------------------------------ the fused add-pre-activation
@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [8, 1000, 65544])
def test_preact_add_act_against_float64(gpu, n, dname):
    """y = elu(x + p + a) + b and gx = g elu'(x + p + a), da = sum gx, db = sum g (n = 65,544: more workgroups
    than one, a ragged tail).  Arithmetic fp32 from 16-bit operands: y and gx within one rounding of the
    format (u |value|, fp16: at least half a subnormal step) plus fp32 noise; the sums within n 2^-23 sum |terms| (any-order fp32 summation, staged)."""
    from vq3d import _lib as L
    dtype, u, fl = DTYPES[dname], U[dname], FLOOR[dname]
    gen = torch.Generator().manual_seed(n)
    x, p, g = (torch.randn(n, generator=gen).to(dtype) for _ in range(3))
    a, b = torch.tensor([0.3]), torch.tensor([-0.2])
    xg, pg, gg, ag, bg = (t.to(gpu) for t in (x, p, g, a, b))
    y = torch.empty_like(xg)
    L.call("vq3d_preact_add_act_fwd", L.dtype_code(xg), n, L.ptr(xg), L.ptr(pg), L.ptr(ag), L.ptr(bg), L.ptr(y), L.stream())
    z = x.double() + p.double() + float(a)
    yr = torch.where(z > 0, z, torch.expm1(z)) + float(b)
    assert bool(((y.cpu().double() - yr).abs() <= u * yr.abs() + fl + 1e-6 * (1 + z.abs())).all())
    gx = torch.empty_like(xg)
    da, db = torch.zeros(1, device=gpu), torch.zeros(1, device=gpu)
    L.call("vq3d_preact_add_act_bwd", L.dtype_code(xg), n, L.ptr(gg), L.ptr(xg), L.ptr(pg), L.ptr(ag), L.ptr(gx), L.ptr(da),
           L.ptr(db), L.stream())
    gr = g.double() * torch.where(z > 0, torch.ones_like(z), torch.exp(z))
    assert bool(((gx.cpu().double() - gr).abs() <= u * gr.abs() + fl + 1e-6 * g.double().abs()).all())
    # the sums are of the unrounded fp32 products
    tol_a = n * 2.0 ** -23 * float(gr.abs().sum()) + 1e-6 * float(g.double().abs().sum())
    assert abs(float(da) - float(gr.sum())) <= tol_a
    assert abs(float(db) - float(g.double().sum())) <= n * 2.0 ** -23 * float(g.double().abs().sum())
    # twice the same bits; the sums are added into their buffers
    da2, db2 = da.clone(), db.clone()
    gx2 = torch.empty_like(xg)
    L.call("vq3d_preact_add_act_bwd", L.dtype_code(xg), n, L.ptr(gg), L.ptr(xg), L.ptr(pg), L.ptr(ag), L.ptr(gx2), L.ptr(da2),
           L.ptr(db2), L.stream())
    assert torch.equal(gx, gx2) and torch.equal(da2, da + da) and torch.equal(db2, db + db)


def test_preact_add_fn_matches_the_unfused_glue(gpu):
    """PreActAddFn against add + PreActFn (the same fp32 arithmetic on x + p rounded once more): outputs within
    a bf16 rounding, both inputs get the one gradient tensor's values"""
    from vq3d import pixelsnail as PS
    prev = PS._compute[0]
    PS._compute[0] = torch.bfloat16
    try:
        gen = torch.Generator().manual_seed(0)
        shape = (2, 8, 3, 4, 5)
        x, p = (torch.randn(shape, generator=gen).to(torch.bfloat16).to(gpu).contiguous(memory_format=CL).requires_grad_(True)
                for _ in range(2))
        a = torch.tensor([0.1], device=gpu, requires_grad=True)
        b = torch.tensor([-0.3], device=gpu, requires_grad=True)
        y = PS.PreActAddFn.apply(x, p, a, b)
        g = torch.randn(shape, generator=gen).to(torch.bfloat16).to(gpu).contiguous(memory_format=CL)
        y.backward(g)
        z = x.detach().double() + p.detach().double() + 0.1
        yr = torch.where(z > 0, z, torch.expm1(z)) - 0.3
        assert float((y.detach().double() - yr).abs().max()) <= 2.0 ** -8 * float(yr.abs().max())
        assert torch.equal(x.grad, p.grad)
        gr = g.double() * torch.where(z > 0, torch.ones_like(z), torch.exp(z))
        assert float((x.grad.double() - gr).abs().max()) <= 2.0 ** -8 * float(gr.abs().max())
        assert abs(float(a.grad) - float(gr.sum())) <= 1e-3 * float(gr.abs().sum())
        assert abs(float(b.grad) - float(g.double().sum())) <= 1e-5 * float(g.double().abs().sum())
    finally:
        PS._compute[0] = prev
