"""Every dispatch path of the quantizer kernels (csrc/vq.hip) through the C-ABI, against plain
references: the C oracle (oracle/vq_nearest.c) for the search, numpy float64 for the statistics,
the EMA update, the moments, the codebook init and the backward.

The host picks a kernel by the row count n, the embedding dim d, the codebook size k and the
storage types; tests/test_vq_paths_cpu.py mirrors those thresholds and asserts that the case
tables below reach every path (if a threshold moves, that test names the case to re-aim).

Harness of every op: each output is a view into a larger buffer pre-filled with a NaN / negative
sentinel (the guard elements on both sides must be untouched, every element inside written), and
the workspace is exactly vq3d_vq_workspace_size bytes, pre-filled with 0xFF (all NaN: nothing may
rely on a zeroed workspace), followed by a guard that must stay intact.  Everything lies inside
one torch allocation each, so a wrong plan shows as a failed assertion, not as a fault.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
HALVES = ("bf16", "f16")  # the two builds behind abi_dispatch.cpp

# ------------------------------------------------------------------------------------------ case tables
# (n, d, k) of vq3d_vq_nearest, by the path they are aimed at
NEAREST_SINGLE_SMALL = [(1000, d, 15) for d in (1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 31, 32, 33, 63, 64)] + \
    [(1, 3, 1), (255, 6, 15), (257, 6, 15)]
NEAREST_SINGLE_LARGE = [(32805, 2, 300), (32805, 64, 256), (32805, 64, 257)]
NEAREST_WIDE = [(1000, 65, 40), (1000, 67, 40), (1000, 96, 40), (300, 128, 200)]
NEAREST_SPLIT = [(1, 3, 17), (300, 7, 100), (4096, 13, 64), (257, 64, 16), (2000, 33, 130), (2000, 20, 75)]
NEAREST_BOUNDARY = (32512, 32513, 8, 64)  # n split, n single pass, d, k
NEAREST_CAPPED = [(26368, 64, 2561), (16384, 32, 4096)]  # oracle on a row subset
NEAREST_TIES = {"single": (1000, 4, 15), "global": (32805, 64, 257), "split": (2048, 4, 64)}
# near-duplicate codeword pairs: which of a pair wins hangs on the rounding of every accumulation
# (single pass in LDS, from memory, wide, split; d % 4 == 3 each)
NEAREST_NEAR = [(1000, 7, 14), (32805, 63, 262), (1000, 67, 40), (1000, 7, 40)]
NEAREST_STORAGE = [(1000, 7, 15), (32805, 64, 257), (1000, 67, 40), (300, 7, 100), (2000, 20, 75)]

STATS_CASES = [(5, 3, 4), (1003, 2, 16), (4099, 8, 33), (8200, 1, 3), (16500, 5, 20), (33000, 2, 128),
               (66000, 1, 7), (140000, 1, 3), (140000, 4, 40), (2000, 32, 512)]
STATS_16BIT = [(4099, 8, 33), (140000, 4, 40)]
STATS_ONE_CODE = (1003, 2, 16)

UPDATE_K = (1, 17, 1024, 1025, 2500)
UPDATE_D = (1, 3, 32)
DECAY, ALPHA = 0.99, 1e-5  # the Quantizer's defaults

MOMENTS_CASES = [(2, 1), (1000, 3), (4097, 65), (300000, 2)]
MOMENTS_OFFSET = (1000, 8)  # mean 1000, std 0.01
MOMENTS_16BIT = (4097, 65)
INIT_CASES = [(1, 1), (17, 3), (300, 32)]
BWD_CASES = [(1003, 7), (1, 1)]


# ------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def nearest_inputs(n, d, k, tie=None):
    """z ~ 1.3 N(0, 1) (n, d), e ~ N(0, 1) (k, d), fp32; `tie` plants exact duplicates, or with
    "near" makes every odd codeword its even neighbour moved by up to 2 ulp per coordinate (and
    for d > 16 scales the first 4 * floor(d / 4) coordinates of z and e by 1 / 4)."""
    rng = np.random.default_rng([n, d, k, {None: 0, "single": 1, "global": 2, "split": 3, "near": 4}[tie]])
    z = (1.3 * rng.standard_normal((n, d))).astype(np.float32)
    e = rng.standard_normal((k, d)).astype(np.float32)
    if tie == "single":  # codewords on a 0.5 grid, z on a 0.25 grid: squared distances are exact
        e = (np.round(e * 2) / 2).astype(np.float32)
        z = (np.round(z * 4) / 4).astype(np.float32)
        e[7] = e[2]
        e[14] = e[2]
        z[:15] = e
    elif tie == "global":
        e[256] = e[0]
        e[128] = e[5]
        z[0:64:2] = e[0]
        z[1:64:2] = e[5]
    elif tie == "split":  # 8 chunks of 8 codes: (7, 8) straddles a chunk boundary, (0, 63) the ends
        e[8] = e[7]
        e[63] = e[0]
        z[0:32:2] = e[7]
        z[1:32:2] = e[0]
    elif tie == "near":
        if d > 16:  # the 3 tail terms weigh as much as the many head terms: both roundings show
            z[:, :d & ~3] *= 0.25
            e[:, :d & ~3] *= 0.25
        base = np.ascontiguousarray(e[0:2 * (k // 2):2])
        e[1:2 * (k // 2):2] = (base.view(np.int32) + rng.integers(-2, 3, size=base.shape, dtype=np.int32)).view(np.float32)
    z.setflags(write=False)
    e.setflags(write=False)
    return z, e


def subset_rows(n):
    """first 256 rows, the last 300, every 17th in between"""
    return np.concatenate([np.arange(256), np.arange(256, n - 300, 17), np.arange(n - 300, n)])


def z_as(z, kind):
    """the fp32 numpy rows as a torch tensor of storage type `kind`"""
    return torch.tensor(z).to(DT[kind])  # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def stats_inputs(n, d, k, one_code=False):
    rng = np.random.default_rng([n, d, k, 7])
    z = (1.3 * rng.standard_normal((n, d))).astype(np.float32)
    used = np.array([c for c in range(k) if c % 3 != 1])  # every third code is never drawn
    idx = rng.choice(used, size=n).astype(np.int64)
    if one_code:
        idx[:] = used[-1]
    return z, idx


def update_inputs(k, d):
    rng = np.random.default_rng([k, d, 11])
    cs = rng.uniform(0.5, 50.0, k).astype(np.float32)
    counts = rng.integers(1, 200, k).astype(np.float32)
    if k > 1:
        cs[2::3] = 0.0  # a third of the codes have no history
        counts[4::5] = 0.0  # a fifth got no row this step
    embed_avg = rng.standard_normal((k, d)).astype(np.float32) * cs[:, None]
    dw = rng.standard_normal((k, d)).astype(np.float32) * counts[:, None]
    embed = rng.standard_normal((k, d)).astype(np.float32)
    return embed, embed_avg, cs, counts, dw


def update_reference(embed_avg, cs, counts, dw):
    """layers.py:649-663 in float64 from the fp32 inputs and the fp32-rounded scalars; returns
    cluster_size, embed_avg, embed and the bounds' ingredients |a| + |b| and smoothed."""
    dec, omd, al = float(np.float32(DECAY)), float(np.float32(1 - DECAY)), float(np.float32(ALPHA))
    k = cs.shape[0]
    cs_r = cs.astype(np.float64) * dec + counts.astype(np.float64) * omd
    a, b = embed_avg.astype(np.float64) * dec, dw.astype(np.float64) * omd
    ntot = cs_r.sum()
    smoothed = ntot * ((cs_r + al) / (ntot + k * al))
    return cs_r, a + b, (a + b) / smoothed[:, None], np.abs(a) + np.abs(b), smoothed


def embed_bound(k, mag, smoothed):
    return (math.ceil(k / 1024) + 32) * U * mag / smoothed[:, None]


def moments_inputs(n, d, offset=False):
    rng = np.random.default_rng([n, d, 13])
    z = rng.standard_normal((n, d))
    z = (1000.0 + 0.01 * z) if offset else (0.3 + 1.3 * z)
    return z.astype(np.float32)


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def ulp_of(x, kind):
    """unit in the last place of storage type `kind` at the magnitude of x (float64 array)"""
    if kind == "f32":
        return ulp32(x)
    bits, emin = (7, -126) if kind == "bf16" else (10, -14)
    ex = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** emin)))
    return 2.0 ** (ex - bits)


# ------------------------------------------------------------------------------------------ harness
GUARD = 64  # elements on either side of an output
_BITS = {torch.float32: torch.int32, torch.int64: torch.int64, torch.bfloat16: torch.int16,
         torch.float16: torch.int16}
_SENTINEL = {torch.int32: 0x7FC5A5A5, torch.int16: 0x7FA5, torch.int64: -0x5A5A5A5A5A5A5A5B}  # NaN / negative


class Guarded:
    """An output of `shape` inside a sentinel-filled buffer; `init` (a CPU tensor) makes it an
    in/out operand, which is only guard-checked."""

    def __init__(self, shape, dtype, dev, init=None):
        self.numel = int(np.prod(shape, dtype=np.int64))
        self.buf = torch.empty(self.numel + 2 * GUARD, dtype=dtype, device=dev)
        self.bits = self.buf.view(_BITS[dtype])
        self.sent = _SENTINEL[self.bits.dtype]
        self.bits.fill_(self.sent)
        self.t = self.buf[GUARD:GUARD + self.numel].view(shape)
        self.inout = init is not None
        if self.inout:
            self.t.copy_(init.to(dtype).reshape(shape))

    def check(self, name):
        bits = self.bits.cpu()
        assert bool((bits[:GUARD] == self.sent).all()), f"{name}: written before its first element"
        assert bool((bits[GUARD + self.numel:] == self.sent).all()), f"{name}: written past its last element"
        if not self.inout:
            missed = int((bits[GUARD:GUARD + self.numel] == self.sent).sum())
            assert missed == 0, f"{name}: {missed} of {self.numel} elements never written"
        return self.t.cpu()


class Workspace:
    def __init__(self, n, d, k, dev):
        from vq3d import _lib as L
        self.nbytes = int(L.query("vq3d_vq_workspace_size", n, d, k))
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)

    def check(self):
        assert bool((self.buf[self.nbytes:] == 0xFF).all()), "written past vq3d_vq_workspace_size bytes"


def finish(ws, **outs):
    torch.cuda.synchronize()
    got = {name: g.check(name) for name, g in outs.items()}
    if ws is not None:
        ws.check()
    return got


# ------------------------------------------------------------------------------------------ a) nearest
def run_nearest(gpu, zt, e, qkind):
    """vq3d_vq_nearest + vq3d_vq_commit_loss on the rows zt (a CPU tensor in its storage type)."""
    from vq3d import _lib as L
    n, d = zt.shape
    k = e.shape[0]
    zg = zt.to(gpu)
    eg = torch.tensor(e).to(gpu)
    idx = Guarded((n,), torch.int64, gpu)
    zst = Guarded((n, d), DT[qkind], gpu)
    sq = Guarded((), torch.float32, gpu)
    loss = Guarded((), torch.float32, gpu)
    ws = Workspace(n, d, k, gpu)
    coef = 0.1 / float(n * d)
    L.call("vq3d_vq_nearest", L.dtype_code(zg), L.ptr(zg), n, d, L.ptr(eg), k, L.ptr(idx.t), L.dtype_code(zst.t),
           L.ptr(zst.t), L.ptr(sq.t), L.ptr(ws.buf), L.stream())
    L.call("vq3d_vq_commit_loss", L.ptr(sq.t), coef, L.ptr(loss.t), L.stream())
    got = finish(ws, idx=idx, zst=zst, sq=sq, loss=loss)
    assert torch.equal(zg.cpu(), zt) and np.array_equal(eg.cpu().numpy(), e), "an input was modified"
    want_loss = np.float32(coef) * got["sq"].numpy()
    assert got["loss"].numpy().view(np.uint32) == want_loss.view(np.uint32), (got["loss"], want_loss)
    return got["idx"].numpy(), got["zst"], float(got["sq"])


_ORACLE = {}


def oracle_nearest(key, x, e, rows):
    """oracle.vq_oracle.nearest on the rows `rows` of x, once per key"""
    if key not in _ORACLE:
        from oracle import vq_oracle
        xr = x if rows is None else x[rows]
        oi, oz, _ = vq_oracle.nearest(xr, e)
        _ORACLE[key] = (oi, oz)
    return _ORACLE[key]


def same_bits(t, want32, qkind):
    """t (CPU tensor of storage type qkind) equals the fp32 array want32 rounded to that type, bitwise"""
    if qkind == "f32":
        return np.array_equal(t.numpy().view(np.uint32), np.ascontiguousarray(want32).view(np.uint32))
    want = torch.from_numpy(np.ascontiguousarray(want32)).to(DT[qkind])
    return torch.equal(t.view(torch.int16), want.view(torch.int16))


def check_nearest(gpu, n, d, k, zkind="f32", qkind="f32", tie=None, subset=False, rows_of=None):
    """Run the first n rows of the case's data (rows_of: the n the data was drawn with) and hold
    idx, zst, sq and the commitment loss against the oracle; returns (idx, zst)."""
    z, e = nearest_inputs(rows_of or n, d, k, tie)
    zt = z_as(z[:n], zkind)
    x = zt.float().numpy()
    idx, zst, sq = run_nearest(gpu, zt, e, qkind)
    rows = subset_rows(n) if subset else None
    oi, oz = oracle_nearest((rows_of or n, n, d, k, tie, zkind), x, e, rows)
    sel = slice(None) if rows is None else rows
    bad = np.flatnonzero(idx[sel] != oi)
    assert bad.size == 0, f"{bad.size} codes differ from the oracle, first at row {bad[:5]}"
    assert same_bits(zst[sel] if rows is None else zst[torch.from_numpy(rows)], oz, qkind)
    # every row (the oracle may have seen a subset): zst = fl(x + fl(q - x)) of the code found
    diff = e[idx] - x
    assert same_bits(zst, x + diff, qkind)
    ref = float((diff.astype(np.float64) ** 2).sum())
    nb_near = -(-n // 256)
    bound = (d + math.ceil(nb_near / 256) + 24) * 2.0 ** -23
    err = abs(sq - ref) / ref if ref > 0 else abs(sq)
    print(f"nearest {(n, d, k)} {zkind}->{qkind}: sq rel err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (sq, ref, err, bound)
    return idx, zst


@pytest.mark.parametrize("n,d,k", NEAREST_SINGLE_SMALL + NEAREST_SINGLE_LARGE, ids=str)
def test_nearest_single_pass(gpu, n, d, k):
    check_nearest(gpu, n, d, k)


@pytest.mark.parametrize("n,d,k", NEAREST_WIDE, ids=str)
def test_nearest_wide(gpu, n, d, k):
    check_nearest(gpu, n, d, k)


@pytest.mark.parametrize("n,d,k", NEAREST_SPLIT, ids=str)
def test_nearest_split(gpu, n, d, k):
    check_nearest(gpu, n, d, k)


def test_nearest_path_boundary(gpu):
    """127 row blocks take the split search, 128 the single pass: the same rows, the same answer"""
    n_split, n_single, d, k = NEAREST_BOUNDARY
    i0, z0 = check_nearest(gpu, n_split, d, k, rows_of=n_single)
    i1, z1 = check_nearest(gpu, n_single, d, k)
    assert np.array_equal(i0, i1[:n_split])
    assert same_bits(z0, z1[:n_split].numpy(), "f32")


@pytest.mark.parametrize("n,d,k", NEAREST_CAPPED, ids=str)
def test_nearest_split_capped_lds(gpu, n, d, k):
    """codebooks whose uncapped chunk would not fit the LDS: more, smaller chunks"""
    check_nearest(gpu, n, d, k, subset=True)


@pytest.mark.parametrize("tie", sorted(NEAREST_TIES))
def test_nearest_ties_first_index(gpu, tie):
    n, d, k = NEAREST_TIES[tie]
    idx, _ = check_nearest(gpu, n, d, k, tie=tie)
    _, e = nearest_inputs(n, d, k, tie)
    dup = [c for c in range(k) if any(np.array_equal(e[c], e[b]) for b in range(c))]
    assert dup and not np.isin(idx, dup).any(), "a later duplicate of a codeword won a tie"


@pytest.mark.parametrize("n,d,k", NEAREST_NEAR, ids=str)
def test_nearest_rounding_of_every_term(gpu, n, d, k):
    """codeword pairs a few ulp apart: an FMA in the first 4 * floor(d / 4) terms, or none in the
    tail, picks the other one of a pair on many rows (tests/test_vq_paths_cpu.py counts them)"""
    check_nearest(gpu, n, d, k, tie="near")


@pytest.mark.parametrize("tq", (False, True), ids=("q32", "q16"))
@pytest.mark.parametrize("tz", (False, True), ids=("z32", "z16"))
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,d,k", NEAREST_STORAGE, ids=str)
def test_nearest_storage_types(gpu, n, d, k, half, tz, tq):
    if not (tz or tq):
        half = "f32"  # fp32 in and out: one build, the same call for both values of `half`
    check_nearest(gpu, n, d, k, zkind=half if tz else "f32", qkind=half if tq else "f32")


# ------------------------------------------------------------------------------------------ b) EMA statistics
def run_stats(gpu, zg, ig, k, ws):
    from vq3d import _lib as L
    n, d = zg.shape
    counts = Guarded((k,), torch.float32, gpu)
    dw = Guarded((k, d), torch.float32, gpu)
    L.call("vq3d_vq_ema_stats", L.dtype_code(zg), L.ptr(zg), n, d, L.ptr(ig), k, L.ptr(counts.t), L.ptr(dw.t),
           L.ptr(ws.buf), L.stream())
    got = finish(ws, counts=counts, dw=dw)
    return got["counts"].numpy(), got["dw"].numpy()


def check_stats(gpu, n, d, k, zkind="f32", one_code=False):
    z, idx = stats_inputs(n, d, k, one_code)
    zt = z_as(z, zkind)
    x = zt.float().numpy().astype(np.float64)
    zg, ig = zt.to(gpu), torch.from_numpy(idx).to(gpu)
    ws = Workspace(n, d, k, gpu)
    counts, dw = run_stats(gpu, zg, ig, k, ws)
    ref_c = np.bincount(idx, minlength=k)
    assert (ref_c == 0).any() or k == 1
    assert np.array_equal(counts, ref_c.astype(np.float32)), np.flatnonzero(counts != ref_c)[:8]
    ref = np.stack([np.bincount(idx, weights=x[:, j], minlength=k) for j in range(d)], axis=1)
    mag = np.stack([np.bincount(idx, weights=np.abs(x[:, j]), minlength=k) for j in range(d)], axis=1)
    bound = (ref_c[:, None] + 1) * U * mag
    err = np.abs(dw.astype(np.float64) - ref)
    print(f"ema_stats {(n, d, k)} {zkind}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]
    counts2, dw2 = run_stats(gpu, zg, ig, k, ws)  # the workspace now holds the first call's partials
    assert np.array_equal(counts2.view(np.uint32), counts.view(np.uint32))
    assert np.array_equal(dw2.view(np.uint32), dw.view(np.uint32))


@pytest.mark.parametrize("n,d,k", STATS_CASES, ids=str)
def test_ema_stats(gpu, n, d, k):
    check_stats(gpu, n, d, k)


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,d,k", STATS_16BIT, ids=str)
def test_ema_stats_16bit(gpu, n, d, k, half):
    check_stats(gpu, n, d, k, zkind=half)


def test_ema_stats_one_code(gpu):
    check_stats(gpu, *STATS_ONE_CODE, one_code=True)


# ------------------------------------------------------------------------------------------ c) EMA update
@pytest.mark.parametrize("d", UPDATE_D)
@pytest.mark.parametrize("k", UPDATE_K)
def test_ema_update(gpu, k, d):
    """layers.py:649-663 with the Quantizer's decay 0.99.  The cluster_size bound of 4 u is what
    made vq3d_vq_ema_update take decay as a double: with an fp32 decay the host could only form
    fl32(1 - fl32(0.99)), 9.3e-7 relative (100 ulp) away from torch's fl32(1 - 0.99), and every code
    without history (cluster_size = counts * (1 - decay)) missed the bound by that much."""
    from vq3d import _lib as L
    embed, embed_avg, cs, counts, dw = update_inputs(k, d)
    assert counts.sum() > 0
    g_e = Guarded((k, d), torch.float32, gpu)  # every element of embed is an output
    g_a = Guarded((k, d), torch.float32, gpu, init=torch.from_numpy(embed_avg))
    g_c = Guarded((k,), torch.float32, gpu, init=torch.from_numpy(cs))
    cg, dg = torch.from_numpy(counts).to(gpu), torch.from_numpy(dw).to(gpu)
    L.call("vq3d_vq_ema_update", L.ptr(g_e.t), L.ptr(g_a.t), L.ptr(g_c.t), L.ptr(cg), L.ptr(dg), k, d, DECAY, ALPHA,
           L.stream())
    got = finish(None, embed=g_e, embed_avg=g_a, cluster_size=g_c)
    cs_r, ea_r, e_r, mag, smoothed = update_reference(embed_avg, cs, counts, dw)
    cs_g = got["cluster_size"].numpy().astype(np.float64)
    assert (np.abs(cs_g - cs_r) <= 4 * U * np.abs(cs_r)).all(), float((np.abs(cs_g - cs_r) / np.maximum(cs_r, 1e-30)).max())
    ea_g = got["embed_avg"].numpy().astype(np.float64)
    assert (np.abs(ea_g - ea_r) <= 3 * U * mag).all()
    e_g = got["embed"].numpy().astype(np.float64)
    bound = embed_bound(k, mag, smoothed)
    err = np.abs(e_g - e_r)
    print(f"ema_update k {k} d {d}: max embed err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]


# ------------------------------------------------------------------------------------------ d) moments, init
def check_moments(gpu, n, d, zkind="f32", offset=False):
    from vq3d import _lib as L
    zt = z_as(moments_inputs(n, d, offset), zkind)
    x = zt.float().numpy().astype(np.float64)
    zg = zt.to(gpu)
    mean = Guarded((d,), torch.float32, gpu)
    std = Guarded((d,), torch.float32, gpu)
    ws = Workspace(n, d, 1, gpu)  # vq3d_vq_moments plans with k = 1
    L.call("vq3d_vq_moments", L.dtype_code(zg), L.ptr(zg), n, d, L.ptr(mean.t), L.ptr(std.t), L.ptr(ws.buf),
           L.stream())
    got = finish(ws, mean=mean, std=std)
    for name, ref in (("mean", x.mean(axis=0)), ("std", x.std(axis=0, ddof=1))):
        err = np.abs(got[name].numpy().astype(np.float64) - ref) / ulp32(ref)
        print(f"moments {(n, d)} {zkind} {name}: max err {float(err.max()):.3f} ulp")
        assert (err <= 2.0).all(), (name, float(err.max()))


@pytest.mark.parametrize("n,d", MOMENTS_CASES, ids=str)
def test_moments(gpu, n, d):
    check_moments(gpu, n, d)


def test_moments_large_mean(gpu):
    """mean 1000, std 0.01: the second pass must centre on more than the fp32-rounded mean (centred
    on that, std was off by (mean error / std)^2 / 2 relative, tens of ulp here; the kernel now keeps
    the fp64 mean in the workspace for its second pass)"""
    check_moments(gpu, *MOMENTS_OFFSET, offset=True)


@pytest.mark.parametrize("half", HALVES)
def test_moments_16bit(gpu, half):
    check_moments(gpu, *MOMENTS_16BIT, zkind=half)


@pytest.mark.parametrize("inv_world", (1.0, 0.5))
@pytest.mark.parametrize("k,d", INIT_CASES, ids=str)
def test_init_apply(gpu, k, d, inv_world):
    from vq3d import _lib as L
    rng = np.random.default_rng([k, d, 17])
    embed = rng.standard_normal((k, d)).astype(np.float32)
    mean = (0.4 + rng.standard_normal(d)).astype(np.float32)
    std = rng.uniform(0.5, 2.0, d).astype(np.float32)
    cs = rng.uniform(0.0, 3.0, k).astype(np.float32)
    n_total = 27648.0
    g_e = Guarded((k, d), torch.float32, gpu, init=torch.from_numpy(embed))
    g_a = Guarded((k, d), torch.float32, gpu)
    g_c = Guarded((k,), torch.float32, gpu, init=torch.from_numpy(cs))
    g_f = Guarded((), torch.int64, gpu, init=torch.tensor(1))
    mg, sg = torch.from_numpy(mean).to(gpu), torch.from_numpy(std).to(gpu)
    L.call("vq3d_vq_init_apply", L.ptr(g_e.t), L.ptr(g_a.t), L.ptr(g_c.t), L.ptr(g_f.t), L.ptr(mg), L.ptr(sg), k, d,
           inv_world, n_total, L.stream())
    got = finish(None, embed=g_e, embed_avg=g_a, cluster_size=g_c, first_pass=g_f)
    e_g = got["embed"].numpy()
    assert np.array_equal(e_g.view(np.uint32), got["embed_avg"].numpy().view(np.uint32))
    a = embed.astype(np.float64) * (std.astype(np.float64) * inv_world)
    b = np.broadcast_to(mean.astype(np.float64) * inv_world, a.shape)
    assert (np.abs(e_g.astype(np.float64) - (a + b)) <= 2 * U * (np.abs(a) + np.abs(b))).all()
    want_cs = cs + np.float32(n_total / k)
    assert np.array_equal(got["cluster_size"].numpy().view(np.uint32), want_cs.view(np.uint32))
    assert int(got["first_pass"]) == 0


# ------------------------------------------------------------------------------------------ e) backward
@pytest.mark.parametrize("with_loss", (True, False), ids=("gloss", "nogloss"))
@pytest.mark.parametrize("tg", (False, True), ids=("g32", "g16"))
@pytest.mark.parametrize("tz", (False, True), ids=("z32", "z16"))
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("n,d", BWD_CASES, ids=str)
def test_vq_bwd(gpu, n, d, half, tz, tg, with_loss):
    from vq3d import _lib as L
    k = 20
    rng = np.random.default_rng([n, d, 19])
    zkind, gkind = (half if tz else "f32"), (half if tg else "f32")
    zt = z_as((1.3 * rng.standard_normal((n, d))).astype(np.float32), zkind)
    gt = z_as(rng.standard_normal((n, d)).astype(np.float32), gkind)
    e = rng.standard_normal((k, d)).astype(np.float32)
    idx = rng.integers(0, k, n).astype(np.int64)
    gl, coef = np.float32(1.7), np.float32(0.37)
    zg, gg, eg, ig = zt.to(gpu), gt.to(gpu), torch.from_numpy(e).to(gpu), torch.from_numpy(idx).to(gpu)
    glg = torch.tensor(float(gl), dtype=torch.float32, device=gpu) if with_loss else None
    gz = Guarded((n, d), DT[zkind], gpu)
    L.call("vq3d_vq_bwd", L.dtype_code(zg), L.ptr(zg), n, d, L.ptr(eg), L.ptr(ig), L.dtype_code(gg), L.ptr(gg),
           L.ptr(glg), float(coef), L.ptr(gz.t), L.stream())
    got = finish(None, gz=gz)["gz"].float().numpy().astype(np.float64)
    g = gt.float().numpy().astype(np.float64)
    t = (float(gl) if with_loss else 0.0) * float(coef) * (zt.float().numpy().astype(np.float64) - e[idx])
    ref = g + t
    bound = 4 * ulp_of(ref, zkind) + 2 * U * (np.abs(g) + np.abs(t))
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


# ------------------------------------------------------------------------------------------ f) the module
def test_quantizer_three_steps_vs_oracle(gpu):
    """Quantizer(64, 8) on a bf16 z of 13,824 rows (split search, LANES = 4 statistics reduce):
    first-pass init and three EMA steps; codes bit-exact, buffers within the project's 2e-5."""
    from oracle import vqvae_cpu as O
    from vq3d import functional as Fn
    from vq3d.layers import Quantizer
    torch.manual_seed(23)
    q = Quantizer(64, 8, 0.1)
    sd = {n: b.clone() for n, b in q.state_dict().items()}
    q = q.to(gpu).train()
    gen = torch.Generator().manual_seed(29)
    for step in range(3):
        z = (0.2 + 1.3 * torch.randn((2, 8, 24, 24, 12), generator=gen)).bfloat16()
        _, _, idx = Fn.QuantizeFn.apply(z.to(gpu).contiguous(memory_format=torch.channels_last_3d), q)
        _, _, ridx = O.quantize(sd, "", z.float(), True)
        torch.cuda.synchronize()
        match = float((idx.cpu() == ridx).float().mean())
        assert torch.equal(idx.cpu(), ridx), (step, match)
        for b in ("embed", "embed_avg", "cluster_size"):
            got, ref = getattr(q, b).double().cpu(), sd[b].double()
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err < 2e-5, (step, b, err)
        assert int(q.first_pass) == int(sd["first_pass"]) == 0
