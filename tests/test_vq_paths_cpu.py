"""CPU side of tests/test_gpu_vq_paths.py: a mirror of the host dispatch of csrc/vq.hip (plan_vq,
the DM buckets, the LANES choice of the statistics reduce, the row blocks of the moments) asserts
that the GPU test's case tables reach every path they name -- if a threshold moves, the failing
assertion says which case to re-aim -- and the references alone are held inside the bounds the
GPU tests state."""
import math

import numpy as np
import torch

import test_gpu_vq_paths as T

LDS_FLOATS = 16384  # kLdsCodebookFloats
U = T.U


# ------------------------------------------------------------------------------------------ mirror of the host
def plan(n, d, k, cap=True):
    """(row blocks, chunks, codes per chunk) of plan_vq; cap=False: without the LDS cap"""
    nb, nc = -(-n // 256), 1
    if nb < 128 and d <= 64:
        nc = min(max(1, 512 // nb), max(1, k // 8))
        if cap and nc > 1:
            nc = max(nc, -(-k // (LDS_FLOATS // d)))
    ck = -(-k // nc)
    return nb, -(-k // ck), ck


def bucket(d, split):
    return next((m for m in ((8, 16, 32, 64) if split else (2, 4, 8, 16, 32, 64)) if d <= m), "wide")


def lanes(n):
    nb, ln = -(-n // 256), 1
    while ln < 64 and ln * 16 < nb:
        ln *= 2
    return ln


def moment_blocks(n):
    rpb = max(256, -(-n // 1024))
    return rpb, -(-n // rpb)


def all_nearest():
    n0, n1, d, k = T.NEAREST_BOUNDARY
    return (T.NEAREST_SINGLE_SMALL + T.NEAREST_SINGLE_LARGE + T.NEAREST_WIDE + T.NEAREST_SPLIT + T.NEAREST_CAPPED +
            [(n0, d, k), (n1, d, k)] + list(T.NEAREST_TIES.values()) + T.NEAREST_NEAR + T.NEAREST_STORAGE)


# ------------------------------------------------------------------------------------------ coverage
def test_tables_take_the_paths_they_name():
    for c in T.NEAREST_SINGLE_SMALL + T.NEAREST_SINGLE_LARGE:
        assert plan(*c)[1] == 1 and c[1] <= 64, f"{c} no longer takes the single pass"
    for c in T.NEAREST_WIDE:
        assert plan(*c)[1] == 1 and c[1] > 64, f"{c} no longer takes the wide kernel"
    for c in T.NEAREST_SPLIT + T.NEAREST_CAPPED:
        assert plan(*c)[1] > 1, f"{c} no longer takes the split search"
    n0, n1, d, k = T.NEAREST_BOUNDARY
    assert n1 == n0 + 1 and plan(n0, d, k)[1] > 1 and plan(n1, d, k)[1] == 1, "the path boundary moved"
    assert plan(*T.NEAREST_TIES["single"])[1] == 1 and plan(*T.NEAREST_TIES["split"])[1:] == (8, 8)
    g = T.NEAREST_TIES["global"]
    assert plan(*g)[1] == 1 and g[1] * g[2] > LDS_FLOATS
    assert plan(300, 7, 100)[1:] == (12, 9)  # 12 chunks of 9, the last holds one code


def test_tables_reach_every_nearest_path():
    single = [c for c in all_nearest() if plan(*c)[1] == 1]
    split = [c for c in all_nearest() if plan(*c)[1] > 1]
    for m in (2, 4, 8, 16, 32, 64):
        hit = [c for c in single if bucket(c[1], False) == m]
        assert hit, f"no single-pass case with DM = {m}"
        assert {c[1] for c in hit} >= {m // 2 + 1 if m > 2 else 1, m}, f"DM = {m}: both ends of the bucket"
        assert any(c[1] % 4 for c in hit) or m == 4 and any(c[1] == 3 for c in hit), f"DM = {m}: no FMA tail"
    for m in (8, 16, 32, 64):
        assert any(bucket(c[1], True) == m for c in split), f"no split case with DM = {m}"
    assert any(c[1] > 64 and c[1] % 4 for c in single) and any(c[1] > 64 and c[1] % 4 == 0 for c in single)
    in_lds = [c for c in single if c[1] <= 64 and c[1] * c[2] <= LDS_FLOATS]
    in_glob = [c for c in single if c[1] <= 64 and c[1] * c[2] > LDS_FLOATS]
    assert any(c[1] * c[2] == LDS_FLOATS for c in in_lds), "the last codebook size held in LDS"
    assert any(c[1] * c[2] == LDS_FLOATS + c[1] for c in in_glob), "the first codebook size read from memory"
    assert any(c[2] % plan(*c)[2] for c in split), "no split case whose last chunk is short"
    assert any(c[0] % 256 for c in split) and any(c[0] % 256 for c in single), "a partial last row block"
    assert any(plan(*c)[0] > 1 for c in split) and any(plan(*c)[0] > 1 for c in single), "more than one row block"
    # every TZ x TQ instantiation family: single pass in LDS, from memory, wide, split
    st = T.NEAREST_STORAGE
    assert any(c in in_lds for c in st) and any(c in in_glob for c in st) and any(c[1] > 64 for c in st)
    assert {bucket(c[1], True) for c in st if plan(*c)[1] > 1} >= {8, 32}


def test_split_never_asks_for_more_than_the_lds_cap():
    for c in all_nearest():
        _, nchunk, ck = plan(*c)
        if nchunk > 1:
            assert ck * c[1] <= LDS_FLOATS, f"{c}: {ck * c[1] * 4} B of LDS per workgroup"
    assert any(plan(*c, cap=False)[2] * c[1] > LDS_FLOATS for c in T.NEAREST_CAPPED), "no case needs the cap"
    assert any(plan(*c)[2] * c[1] == LDS_FLOATS for c in T.NEAREST_CAPPED), "no case exactly at the cap"
    # user-reachable codebooks (--num-embeddings): any k fits once capped
    for n, d, k in [(16384, 64, 8192), (1, 64, 100000), (32512, 64, 65536), (300, 33, 70001)]:
        _, nchunk, ck = plan(n, d, k)
        assert ck * d <= LDS_FLOATS and (nchunk - 1) * ck < k <= nchunk * ck


def test_tables_reach_every_statistics_path():
    cases = T.STATS_CASES
    assert {lanes(c[0]) for c in cases} == {1, 2, 4, 8, 16, 32, 64}
    assert all(lanes(c[0]) >= 2 for c in T.STATS_16BIT) and set(T.STATS_16BIT) <= set(cases)
    assert any(c[0] < 8 for c in cases), "only the scalar tail loop"
    assert any(c[0] % 8 and c[0] > 256 for c in cases), "a tail after the 8-row loop in a later block"
    assert any((c[2] * (c[1] + 1)) % 256 for c in cases) and any(c[2] * (c[1] + 1) > 256 for c in cases)
    assert any(-(-c[2] * (c[1] + 1) // 256) == 66 for c in cases), "66 entry tiles"
    assert {k > 1024 for k in T.UPDATE_K} == {True, False} and 1024 in T.UPDATE_K and 1025 in T.UPDATE_K
    rpb, nb = moment_blocks(300000)
    assert (300000, 2) in T.MOMENTS_CASES and rpb == 293 and 300000 % rpb and nb <= 1024
    assert any(d > 64 for _, d in T.MOMENTS_CASES) and T.MOMENTS_16BIT[1] > 64, "two fin blocks"


# ------------------------------------------------------------------------------------------ the data
def test_tie_cases_hold_exact_ties():
    from oracle import vq_oracle
    for name, (n, d, k) in T.NEAREST_TIES.items():
        z, e = T.nearest_inputs(n, d, k, name)
        dist = np.sort(vq_oracle.cdist(z[:2048], e), axis=1)
        ties = int((dist[:, 0] == dist[:, 1]).sum())
        assert ties >= 15, (name, ties)
    e = T.nearest_inputs(*T.NEAREST_TIES["split"], "split")[1]
    ck = plan(*T.NEAREST_TIES["split"])[2]
    assert np.array_equal(e[ck - 1], e[ck]) and np.array_equal(e[0], e[-1])


def _argmin_variant(z, e, fma_head, fma_tail):
    """first-index argmin of the cdist arithmetic with an FMA (emulated in float64: the product of
    two fp32 values is exact there) or a rounded product in the head / tail terms"""
    d = z.shape[1]
    acc = np.zeros((z.shape[0], e.shape[0]), np.float32)
    for i in range(d):
        t = z[:, i, None] - e[None, :, i]
        if fma_head if i < 4 * (d // 4) else fma_tail:
            acc = (acc.astype(np.float64) + t.astype(np.float64) ** 2).astype(np.float32)
        else:
            acc = acc + t * t
    return np.argmin(np.sqrt(acc), axis=1)


def test_near_duplicate_cases_tell_the_roundings_apart():
    from oracle import vq_oracle
    paths = set()
    for n, d, k in T.NEAREST_NEAR:
        nb, nchunk, _ = plan(n, d, k)
        paths.add("split" if nchunk > 1 else "wide" if d > 64 else "lds" if d * k <= LDS_FLOATS else "global")
        assert d % 4 and d > 4
        z, e = T.nearest_inputs(n, d, k, "near")
        z = z[:1024]
        ref = vq_oracle.nearest(z, e)[0]
        assert int((_argmin_variant(z, e, False, True) != ref).sum()) <= 2  # the emulation is the oracle
        no_fma = int((_argmin_variant(z, e, False, False) != ref).sum())
        all_fma = int((_argmin_variant(z, e, True, True) != ref).sum())
        print(f"near duplicates {(n, d, k)}: {no_fma} rows flip without the tail FMA, {all_fma} with FMA everywhere")
        assert no_fma >= 15 and all_fma >= 15, (n, d, k, no_fma, all_fma)
    assert paths == {"lds", "global", "wide", "split"}


def test_subset_rows():
    for n, _, _ in T.NEAREST_CAPPED:
        r = T.subset_rows(n)
        assert r[0] == 0 and r[-1] == n - 1 and (np.diff(r) > 0).all() and np.diff(r).max() <= 17
        assert (r[:256] == np.arange(256)).all() and (r[-300:] == np.arange(n - 300, n)).all()


# ------------------------------------------------------------------------------------------ the bounds
def test_ema_update_restatement_inside_the_bounds():
    """torch fp32 restatement of layers.py:649-663 (what the kernel has to reproduce) against the
    float64 reference: inside the cluster_size / embed_avg bounds, and well inside embed's."""
    worst = 0.0
    for k in T.UPDATE_K:
        for d in T.UPDATE_D:
            _, embed_avg, cs, counts, dw = T.update_inputs(k, d)
            assert counts.sum() > 0
            if k > 1:
                assert abs((cs == 0).mean() - 1 / 3) < 0.01 + 1 / k and abs((counts == 0).mean() - 1 / 5) < 0.01 + 1 / k
            tcs, tea = torch.from_numpy(cs.copy()), torch.from_numpy(embed_avg.copy())
            tcs.mul_(T.DECAY).add_(torch.from_numpy(counts), alpha=1 - T.DECAY)
            tea.mul_(T.DECAY).add_(torch.from_numpy(dw), alpha=1 - T.DECAY)
            ntot = tcs.sum()
            smoothed = ntot * ((tcs + T.ALPHA) / (ntot + k * T.ALPHA))
            te = tea / smoothed.unsqueeze(-1)
            cs_r, ea_r, e_r, mag, sm = T.update_reference(embed_avg, cs, counts, dw)
            assert (np.abs(tcs.double().numpy() - cs_r) <= 4 * U * np.abs(cs_r)).all(), (k, d)
            assert (np.abs(tea.double().numpy() - ea_r) <= 3 * U * mag).all(), (k, d)
            bound = T.embed_bound(k, mag, sm)
            err = np.abs(te.double().numpy() - e_r)
            assert (err <= bound).all(), (k, d)
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"torch fp32 restatement: worst embed err / bound {worst:.3f}")
    assert worst <= 0.5


def test_ema_update_needs_the_double_decay():
    """fl32(1 - decay) cannot be had from fl32(decay): at 0.99 the two differ by ~100 ulp, which a
    code without history (cluster_size = counts * (1 - decay)) shows in full."""
    omd_ref = np.float32(1 - T.DECAY)
    omd_from_f32 = np.float32(1.0 - float(np.float32(T.DECAY)))
    assert abs(float(omd_from_f32) - float(omd_ref)) / float(omd_ref) > 4 * U


def _moments_two_pass(x32, centre_fp32):
    """the kernel's arithmetic: fp64 partials per row block in block order, fp64 division, casts"""
    n = x32.shape[0]
    rpb, nb = moment_blocks(n)
    x = x32.astype(np.float64)
    blocks = [x[b * rpb:(b + 1) * rpb] for b in range(nb)]
    mean = sum(b.sum(axis=0) for b in blocks) / n
    mu = mean.astype(np.float32).astype(np.float64) if centre_fp32 else mean
    var = sum(((b - mu) ** 2).sum(axis=0) for b in blocks) / (n - 1)
    return mean.astype(np.float32), np.sqrt(var).astype(np.float32)


def test_moments_restatement_inside_2_ulp():
    cases = [(n, d, False) for n, d in T.MOMENTS_CASES] + [T.MOMENTS_OFFSET + (True,)]
    for n, d, offset in cases:
        x32 = T.moments_inputs(n, d, offset)
        x = x32.astype(np.float64)
        mean, std = _moments_two_pass(x32, centre_fp32=False)
        for got, ref in ((mean, x.mean(axis=0)), (std, x.std(axis=0, ddof=1))):
            assert (np.abs(got.astype(np.float64) - ref) <= 2 * T.ulp32(ref)).all(), (n, d)
    # centred on the fp32-rounded mean the variance gains (mean error / std)^2 relative: the large-mean
    # case is there to tell the two apart
    x32 = T.moments_inputs(*T.MOMENTS_OFFSET, offset=True)
    _, std = _moments_two_pass(x32, centre_fp32=True)
    ref = x32.astype(np.float64).std(axis=0, ddof=1)
    assert (np.abs(std.astype(np.float64) - ref) > 2 * T.ulp32(ref)).any()


def test_sq_bound_counts_the_additions():
    """(d + ceil(nb_near / 256) + 24) * 2^-23 covers the longest chain of rounded fp32 additions from
    a term to the result: d in the row, 6 + 4 in the block tree, ceil(nb / 256) + 6 + 4 in the sum of
    the partials, and 2 for the square of the rounded difference."""
    for n, d, k in all_nearest():
        nb = -(-n // 256)
        chain = d + (6 + 4) + math.ceil(nb / 256) + (6 + 4) + 2
        assert chain <= d + math.ceil(nb / 256) + 24
