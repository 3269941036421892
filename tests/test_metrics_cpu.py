"""CPU: the validation metrics (vq3d/metrics.py, vq3d/evaluate.py) without a GPU.

The comparator below is an independent float64 numpy / scipy restatement of the definition in
include/vq3d.h (vq3d_slice_metrics): `scipy.ndimage.correlate1d` with the normalised 11-tap
Gaussian along h and w, then the 5-pixel border cropped, which leaves exactly the windows that lie
wholly inside a slice.  It never calls vq3d.metrics.  PyTorch-Lightning is not available, so the
implementation is pinned to this definition, not to a run of PL's `ssim`.

Tolerances (shared with tests/test_gpu_metrics.py): an fp32 evaluation of the definition differs
from float64 on these shapes by at most 5.1e-7 in the mean SSIM and 5.0e-6 in one slice, so the
bounds are 20x / 10x that (1e-5, 5e-5) to leave room for another summation order; mse and nmse
relative 1e-5 (fp32 partial sums, double finish, at most ~1.4e5 voxels), psnr 1e-4 dB (the same bound
through 10 log10), the computed data range to fp32 rounding."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import correlate1d

# (shape, nvs, cylinder): the issue's table, then two shapes that cross every tile edge of the kernel
# (csrc/metrics.hip: 16 output columns x 64 d per workgroup, H cut into segments of >= 32 output rows)
CASES = [
    ((1, 1, 11, 11, 4), [3], False),       # one window per slice; D below a wave
    ((2, 1, 12, 19, 8), [8, 5], False),    # batch; odd W; nvs differs per element
    ((1, 1, 24, 40, 16), [15], False),
    ((2, 1, 43, 37, 24), [24, 17], False),  # odd sizes; D not a power of two
    ((1, 1, 64, 64, 32), [31], False),
    ((1, 1, 32, 32, 8), [8], True),        # centre cylinder; square, for the mask
    # H - 10 = 65 = 33 + 32: two row segments (the second one row shorter); W - 10 = 19 = 16 + 3: two
    # column strips, the second partial; D = 66 = 64 + 2: two d chunks, the second two lanes wide, and
    # D % 4 != 0 takes the scalar-load staging path
    ((1, 1, 75, 29, 66), [60], False),
    # the vector-load staging path (D % 4 == 0) across a d-chunk edge (68 = 64 + 4) and a strip edge
    # (W - 10 = 18 = 16 + 2), with the cylinder
    ((1, 1, 30, 28, 68), [68], True),
]
TOL_SSIM, TOL_SLICE, RTOL_MSE, TOL_PSNR = 1e-5, 5e-5, 1e-5, 1e-4


@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    """(target fp32, pred bf16): a smooth target -- the trilinear upsample of a coarse uniform field
    in [-0.5, 4] -- and the target plus noise rounded to bf16."""
    g = torch.Generator().manual_seed(sum(s * 131 ** i for i, s in enumerate(shape)))
    coarse = [max(2, n // 8 + 1) for n in shape[2:]]
    field = torch.rand((shape[0], 1, *coarse), generator=g) * 4.5 - 0.5
    x = torch.nn.functional.interpolate(field, size=shape[2:], mode="trilinear", align_corners=True).contiguous()
    pred = (x + 0.1 * torch.randn(shape, generator=g)).to(torch.bfloat16)
    return x, pred


def reference_metrics(pred, target, nvs, elu, cylinder, data_range, k1=0.01, k2=0.03, psnr_range=4.0):
    """float64: dict of ssim, ssim_per_slice (B, D), mse, nmse, psnr, data_range."""
    p = pred.double().numpy().copy()
    t = target.double().numpy()
    b, _, h, w, d = p.shape
    if elu:
        p = np.where(p > 0, p, np.expm1(np.minimum(p, 0)))
    for i, n in enumerate(nvs):
        p[i, ..., int(n):] = 0.0
    rng = float(data_range) if data_range is not None else max(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    g = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    g /= g.sum()

    def win(a):
        a = correlate1d(correlate1d(a, g, axis=2, mode="constant"), g, axis=3, mode="constant")
        return a[:, :, 5:h - 5, 5:w - 5, :]
    mp, mt = win(p), win(t)
    spp, stt, spt = win(p * p) - mp * mp, win(t * t) - mt * mt, win(p * t) - mp * mt
    with np.errstate(invalid="ignore", divide="ignore"):
        smap = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    per_slice = smap.mean(axis=(2, 3)).reshape(b, d)
    hh, ww = np.arange(h)[:, None], np.arange(w)[None, :]
    m = ((2 * hh - h) ** 2 + (2 * ww - w) ** 2 <= min(h, w) ** 2) if cylinder else np.ones((h, w), bool)
    m = m[None, None, :, :, None]
    sse, st2, count = (((p - t) ** 2) * m).sum(), ((t * t) * m).sum(), b * d * int(m.sum())
    mse = sse / count
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(psnr_range ** 2 / mse)
    return {"ssim": per_slice.mean(), "ssim_per_slice": per_slice, "mse": mse, "nmse": sse / st2, "psnr": psnr,
            "data_range": rng}


def check_against_reference(q, ref):
    """Print every figure, then hold it to the tolerances of the module docstring."""
    got = {k: getattr(q, k).detach().cpu().double().numpy() for k in q._fields}
    d_slice = float(np.abs(got["ssim_per_slice"] - ref["ssim_per_slice"]).max())
    print(f"ssim {got['ssim']:.9f} ref {ref['ssim']:.9f} diff {abs(got['ssim'] - ref['ssim']):.2e}; slice diff "
          f"{d_slice:.2e}; mse {got['mse']:.9e} ref {ref['mse']:.9e}; nmse {got['nmse']:.9e} ref {ref['nmse']:.9e}; "
          f"psnr {got['psnr']:.6f} ref {ref['psnr']:.6f}; range {got['data_range']:.7f} ref {ref['data_range']:.7f}")
    assert got["ssim_per_slice"].shape == ref["ssim_per_slice"].shape
    assert abs(got["ssim"] - ref["ssim"]) <= TOL_SSIM
    assert d_slice <= TOL_SLICE
    assert abs(got["mse"] - ref["mse"]) <= RTOL_MSE * ref["mse"]
    assert abs(got["nmse"] - ref["nmse"]) <= RTOL_MSE * ref["nmse"]
    assert abs(got["psnr"] - ref["psnr"]) <= TOL_PSNR
    assert got["data_range"] == pytest.approx(ref["data_range"], rel=2.0 ** -22)


@pytest.mark.parametrize("data_range", [None, 4.24])
@pytest.mark.parametrize("activation", ["elu", "none"])
@pytest.mark.parametrize("shape,nvs,cylinder", CASES)
def test_cpu_path_matches_float64_definition(shape, nvs, cylinder, activation, data_range):
    from vq3d.metrics import slice_metrics
    x, pred = make_inputs(shape)
    q = slice_metrics(pred, x, torch.tensor(nvs), activation=activation, cylinder=cylinder, data_range=data_range)
    assert not q.ssim.is_cuda and q.ssim_per_slice.shape == (shape[0], shape[4])
    check_against_reference(q, reference_metrics(pred, x, nvs, activation == "elu", cylinder, data_range))


def test_identical_volumes_score_one():
    import vq3d
    x, _ = make_inputs((2, 1, 12, 19, 8))
    for data_range in (None, 4.24):
        q = vq3d.slice_metrics(x, x, data_range=data_range)
        assert abs(float(q.ssim) - 1.0) <= 1e-6 and float((q.ssim_per_slice - 1).abs().max()) <= 1e-6
        assert float(q.nmse) == 0.0 and float(q.mse) == 0.0 and math.isinf(float(q.psnr)) and float(q.psnr) > 0
    assert abs(float(vq3d.SSIM3DSlices()(x, x)) - 1.0) <= 1e-6


def test_module_and_helpers_follow_the_reference_interface():
    import vq3d
    x, pred = make_inputs((1, 1, 24, 40, 16))
    m = vq3d.SSIM3DSlices(data_range=4.24)
    ref = reference_metrics(pred, x, [16], False, False, 4.24)
    assert abs(float(m(pred, x)) - ref["ssim"]) <= TOL_SSIM
    p = pred.float()
    assert float(vq3d.nmse(x, p)) == pytest.approx(ref["nmse"], rel=1e-5)
    assert float(vq3d.psnr(x, p, 4)) == pytest.approx(ref["psnr"], abs=1e-4)
    # a constant pair has data range 0: NaN, as the formula gives
    z = torch.zeros((1, 1, 11, 11, 2))
    assert math.isnan(float(vq3d.slice_metrics(z, z).ssim))


def test_bad_arguments_are_refused():
    import vq3d
    x = torch.zeros((1, 1, 10, 16, 4))
    with pytest.raises(ValueError, match="at least 11"):
        vq3d.slice_metrics(x, x)
    with pytest.raises(ValueError, match="at least 11"):
        vq3d.slice_metrics(x.transpose(2, 3), x.transpose(2, 3))
    y = torch.zeros((1, 1, 11, 11, 4))
    with pytest.raises(ValueError, match="data_range"):
        vq3d.slice_metrics(y, y, data_range=0.0)
    with pytest.raises(ValueError, match="k1"):
        vq3d.slice_metrics(y, y, k1=-0.01)
    with pytest.raises(ValueError, match="activation"):
        vq3d.slice_metrics(y, y, activation="relu")
    with pytest.raises(TypeError, match="fp32"):
        vq3d.slice_metrics(y, y.double())
    with pytest.raises(ValueError, match="kernel_size"):
        vq3d.SSIM3DSlices(kernel_size=(7, 7))
    with pytest.raises(ValueError, match="sigma"):
        vq3d.SSIM3DSlices(sigma=(1.0, 1.0))


def test_c_entry_validates_before_any_launch():
    from vq3d import _lib as L
    lib = L.load()
    assert L.query("vq3d_slice_metrics_workspace_size", 1, 512, 512, 128) > 0
    assert L.query("vq3d_slice_metrics_workspace_size", 1, 10, 512, 128) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(pred=p, target=p, nvs=p, h=16, w=16, k1=0.01, k2=0.03, per_slice=p, stats=p, ws=p):
        return lib.vq3d_slice_metrics(L.F32, pred, target, nvs, 1, h, w, 4, 1, 0, 0.0, k1, k2, 4.0, per_slice, stats,
                                      ws, None)
    for kw in ({"pred": None}, {"target": None}, {"nvs": None}, {"per_slice": None}, {"stats": None}, {"ws": None}):
        assert call(**kw) < 0 and b"null" in lib.vq3d_last_error(), kw
    assert call(h=10) < 0 and b"at least 11" in lib.vq3d_last_error()
    assert call(w=10) < 0 and b"at least 11" in lib.vq3d_last_error()
    assert call(h=0) < 0 and b"bad sizes" in lib.vq3d_last_error()
    assert call(k1=-1.0) < 0 and b"negative" in lib.vq3d_last_error()
    assert call(k2=-1.0) < 0 and b"negative" in lib.vq3d_last_error()


def test_fake_operator_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import vq3d.library as Lb
    assert "slice_metrics" in Lb.OPS
    with FakeTensorMode(allow_non_fake_inputs=True):
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            pred = torch.empty((2, 1, 43, 37, 24), dtype=dt, device="cuda")
            x = torch.empty((2, 1, 43, 37, 24), device="cuda")
            nvs = torch.empty(2, dtype=torch.int64, device="cuda")
            per_slice, stats = torch.ops.vq3d.slice_metrics(pred, x, nvs, True, False, 0.0, 0.01, 0.03, 4.0)
            assert tuple(per_slice.shape) == (2, 24) and per_slice.dtype == torch.float32
            assert tuple(stats.shape) == (5,) and stats.dtype == torch.float32
            assert per_slice.device.type == "cuda" and stats.device.type == "cuda"


# ------------------------------------------------------------------------------------------------ vq3d.evaluate
def test_evaluate_arguments():
    from vq3d import evaluate as E
    a = E.parse_arguments(["/data/ct", "/runs/last.ckpt"])
    assert str(a.dataset_path) == "/data/ct" and str(a.ckpt_path) == "/runs/last.ckpt"
    assert a.split == "val" and a.batch_size == 5 and a.out is None
    a = E.parse_arguments(["d", "c", "--split", "both", "--batch-size", "2", "--out", "r.json"])
    assert a.split == "both" and a.batch_size == 2 and str(a.out) == "r.json"
    with pytest.raises(SystemExit):
        E.parse_arguments(["d", "c", "--split", "test"])
    assert E.splits_of("val") == ["val"] and E.splits_of("train") == ["train"]
    assert E.splits_of("both") == ["val", "train"]
    with pytest.raises(ValueError):
        E.splits_of("test")
    assert E.DATA_RANGE == pytest.approx(4.24) and E.PSNR_RANGE == 4.0


def test_evaluate_report_layout(tmp_path):
    """The host half of vq3d.evaluate on real metric values (the CPU path of slice_metrics)."""
    import vq3d
    from vq3d import evaluate as E
    recs = []
    for shape in ((1, 1, 12, 19, 8), (1, 1, 24, 40, 16)):
        x, pred = make_inputs(shape)
        q = vq3d.slice_metrics(pred, x, activation="elu", data_range=E.DATA_RANGE, psnr_range=E.PSNR_RANGE)
        recs.append(E.volume_record(len(recs), q))
    assert recs[1]["index"] == 1 and len(recs[0]["ssim_per_slice"]) == 8 and len(recs[1]["ssim_per_slice"]) == 16
    assert recs[0]["ssim"] == pytest.approx(np.mean(recs[0]["ssim_per_slice"]), abs=1e-6)
    args = E.parse_arguments([str(tmp_path), str(tmp_path / "last.ckpt"), "--split", "both",
                              "--out", str(tmp_path / "sub" / "report.json")])
    report = E.make_report(args, {"val": recs, "train": []})
    E.write_report(report, args.out)
    back = json.loads((tmp_path / "sub" / "report.json").read_text())
    assert back == report and list(back["splits"]) == ["val", "train"]
    val = back["splits"]["val"]
    assert val["count"] == 2 and [v["index"] for v in val["volumes"]] == [0, 1]
    for k in ("ssim", "nmse", "psnr"):
        assert val["mean"][k] == pytest.approx((recs[0][k] + recs[1][k]) / 2)
    assert back["splits"]["train"] == {"count": 0, "mean": {"ssim": None, "nmse": None, "psnr": None}, "volumes": []}
    assert back["seed"] == 42 and back["data_range"] == pytest.approx(4.24) and back["psnr_range"] == 4.0


def test_evaluate_main_needs_a_gpu(tmp_path):
    """Without a device main refuses (the model has no CPU path); tests/test_gpu_metrics.py runs it
    end to end."""
    from vq3d import evaluate as E
    if torch.cuda.is_available():
        return

    class Tiny:
        batch_size, num_workers = 1, 0

        def setup(self, stage=None):
            x, _ = make_inputs((1, 1, 12, 19, 8))
            self.train_dataset = self.val_dataset = [(x[0], 8)]
    with pytest.raises(RuntimeError, match="GPU"):
        E.main(E.parse_arguments([str(tmp_path), str(tmp_path / "last.ckpt")]), datamodule=Tiny())
