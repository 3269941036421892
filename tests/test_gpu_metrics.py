"""GPU: the fused slice-wise SSIM / NMSE / PSNR kernel (csrc/metrics.hip) against the float64
comparator of tests/test_metrics_cpu.py (same shapes, inputs and tolerances: see that module's
docstring), its determinism, its two bindings, and the model / train / evaluate paths that log it."""
import json

import pytest
import torch

from test_metrics_cpu import CASES, check_against_reference, make_inputs, reference_metrics

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("data_range", [None, 4.24])
@pytest.mark.parametrize("activation", ["elu", "none"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape,nvs,cylinder", CASES)
def test_kernel_matches_float64_definition(gpu, shape, nvs, cylinder, dtype, activation, data_range):
    from vq3d.metrics import slice_metrics
    x, pred = make_inputs(shape)
    pred = pred.to(DTYPES[dtype])  # the bf16-rounded values, exactly representable in all three formats
    q = slice_metrics(pred.to(gpu), x.to(gpu), torch.tensor(nvs, device=gpu), activation=activation,
                      cylinder=cylinder, data_range=data_range)
    assert q.ssim.is_cuda and q.ssim_per_slice.shape == (shape[0], shape[4])
    check_against_reference(q, reference_metrics(pred, x, nvs, activation == "elu", cylinder, data_range))


@pytest.mark.parametrize("shape,nvs,cylinder", [CASES[3], CASES[6]])
def test_two_calls_are_bit_identical(gpu, shape, nvs, cylinder):
    from vq3d.metrics import slice_metrics_kernel
    x, pred = make_inputs(shape)
    args = (pred.to(gpu), x.to(gpu), torch.tensor(nvs, device=gpu), True, cylinder, 0.0, 0.01, 0.03, 4.0)
    a = slice_metrics_kernel(*args)
    b = slice_metrics_kernel(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()


def test_operator_equals_ctypes_binding(gpu):
    import vq3d.library  # noqa: F401
    from vq3d import functional as Fn
    from vq3d.metrics import slice_metrics, slice_metrics_kernel
    shape, nvs, _ = CASES[3]
    x, pred = make_inputs(shape)
    args = (pred.to(gpu), x.to(gpu), torch.tensor(nvs, device=gpu), True, True, 0.0, 0.01, 0.03, 4.0)
    a = slice_metrics_kernel(*args)
    b = torch.ops.vq3d.slice_metrics(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    try:  # the public function follows the chosen binding
        Fn.set_binding("library")
        q = slice_metrics(args[0], args[1], args[2], activation="elu", cylinder=True)
    finally:
        Fn.set_binding("ctypes")
    assert torch.equal(q.ssim_per_slice, a[0]) and torch.equal(q.ssim, a[1][0]) and torch.equal(q.psnr, a[1][3])


def _small_model(gpu, **kw):
    import vq3d
    torch.manual_seed(0)
    return vq3d.VQVAE(vq3d.default_args(n_bottleneck_blocks=2, compute_dtype="fp32", **kw)).to(gpu)


@pytest.mark.parametrize("cylinder", [True, False])
def test_validation_step_logs_quality_metrics(gpu, cylinder):
    from vq3d import functional as Fn
    from vq3d.metrics import slice_metrics
    m = _small_model(gpu, extract_center_cylinder=cylinder).eval()
    x = (torch.rand((1, 1, 32, 32, 32), generator=torch.Generator().manual_seed(1234)) * 4.5 - 0.5).to(gpu)
    nvs = torch.tensor([29], device=gpu)
    cap = {}
    fwd = m.forward

    def capture(data):
        cap["r"] = fwd(data)
        return cap["r"]
    m.forward = capture
    with torch.no_grad():
        m.validation_step((x, nvs), 0)
        val = dict(m.logged)
        loc, (commit, *_) = cap["r"]
        q = slice_metrics(loc, x, nvs, activation="elu", cylinder=cylinder, psnr_range=4.0)
        _, recon = Fn.recon_loss(loc, x, nvs, cylinder, *commit)
        m.logged.clear()
        m.training_step((x, nvs), 0)
    del m.forward
    for key, ref in (("val_ssim_mean", q.ssim), ("val_nmse", q.nmse), ("val_psnr", q.psnr)):
        assert torch.equal(val[key], ref) and torch.isfinite(val[key]), key
    # the loss is what it was without the metrics, and training logs none of them
    assert torch.equal(val["val_recon_loss_mean"], recon)
    assert "train_recon_loss_mean" in m.logged
    assert not [k for k in m.logged if k.endswith(("ssim_mean", "nmse", "psnr"))]


class _Volumes:
    """A datamodule over four synthetic 32^3 volumes: three to train on, one to validate on."""
    batch_size, num_workers = 2, 0

    def setup(self, stage=None):
        from vq3d.utils import synthetic_volume
        vols = [(synthetic_volume((1, 32, 32, 32), i), 32 - i) for i in range(4)]
        self.train_dataset, self.val_dataset = vols[:3], vols[3:]


def test_validate_averages_the_metrics(gpu):
    from vq3d import train
    m = _small_model(gpu)
    dm = _Volumes()
    dm.setup()
    loader = torch.utils.data.DataLoader(dm.train_dataset, batch_size=1, shuffle=False)
    score = train.validate(m, loader, gpu)
    assert set(m.val_metrics) == set(train.VAL_KEYS) and score == m.val_metrics["val_recon_loss_mean"]
    per = {k: [] for k in train.VAL_KEYS}
    m.eval()
    with torch.no_grad():
        for x, nvs in loader:
            m.validation_step((x.to(gpu).float(), nvs.to(gpu)), 0)
            for k in per:
                per[k].append(float(m.logged[k]))
    for k, vals in per.items():
        assert m.val_metrics[k] == pytest.approx(sum(vals) / len(vals), rel=1e-12), k
    assert 0 < m.val_metrics["val_ssim_mean"] < 1 and m.val_metrics["val_nmse"] > 0


def test_evaluate_writes_the_report(gpu, tmp_path):
    from vq3d import evaluate as E
    from vq3d.checkpoint import save_checkpoint
    from vq3d.metrics import slice_metrics
    m = _small_model(gpu)
    ckpt = tmp_path / "last.ckpt"
    save_checkpoint(str(ckpt), m)
    out = tmp_path / "report.json"
    report = E.main(E.parse_arguments([str(tmp_path), str(ckpt), "--split", "both", "--batch-size", "2",
                                       "--out", str(out)]), datamodule=_Volumes())
    assert json.loads(out.read_text()) == report
    assert report["splits"]["val"]["count"] == 1 and report["splits"]["train"]["count"] == 3
    # one volume recomputed by hand: the model's output through slice_metrics at the script's settings
    m.eval()
    dm = _Volumes()
    dm.setup()
    x = dm.train_dataset[2][0][None].to(gpu)
    with torch.no_grad():
        dec, *_ = m(x)
        q = slice_metrics(dec, x, activation="elu", data_range=E.DATA_RANGE, psnr_range=4.0)
    rec = report["splits"]["train"]["volumes"][2]
    assert rec["index"] == 2 and len(rec["ssim_per_slice"]) == 32
    assert rec["ssim"] == pytest.approx(float(q.ssim), abs=1e-5) and rec["psnr"] == pytest.approx(float(q.psnr), abs=1e-3)
    means = report["splits"]["train"]["mean"]
    assert means["ssim"] == pytest.approx(sum(v["ssim"] for v in report["splits"]["train"]["volumes"]) / 3)
