"""No GPU: the definition of the prior's fused head + loss (vq3d.head_loss.head_loss_reference), the
argument surface and data module of vq3d.train_prior, and its metric dictionary."""
import math

import numpy as np
import pytest
import torch


def _case(n=37, c=16, k=24, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    hid = torch.randn((n, c), generator=g).to(dtype)
    w = torch.randn((k, c), generator=g) * (4.0 / c ** 0.5)
    b = torch.randn(k, generator=g)
    ta = torch.randint(0, k, (n,), generator=g)
    tb = torch.randint(0, k, (n,), generator=g)
    return hid, w, b, ta, tb


def _logp64(hid, w, b):
    return torch.log_softmax(b.double() + hid.double() @ w.double().t(), dim=1)


@pytest.mark.parametrize("lam", [None, 0.3, 0.0, 1.0])
def test_reference_matches_float64_log_softmax(lam):
    from vq3d.head_loss import head_loss, head_loss_reference
    hid, w, b, ta, tb = _case()
    lp = _logp64(hid, w, b)
    ce = lambda t: -lp.gather(1, t.view(-1, 1)).view(-1)  # noqa: E731
    ref = ce(ta) if lam is None else lam * ce(ta) + (1 - lam) * ce(tb)
    loss, pred = head_loss_reference(hid, w, b, ta, None if lam is None else tb, lam)
    assert loss.dtype == torch.float32 and pred.dtype == torch.int64
    # fp32 evaluation of logits of scale ~5 and a 24-term logsumexp: a few ulp of |logit| ~ 1e-5
    torch.testing.assert_close(loss.double(), ref, rtol=0, atol=2e-5)
    assert torch.equal(pred, lp.argmax(1))
    # the public entry takes CPU tensors to the same definition; lam as a tensor too
    loss2, pred2 = head_loss(hid, w, b, ta, None if lam is None else tb, None if lam is None else torch.tensor(lam))
    assert torch.equal(loss2, loss) and torch.equal(pred2, pred)


def test_two_target_identity():
    """loss = lam CE(a) + (1 - lam) CE(b), with CE from F.cross_entropy on the same fp32 logits"""
    from vq3d.head_loss import head_loss_reference
    hid, w, b, ta, tb = _case(seed=3)
    logits = b + hid @ w.t()
    F = torch.nn.functional
    lam = 0.37
    ce = lambda t: F.cross_entropy(logits, t, reduction="none")  # noqa: E731
    ref = lam * ce(ta) + (1 - lam) * ce(tb)
    loss, _ = head_loss_reference(hid, w, b, ta, tb, lam)
    torch.testing.assert_close(loss, ref, rtol=0, atol=1e-5)


def test_sixteen_bit_rows_round_the_weight():
    from vq3d.head_loss import head_loss_reference
    hid, w, b, ta, _ = _case(dtype=torch.bfloat16)
    lp = _logp64(hid.float(), w.to(torch.bfloat16).float(), b)
    loss, _ = head_loss_reference(hid, w, b, ta)
    torch.testing.assert_close(loss.double(), -lp.gather(1, ta.view(-1, 1)).view(-1), rtol=0, atol=2e-5)


def test_pred_takes_the_first_index_on_a_tie():
    from vq3d.head_loss import head_loss_reference
    k, c = 16, 8
    hid = torch.zeros((3, c))
    w = torch.zeros((k, c))
    b = torch.zeros(k)
    b[[5, 9, 12]] = 2.0  # three exact maxima
    _, pred = head_loss_reference(hid, w, b, torch.zeros(3, dtype=torch.int64))
    assert pred.tolist() == [5, 5, 5]
    _, pred = head_loss_reference(hid, w, torch.zeros(k), torch.zeros(3, dtype=torch.int64))
    assert pred.tolist() == [0, 0, 0]


def test_a_target_outside_the_codes_contributes_nothing():
    from vq3d.head_loss import head_loss_reference
    hid, w, b, ta, tb = _case(seed=5)
    lse = torch.logsumexp(b + hid @ w.t(), dim=1)
    loss, _ = head_loss_reference(hid, w, b, torch.full_like(ta, -1))
    torch.testing.assert_close(loss, lse, rtol=0, atol=1e-6)
    # one of two targets outside: only the other's logit is subtracted
    la, _ = head_loss_reference(hid, w, b, ta)
    loss, _ = head_loss_reference(hid, w, b, ta, torch.full_like(tb, 24), 0.25)
    torch.testing.assert_close(loss, lse - 0.25 * (lse - la), rtol=0, atol=1e-5)


def test_gradcheck_float64():
    from vq3d.head_loss import head_loss_reference
    hid, w, b, ta, tb = _case(n=5, c=8, k=8, seed=7)
    hid, w, b = (t.double().requires_grad_(True) for t in (hid, w, b))
    lam = torch.tensor(0.3, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda h, ww, bb: head_loss_reference(h, ww, bb, ta, tb, lam)[0], (hid, w, b))
    assert torch.autograd.gradcheck(lambda h, ww, bb: head_loss_reference(h, ww, bb, ta)[0], (hid, w, b))


def test_abi_limits_are_checked_on_the_host():
    """the entry points refuse what the kernel cannot run, before any launch (no GPU touched)"""
    import ctypes

    from vq3d import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    ok = dict(dtype=L.BF16, nrows=4, c=8, k=8, ldh=8, ldw=8)
    for kw, word in (({"dtype": L.F32}, b"16-bit"), ({"k": 4}, b"k % 8"), ({"k": 1032}, b"k <= 1024"),
                     ({"k": 12}, b"k % 8"), ({"c": 12}, b"multiple of 8"), ({"c": 1032}, b"1024"),
                     ({"ldh": 12}, b"strides"), ({"ldw": 4}, b"strides")):
        a = dict(ok, **kw)
        rc = lib.vq3d_prior_head_loss_fwd(a["dtype"], a["nrows"], a["c"], a["k"], p, a["ldh"], p, a["ldw"], p, p, None,
                                          None, p, p, p, None)
        assert rc != 0 and word in lib.vq3d_last_error(), (kw, lib.vq3d_last_error())
    rc = lib.vq3d_prior_head_loss_fwd(L.BF16, 4, 8, 8, p + 2, 8, p, 8, p, p, None, None, p, p, p, None)
    assert rc != 0 and b"aligned" in lib.vq3d_last_error()
    rc = lib.vq3d_prior_head_loss_bwd(L.F16, 4, 8, 8, p, 8, p, 8, p, p, None, None, p, p, p, 4, None)
    assert rc != 0 and b"strides" in lib.vq3d_last_error()


# ------------------------------------------------------------------ vq3d.train_prior
def test_parse_arguments_defaults_are_the_references():
    from vq3d import train_prior as TP
    a = TP.parse_arguments(["codes", "1", "--use-model", "pixelsnail"])
    # pixel_model/train.py:28-44
    assert (a.gpus, a.accelerator, a.benchmark, a.num_sanity_val_steps, a.precision) == ("-1", "ddp", True, 0, 16)
    assert (a.log_every_n_steps, a.val_check_interval, a.flush_logs_every_n_steps) == (50, 0.5, 100)
    assert a.weights_summary == "full" and a.max_epochs == 50000 and a.max_steps is None
    assert a.level == 1 and a.batch_size is None and a.use_model == "pixelsnail" and a.compute_dtype == "bf16"
    # PixelSNAIL.add_model_specific_args' defaults
    assert (a.model_dim, a.num_blocks, a.num_layers_per_block, a.mixup_alpha, a.lr) == (32, 5, 5, 0, 1e-5)
    assert a.use_conditioning is False and isinstance(a.dataset_path, str)


def test_pixelcnn_is_refused():
    from vq3d import train_prior as TP
    with pytest.raises(NotImplementedError, match="DESIGN.md §8"):
        TP.parse_arguments(["codes", "0", "--use-model", "pixelcnn"])
    with pytest.raises(NotImplementedError, match="DESIGN.md §8"):  # the reference's default model
        TP.parse_arguments(["codes", "0"])


def _store(root, n=40, levels=(16, 8)):
    from vq3d.extract import CodeStore
    g = np.random.default_rng(0)
    with CodeStore(str(root), list(levels), n) as st:
        for i in range(n):
            st.put(i, [g.integers(0, k, (1, 2, 2, 2)) + 0 * i for k in levels])
    return str(root)


def test_codes_datamodule_split(tmp_path):
    from vq3d import train_prior as TP
    from vq3d.extract import CodesDataset
    from vq3d.train import seed_everything
    root = _store(tmp_path / "codes")
    splits = []
    for _ in range(2):
        seed_everything(42)
        dm = TP.CodesDataModule(root, embedding_id=1, batch_size=2, num_workers=0)
        dm.setup()
        assert (len(dm.train_dataset), len(dm.val_dataset)) == (38, 2) == (dm.train_len, dm.val_len)
        tr, va = set(dm.train_dataset.indices), set(dm.val_dataset.indices)
        assert not tr & va and tr | va == set(range(40))
        splits.append((list(dm.train_dataset.indices), list(dm.val_dataset.indices)))
        assert dm.num_embeddings == CodesDataset(root, embedding_id=1).num_embeddings == [8, 0]
    assert splits[0] == splits[1]
    # loaders: drop_last on both, only the training one shuffles
    assert len(dm.train_dataloader()) == 19 and len(dm.val_dataloader()) == 1
    batch = next(iter(dm.val_dataloader()))
    assert tuple(batch[0].shape) == (2, 1, 2, 2, 2) and batch[0].dtype == torch.int64
    dm0 = TP.CodesDataModule(root, embedding_id=0, batch_size=2, num_workers=0)
    dm0.setup()
    assert dm0.num_embeddings == [16, 8]


def test_metric_dictionary():
    from vq3d import train_prior as TP
    rows = torch.tensor([[4.0, 1.0], [3.0, 2.0]])  # even count: the lower median is 2, not 2.5
    m = {k: float(v) for k, v in TP.loss_metrics(rows, "val").items()}
    assert set(m) == {"val_loss_min", "val_loss_max", "val_loss_mean", "val_loss_median", "val_loss_std",
                      "val_bits_per_dim"}
    assert (m["val_loss_min"], m["val_loss_max"], m["val_loss_mean"], m["val_loss_median"]) == (1.0, 4.0, 2.5, 2.0)
    assert m["val_loss_std"] == pytest.approx(math.sqrt(5.0 / 3.0), rel=1e-6)  # unbiased: / (n - 1)
    assert m["val_bits_per_dim"] == pytest.approx(2.5 / math.log(2), rel=1e-12)
    assert set(TP.VAL_KEYS) == set(m) | {"val_accuracy"}
    assert all(k.startswith("train_") for k in TP.loss_metrics(rows, "train"))


def test_onehot_by_scatter():
    from vq3d import train_prior as TP
    codes = torch.randint(0, 16, (2, 3, 4, 5), generator=torch.Generator().manual_seed(0))
    x = TP.onehot_codes(codes, 16)
    assert torch.equal(x, torch.nn.functional.one_hot(codes, 16).permute(0, 4, 1, 2, 3).float())
    assert x.is_contiguous(memory_format=torch.channels_last_3d)
