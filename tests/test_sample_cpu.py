"""CPU: the prior sampler's definition (vq3d/sample.py; include/vq3d.h, the prior sampling entry)
without a GPU -- the host restatement of the kernel (hash -> uniform -> Gumbel -> argmax), the driver
loop over an injected `hidden_fn`, the background crop of PixelSNAIL.hidden, the host-side checks of
the C entry and the operator's registration.  tests/test_gpu_sample.py holds the kernel to the same
restatement.

The distribution test is deterministic (fixed seed): chi-square of 20,000 draws against
softmax(logits / T) with K = 8, bound the 99.9 % quantile of chi-square with 7 degrees of freedom."""
import ctypes

import numpy as np
import pytest
import torch

CHI2_7_999 = 24.3219  # scipy.stats.chi2.ppf(0.999, 7)
LOGITS = np.array([[0.3, -1.2, 2.0, 0.5, 1.1, -0.4, 0.0, 1.7]], dtype=np.float32)
N_DRAWS = 20000
CL = torch.channels_last_3d


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_draws_follow_the_softmax(temperature):
    from vq3d import sample as S
    counts = np.zeros(LOGITS.shape[1])
    for p in range(N_DRAWS):  # one draw per position counter
        counts[S.draw_codes(LOGITS, temperature, 1234, 0, p)[0]] += 1
    prob = np.exp(LOGITS[0].astype(np.float64) / temperature)
    prob /= prob.sum()
    chi2 = float(((counts - N_DRAWS * prob) ** 2 / (N_DRAWS * prob)).sum())
    print(f"T = {temperature}: chi-square {chi2:.3f} (bound {CHI2_7_999})")
    assert chi2 < CHI2_7_999


def test_zero_temperature_is_the_first_argmax():
    from vq3d import sample as S
    tied = np.array([[1.0, 3.0, -2.0, 3.0, 0.0, 3.0, 1.0, 2.0]], dtype=np.float32)
    for p in range(200):
        assert S.draw_codes(LOGITS, 0.0, 1234, 0, p)[0] == 2
        assert S.draw_codes(tied, 0.0, 1234, p, p)[0] == 1


def test_uniform_is_strictly_inside_the_unit_interval():
    from vq3d import sample as S
    rng = np.random.default_rng(0)
    h = np.concatenate([np.array([0, 2 ** 32 - 1, 511, 512], dtype=np.uint32),
                        rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    u32, u64 = S.uniform_from_hash(h, np.float32), S.uniform_from_hash(h, np.float64)
    assert u32.dtype == np.float32 and u64.dtype == np.float64
    assert np.array_equal(u32.astype(np.float64), u64)  # exactly representable in fp32
    assert (u32 > 0).all() and (u32 < 1).all()
    assert u64.min() == 2.0 ** -24 and u64.max() == 1 - 2.0 ** -24
    g = -np.log(-np.log(u32))
    assert np.isfinite(g).all()


def test_hash_separates_its_arguments():
    from vq3d import sample as S
    k = np.arange(256).reshape(1, 256)
    base = S.gumbel_hash(7, [[0]], 5, k)
    assert base.dtype == np.uint32 and len(np.unique(base)) == 256  # a row's hashes are distinct
    for other in (S.gumbel_hash(8, [[0]], 5, k), S.gumbel_hash(7, [[1]], 5, k), S.gumbel_hash(7, [[0]], 6, k),
                  S.gumbel_hash(7 + 2 ** 32, [[0]], 5, k), S.gumbel_hash(7, [[2 ** 32]], 5, k)):
        assert (other != base).mean() > 0.99
    assert np.array_equal(S.gumbel_hash(7, [[0], [1]], 5, k)[1:], S.gumbel_hash(7, [[1]], 5, k))
    assert np.array_equal(S.gumbel_hash(-1, [[0]], 5, k), S.gumbel_hash(2 ** 64 - 1, [[0]], 5, k))


def _tiny_prior(k=8, model_dim=32):
    from vq3d import pixelsnail as PS
    torch.manual_seed(0)
    args = PS.default_args(num_embeddings=[k, 0], model_dim=model_dim, num_blocks=1, num_layers_per_block=1)
    return PS.PixelSNAIL(args, compute_dtype="fp32").eval()


class FakeHidden:
    """hidden_fn of the driver: a fixed random field plus a term that depends on the prefix it is
    given; records every call"""

    def __init__(self, b, c, size):
        g = torch.Generator().manual_seed(3)
        self.field = torch.randn((b, c) + tuple(size), generator=g)
        self.calls = []

    def __call__(self, prefix, full_dims):
        self.calls.append((prefix.clone(), tuple(full_dims)))
        s1 = prefix.shape[2]
        mix = prefix.float().mean(dim=1, keepdim=True).cumsum(2).cumsum(3).cumsum(4)
        return (self.field[:, :, :s1] + 0.5 * torch.sin(7.0 * mix)).contiguous(memory_format=CL)


def _run(model, size, b, **kw):
    from vq3d.sample import sample_codes
    fake = FakeHidden(b, 32, size)
    out = sample_codes(model, size, batch_size=b, hidden_fn=fake, **kw)
    return out, fake


@pytest.mark.parametrize("size", [(3, 2, 4), (1, 1, 5)])
def test_driver_visits_positions_in_raster_order(size):
    from vq3d import sample as S
    model, b, k = _tiny_prior(), 2, 8
    d, h, w = size
    npos, hw = d * h * w, h * w
    (codes, logits), fake = _run(model, size, b, seed=11, sample_base=4, return_logits=True)
    assert codes.shape == (b,) + size and codes.dtype == torch.int64
    assert logits.shape == (b, k) + size and logits.dtype == torch.float32
    assert int(codes.min()) >= 0 and int(codes.max()) < k
    assert len(fake.calls) == npos  # every position once
    final = torch.nn.functional.one_hot(codes, k).float().reshape(b, npos, k)
    weight, bias = model.parse_output.weight.detach(), model.parse_output.bias.detach()
    for p, (prefix, full_dims) in enumerate(fake.calls):
        assert full_dims == size
        assert prefix.shape == (b, k, p // hw + 1, h, w)  # the slab prefix holding p
        rows = prefix.permute(0, 2, 3, 4, 1).reshape(b, -1, k)
        # what was drawn before p is in place and is never rewritten; p and everything after it is empty
        assert torch.equal(rows[:, :p], final[:, :p])
        assert not rows[:, p:].any()
        # position p's draw: the head on the fake's row p, then the restatement's draw
        hid = fake.field[:, :, :p // hw + 1] + 0.5 * torch.sin(
            7.0 * prefix.float().mean(dim=1, keepdim=True).cumsum(2).cumsum(3).cumsum(4))
        lg = S.head_logits(hid.permute(0, 2, 3, 4, 1).reshape(b, -1, 32)[:, p], weight, bias)
        assert torch.equal(lg, logits.reshape(b, k, npos)[:, :, p])
        assert np.array_equal(S.draw_codes(lg.numpy(), 1.0, 11, 4, p), codes.reshape(b, npos)[:, p].numpy())


def test_driver_seeds_and_sample_base():
    model, size = _tiny_prior(), (2, 3, 3)
    a, _ = _run(model, size, 2, seed=5)
    again, _ = _run(model, size, 2, seed=5)
    other_seed, _ = _run(model, size, 2, seed=6)
    other_base, _ = _run(model, size, 2, seed=5, sample_base=2)
    assert torch.equal(a, again)
    assert not torch.equal(a, other_seed) and not torch.equal(a, other_base)
    cold, _ = _run(model, size, 2, seed=5, temperature=0.0)
    cold2, _ = _run(model, size, 2, seed=9, temperature=0.0)
    assert torch.equal(cold, cold2)  # the argmax ignores the seed


def test_driver_refuses_a_training_model_and_bad_arguments():
    from vq3d.sample import sample_codes
    model = _tiny_prior()
    with pytest.raises(RuntimeError, match="eval"):
        sample_codes(model.train(), (1, 2, 2), hidden_fn=FakeHidden(1, 32, (1, 2, 2)))
    model.eval()
    with pytest.raises(ValueError):
        sample_codes(model, (1, 2, 2), temperature=-1.0, hidden_fn=FakeHidden(1, 32, (1, 2, 2)))
    with pytest.raises(ValueError):
        sample_codes(model, (0, 2, 2), hidden_fn=FakeHidden(1, 32, (1, 2, 2)))
    with pytest.raises(ValueError, match="GPU"):
        sample_codes(model, (1, 2, 2), graphs=True, hidden_fn=FakeHidden(1, 32, (1, 2, 2)))


@pytest.mark.parametrize("dims", [(4, 4, 4), (3, 5, 7)])
def test_background_crop_is_a_slice_of_the_full_background(dims):
    from vq3d.pixelsnail import background_list
    full = background_list(2, dims, torch.float32, "cpu")
    assert all(torch.equal(f, full[0]) for f in full)
    same = background_list(2, dims, torch.float32, "cpu", full_dims=dims)
    assert torch.equal(same[0], full[0])
    for s1 in range(1, dims[0] + 1):
        crop = background_list(2, (s1,) + dims[1:], torch.float32, "cpu", full_dims=dims)
        assert len(crop) == 3 and crop[0].is_contiguous(memory_format=CL)
        assert torch.equal(crop[0], full[0][:, :, :s1])
    if dims[0] > 2:  # not a fresh linspace over the crop
        fresh = background_list(2, (2,) + dims[1:], torch.float32, "cpu")
        assert not torch.equal(fresh[0], full[0][:, :, :2])
    with pytest.raises(ValueError):
        background_list(1, (dims[0] + 1,) + dims[1:], torch.float32, "cpu", full_dims=dims)
    with pytest.raises(ValueError):
        background_list(1, (1, dims[1] + 1, dims[2]), torch.float32, "cpu", full_dims=dims)


def test_entry_refuses_unsupported_sizes_before_any_launch():
    from vq3d import _lib as L
    lib = L.load()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails its host-side checks

    def call(k=8, c=32, hd=L.F32, od=L.F32, temperature=1.0, batch=1, hidden=one):
        return lib.vq3d_prior_sample_step(hd, hidden, 64, c, one, one, k, one, temperature, one, 0, od, one, one, 64,
                                          batch, None, None)
    for kw, word in ((dict(k=7), b"k"), (dict(k=1025), b"k"), (dict(c=12), b"multiple of 8"), (dict(c=1032), b"1024"),
                     (dict(c=0), b"multiple of 8"), (dict(hd=L.BF16, od=L.F16), b"16-bit"), (dict(hd=3), b"fp32"),
                     (dict(temperature=-0.5), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
                     (dict(batch=0), b"sizes"), (dict(hidden=None), b"null")):
        assert call(**kw) < 0, kw
        assert word in lib.vq3d_last_error(), (kw, lib.vq3d_last_error())


def test_operator_is_registered_with_a_fake():
    import vq3d.library as Lb
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "prior_sample_step" in Lb.OPS
    schema = str(torch.ops.vq3d.prior_sample_step.default._schema)
    assert "Tensor(a7!) onehot" in schema and "Tensor(a8!) codes" in schema and "-> ()" in schema
    with FakeTensorMode():
        dev = "cuda"
        hid = torch.empty((2, 32, 1, 4, 4), device=dev).contiguous(memory_format=CL)
        x = torch.empty((2, 8, 4, 4, 4), device=dev).contiguous(memory_format=CL)
        out = torch.ops.vq3d.prior_sample_step(
            hid, torch.empty((8, 32), device=dev), torch.empty(8, device=dev),
            torch.empty((), dtype=torch.int64, device=dev), 1.0, torch.empty((), dtype=torch.int64, device=dev), 0, x,
            torch.empty((2, 64), dtype=torch.int64, device=dev), None)
        assert out is None


def test_sample_codes_is_exported():
    import vq3d
    from vq3d.sample import sample_codes
    assert vq3d.sample_codes is sample_codes and "sample_codes" in vq3d.__all__
