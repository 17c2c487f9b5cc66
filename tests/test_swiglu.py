"""The gated feed-forward (``--ffn swiglu``) on the CPU: the mirror of csrc/swiglu.hip against autograd, the
model against the fp64 oracle (models/oracle.py) at the thresholds of tests/test_model_oracle.py, the new
leaves, the untouched GELU path, the flags, checkpoints, the FLOP count and the hidden width."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swiglu_ref as R
from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params, load_pretrained_params, save_params, writer
from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig, decoder_config, ffn_hidden, vit_config
from jumbo_mae_tpu_amd.models import oracle
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import functional as Fn
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.ops.swiglu import drop_factors, swiglu_bwd_torch, swiglu_torch


# ------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("masked", [False, True])
def test_mirror_matches_fp64_autograd(masked):
    g = torch.Generator().manual_seed(0)
    pre = (4.0 * torch.randn(7, 2 * 24, generator=g, dtype=torch.float64))
    pre[:, :8] = torch.tensor(R.SPECIAL, dtype=torch.float64)
    da = torch.randn(7, 24, generator=g, dtype=torch.float64)
    mask = None
    if masked:
        mask = drop_factors(torch.tensor([77]), 7, 24, 0.25, dtype=torch.float64)
        assert 0 < int((mask == 0).sum()) < mask.numel()
    x = pre.clone().requires_grad_(True)
    want = F.silu(x[:, :24]) * x[:, 24:]
    if masked:
        want = want * mask
    (gx,) = torch.autograd.grad((want * da).sum(), x)
    got = swiglu_torch(pre, mask)
    assert got.dtype == torch.float64 and (got - want.detach()).abs().max().item() <= 1e-12
    assert (swiglu_bwd_torch(pre, da, mask) - gx).abs().max().item() <= 1e-12
    # every dtype: fp32 in, fp32 out
    assert swiglu_torch(pre.float()).dtype == torch.float32
    # saturation: no NaN where exp leaves the range
    big = torch.tensor([[-800.0, 800.0, 1.0, 1.0]], dtype=torch.float64)
    assert torch.isfinite(swiglu_torch(big)).all() and torch.isfinite(swiglu_bwd_torch(big, torch.ones(1, 2).double())).all()


def test_prims_and_autograd_wrapper_on_cpu():
    """``P.swiglu_fwd`` / ``P.swiglu_bwd`` take the mirror on the CPU, with the generator's mask; ``Fn.swiglu``
    differentiates through them."""
    pre, da = R.inputs(5, 128, seed=1)
    pre, da = pre.float(), da.float()
    seed = torch.tensor([5])
    mask = drop_factors(seed, 5, 128, 0.25)
    assert torch.equal(P.swiglu_fwd(pre), swiglu_torch(pre))
    assert torch.equal(P.swiglu_fwd(pre, (seed, 0.25)), swiglu_torch(pre, mask))
    dpre, done = P.swiglu_bwd(pre, da, None, (seed, 0.25))
    assert not done and torch.equal(dpre, swiglu_bwd_torch(pre, da, mask))
    x = pre.clone().requires_grad_(True)
    out = Fn.swiglu(x.view(1, 5, 256), (seed, 0.25))
    assert out.shape == (1, 5, 128)
    (out * da.view(1, 5, 128)).sum().backward()
    assert torch.equal(x.grad, dpre)


# ------------------------------------------------------------------------------ the model
def _pre(ffn="swiglu", dec_ffn="swiglu", seed=0, **kw):
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75, ffn=ffn, **kw)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16, dec_ffn=dec_ffn)
    return PretrainModel(vc, dc, mask_mode="per-sample").to("cpu", seed=seed)


def _ft(ffn="swiglu", **kw):
    return FinetuneModel(ViTConfig(layers=1, dim=32, heads=4, labels=10, image_size=32, patch_size=8,
                                   posemb="sincos2d", image_mask_ratio=None, ffn=ffn, **kw)).to("cpu")


def _grads_match(store, tp, atol_scale=2e-4):  # as tests/test_model_oracle.py
    flat = oracle.flatten(tp)
    total = np.sqrt(sum(float((v.grad.numpy() ** 2).sum()) for v in flat.values() if v.grad is not None))
    for s in store.segments:
        g = s.to_flax(store.grad[s.offset:s.offset + s.numel].numpy().reshape(s.shape))
        r = flat[s.key].grad
        r = np.zeros_like(g) if r is None else r.numpy()
        err = np.abs(g - r).max()
        assert err <= atol_scale * total + 1e-4 * np.abs(r).max(), (s.key, err, np.abs(r).max())


@pytest.mark.parametrize("per_op", ["0", "1"])
def test_pretrain_step_matches_oracle(monkeypatch, per_op):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    torch.manual_seed(0)
    m = _pre()
    m.store.master.add_(torch.randn_like(m.store.master) * 0.05)
    imgs = torch.randint(0, 256, (3, 3, 64, 64), dtype=torch.uint8)
    noise = torch.rand(3, 16)
    out = m(imgs, noise=noise)
    out["loss"].backward()
    tree = m.flax_params()
    tp = oracle.tree_to_torch(tree)
    kw = dict(layers=2, dim=128, heads=2, dec_layers=2, dec_dim=64, dec_heads=2, patch=16, mask_ratio=0.75)
    ref = oracle.mae_loss(tp, imgs, noise.double(), posemb="sincos2d", **kw)
    ref.backward()
    assert abs(out["loss"].item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    _grads_match(m.store, tp)
    flat = oracle.flatten(tp)
    for key in ("model/layer_0/ff/w3/kernel", "model/jumbo_mlp/w3/bias", "decoder_model/dec_layer_1/ff/w3/kernel"):
        assert flat[key].grad is not None and flat[key].grad.abs().max().item() > 1e-7, key  # the up branch is live


def test_leaves_widths_and_name_rules():
    from jumbo_mae_tpu_amd.optim.flat import layer_index
    m = _pre()
    by = m.store.by_key
    # dim 128 -> Hs 384; the jumbo MLP over 3 * 128 channels -> ceil((8 * 384 / 3) / 128) * 128 = 1024; the decoder 64 -> 256
    for node, din, hs in (("model/layer_0/ff", 128, 384), ("model/layer_1/ff", 128, 384), ("model/jumbo_mlp", 384, 1024),
                          ("decoder_model/dec_layer_0/ff", 64, 256), ("decoder_model/dec_layer_1/ff", 64, 256)):
        for w in ("w1", "w3"):
            k, b = by[f"{node}/{w}/kernel"], by[f"{node}/{w}/bias"]
            assert k.shape == (hs, din) and k.flax_shape == (din, hs) and k.is_kernel and k.trainable
            assert b.shape == (hs,) and not b.is_kernel
        assert by[f"{node}/w2/kernel"].shape == (din, hs)
        # w1 | w3 are adjacent: one [2 Hs, dim] handle
        assert by[f"{node}/w3/kernel"].offset == by[f"{node}/w1/kernel"].offset + hs * din
        assert by[f"{node}/w3/bias"].offset == by[f"{node}/w1/bias"].offset + hs
    ff = m.encoder.layers[0].ff
    assert ff.kind == "swiglu" and ff.w13.k.shape == (768, 128) and ff.w13.b.shape == (768,) and len(ff.w13.k.segs) == 2
    assert m.encoder.jumbo_mlp.kind == "swiglu" and m.encoder.jumbo_mlp.w13.k.defer_wgrad
    # init as the other Dense leaves: truncated normal kernels, zero biases
    k3 = by["model/layer_0/ff/w3/kernel"]
    v = m.store.master[k3.offset:k3.offset + k3.numel]
    assert 0.015 < v.std().item() < 0.025 and v.abs().max().item() <= 0.02 * 2 / 0.8796 + 1e-6
    b3 = by["model/layer_0/ff/w3/bias"]
    assert not m.store.master[b3.offset:b3.offset + b3.numel].any()
    # layer-wise lr decay: with their layer
    assert layer_index(k3.path, 2) == layer_index(by["model/layer_0/ff/w2/kernel"].path, 2)
    # one stack only
    assert not any("w3" in s.path for s in _pre("gelu", "swiglu").store.segments if s.path[0] == "model")
    assert not any("w3" in s.path for s in _pre("swiglu", "gelu").store.segments if s.path[0] == "decoder_model")
    with pytest.raises(ValueError, match="ffn"):
        _ft("geglu")


def test_off_path_is_todays_model():
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16)
    a = PretrainModel(vc, dc, mask_mode="per-sample").to("cpu", seed=0)
    b = _pre("gelu", "gelu")
    assert [(s.key, s.offset, s.shape) for s in a.store.segments] == [(s.key, s.offset, s.shape) for s in b.store.segments]
    assert not any("w3" in s.path for s in b.store.segments)
    assert torch.equal(a.store.master, b.store.master)
    assert vc.hidden_dim == 512 and vc.jumbo_hidden_dim == 4 * 384 and dc.hidden_dim == 256
    assert all(layer.ff.kind == "gelu" for layer in b.encoder.layers + b.decoder.layers)


def test_cli_flags():
    from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
    for parser in (pretrain_parser, finetune_parser):
        assert parser().parse_args([]).ffn == "gelu"
        assert parser().parse_args(["--ffn", "swiglu"]).ffn == "swiglu"
        with pytest.raises(SystemExit):
            parser().parse_args(["--ffn", "geglu"])
    assert pretrain_parser().parse_args([]).dec_ffn == "gelu"
    assert pretrain_parser().parse_args(["--dec-ffn", "swiglu"]).dec_ffn == "swiglu"
    with pytest.raises(SystemExit):
        pretrain_parser().parse_args(["--dec-ffn", "relu"])
    with pytest.raises(SystemExit):  # the finetune model has no decoder
        finetune_parser().parse_args(["--dec-ffn", "swiglu"])
    assert finetune_parser().parse_args([]).teacher_ffn is None  # the student's kind
    assert finetune_parser().parse_args(["--teacher-ffn", "swiglu"]).teacher_ffn == "swiglu"
    with pytest.raises(SystemExit):
        finetune_parser().parse_args(["--teacher-ffn", "x"])
    assert "same --ffn" in " ".join(pretrain_parser().format_help().split())


def test_drivers_build_the_flagged_model():
    from jumbo_mae_tpu_amd.train import finetune as FT
    from jumbo_mae_tpu_amd.train import pretrain as PT
    from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
    small = ["--layers", "1", "--dim", "32", "--heads", "2", "--image-size", "32", "--patch-size", "8"]
    args = pretrain_parser().parse_args(small + ["--ffn", "swiglu", "--dec-layers", "1", "--dec-dim", "16", "--dec-heads",
                                                 "2", "--dec-ffn", "swiglu"])
    m = PT.build_model(args, torch.device("cpu"), torch.float32)
    assert "model/jumbo_mlp/w3/kernel" in m.store.by_key and "decoder_model/dec_layer_0/ff/w3/bias" in m.store.by_key
    args = finetune_parser().parse_args(small + ["--labels", "5", "--ffn", "swiglu"])
    assert "model/layer_0/ff/w3/kernel" in FT.build_model(args, torch.device("cpu"), torch.float32).store.by_key


# ------------------------------------------------------------------------------ checkpoints
def _save(tmp_path, name, model):
    url = save_params(str(tmp_path), name, model.flax_params(), "last")
    writer().flush()
    return url


def test_checkpoint_round_trip_and_mismatched_loads(tmp_path):
    quiet = lambda *a: None  # noqa: E731
    sw = _pre(seed=3)
    with torch.no_grad():
        sw.store.master.add_(torch.randn_like(sw.store.master) * 0.1)
    # flax -> store -> flax keeps every leaf's bits
    tree = sw.flax_params()
    back = _pre()
    back.load_flax_params(tree)
    again = oracle.flatten(back.flax_params())
    first = oracle.flatten(tree)
    assert set(again) == set(first) and "model/jumbo_mlp/w3/kernel" in first
    for k in first:
        assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32)), k
    # ... through a file as well
    url_sw = _save(tmp_path, "sw", sw)
    url_ge = _save(tmp_path, "ge", _pre("gelu", "gelu", seed=4))
    url_dec = _save(tmp_path, "dec", _pre("gelu", "swiglu", seed=5))
    back = _pre()
    back.load_flax_params(load_params(url_sw))
    for seg in sw.store.segments:
        sl = slice(seg.offset, seg.offset + seg.numel)
        assert torch.equal(back.store.master[sl], sw.store.master[sl]), seg.key
    # a GELU checkpoint into a SwiGLU model: the named error, not w1/kernel's shape mismatch -- and the reverse
    with pytest.raises(ValueError, match=r"(?s)w3.*--ffn"):
        _pre().load_flax_params(load_params(url_ge))
    with pytest.raises(ValueError, match=r"(?s)w3.*--ffn"):
        _pre("gelu", "gelu").load_flax_params(load_params(url_sw))
    with pytest.raises(ValueError, match=r"(?s)decoder_model/dec_layer_0/ff/w3.*--dec-ffn"):
        _pre("gelu", "gelu").load_flax_params(load_params(url_dec))
    # --pretrained-ckpt both ways; the decoder's kind does not matter to a finetune model
    ft_sw = FinetuneModel(ViTConfig(layers=2, dim=128, heads=2, labels=10, image_size=64, patch_size=16,
                                    posemb="sincos2d", image_mask_ratio=None, ffn="swiglu")).to("cpu")
    ft_ge = FinetuneModel(ViTConfig(layers=2, dim=128, heads=2, labels=10, image_size=64, patch_size=16,
                                    posemb="sincos2d", image_mask_ratio=None)).to("cpu")
    with pytest.raises(ValueError, match=r"(?s)w3.*--ffn"):
        load_pretrained_params(url_ge, ft_sw.flax_params(), quiet)
    with pytest.raises(ValueError, match=r"(?s)w3.*--ffn"):
        load_pretrained_params(url_sw, ft_ge.flax_params(), quiet)
    load_pretrained_params(url_dec, ft_ge.flax_params(), quiet)
    ft_sw.store.load_flax_tree(load_pretrained_params(url_sw, ft_sw.flax_params(), quiet), strict=True)
    a, b = ft_sw.store.by_key["model/layer_1/ff/w3/kernel"], sw.store.by_key["model/layer_1/ff/w3/kernel"]
    assert torch.equal(ft_sw.store.master[a.offset:a.offset + a.numel], sw.store.master[b.offset:b.offset + b.numel])


def test_timm_converter_round_trip():
    from jumbo_mae_tpu_amd.ckpt.convert import flax_to_torch, torch_to_flax
    from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
    m = FinetuneModel(ViTConfig(layers=1, dim=32, heads=4, labels=10, image_size=32, patch_size=8, posemb="learnable",
                                image_mask_ratio=None, ffn="swiglu")).to("cpu")
    with torch.no_grad():
        m.store.master.add_(torch.randn_like(m.store.master) * 0.1)
    tree = m.flax_params()
    sd = flax_to_torch(tree)
    ff = tree["model"]["layer_0"]["ff"]
    assert np.array_equal(sd["blocks.0.mlp.fc1_g.weight"], ff["w1"]["kernel"].T)
    assert np.array_equal(sd["blocks.0.mlp.fc1_x.weight"], ff["w3"]["kernel"].T)
    assert np.array_equal(sd["jumbo_mlp.fc1_x.bias"], tree["model"]["jumbo_mlp"]["w3"]["bias"])
    assert "blocks.0.mlp.fc1.weight" not in sd
    a, b = flatten_tree(tree), flatten_tree(torch_to_flax(sd, num_heads=4))
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], atol=1e-6, err_msg=str(k))


# ------------------------------------------------------------------------------ FLOPs, width
def test_flops_hand_count():
    from jumbo_mae_tpu_amd.utils.flops import finetune_fwd_flops_per_image, pretrain_fwd_flops_per_image
    vc = vit_config("vit_base_patch16", labels=0, posemb="sincos2d", ffn="swiglu")
    dc = decoder_config(dec_ffn="swiglu")
    D, Hs, J, Hj, dd, Hd = 768, 2048, 2304, 6144, 512, 1408
    assert (vc.hidden_dim, vc.jumbo_hidden_dim, dc.hidden_dim) == (Hs, Hj, Hd)
    keep, n, c = 49, 196, 3
    t = c + keep
    enc_layer = 2 * t * D * 4 * D + 4 * t * t * D + 3 * 2 * keep * D * Hs + 3 * 2 * 1 * J * Hj
    enc = 12 * enc_layer + 2 * keep * 768 * D
    dec_layer = 2 * (c + n) * dd * 4 * dd + 4 * (c + n) ** 2 * dd + 3 * 2 * (c + n) * dd * Hd
    want = enc + 2 * t * D * dd + 8 * dec_layer + 2 * n * dd * 768
    assert pretrain_fwd_flops_per_image(vc, dc) == want
    # the GELU count is what it was: 2 * 2 * tokens * dim * 4 dim per feed-forward, the jumbo MLP's 4 c d included
    g = vit_config("vit_base_patch16", labels=1000, image_mask_ratio=None)
    t = c + n
    lay = 2 * t * D * 4 * D + 4 * t * t * D + 4 * n * D * 4 * D + 4 * J * 4 * J
    assert finetune_fwd_flops_per_image(g) == 12 * lay + 2 * n * 768 * D + 2 * c * D * 1000


def test_hidden_width():
    for dim, hs in ((192, 512), (768, 2048), (1024, 2816), (1280, 3456), (2304, 6144), (3072, 8192)):
        assert ffn_hidden(dim, "swiglu") == hs and hs % 128 == 0 and hs >= 8 * dim / 3 > hs - 128
        assert ffn_hidden(dim, "gelu") == 4 * dim
        assert ViTConfig(dim=dim, ffn="swiglu").hidden_dim == hs and ViTConfig(dim=dim).hidden_dim == 4 * dim
    assert ViTConfig(dim=768, ffn="swiglu").jumbo_hidden_dim == 6144
    assert DecoderConfig(dec_dim=512, dec_ffn="swiglu").hidden_dim == 1408
