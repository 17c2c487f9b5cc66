"""QK-norm (``--qk-norm rms``) on the CPU: the definition ``qknorm_torch`` (ops/qknorm.py) in fp64
against the NumPy mirror of tests/qknorm_ref.py, its gradients, the edge cases g == 0 and x == 0, the
model against the fp64 oracle, the CLI, the leaves and the checkpoint rules."""

import numpy as np
import pytest
import torch

from qknorm_ref import qknorm_bwd_np, qknorm_np

from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params, load_pretrained_params, save_params, writer
from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.models import oracle
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import functional as Fn
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.ops import qknorm as QN
from jumbo_mae_tpu_amd.ops.qknorm import qknorm_bwd_torch, qknorm_torch
from jumbo_mae_tpu_amd.ops.rope import Rope

THETA = 100.0


def _exact_table(G, hd, theta=THETA):  # as tests/test_rope.py: fp64, unrounded
    n = hd // 4
    ang = torch.arange(G, dtype=torch.float64)[:, None] * theta ** (-torch.arange(n, dtype=torch.float64) / n)[None]
    return torch.stack([ang.cos(), ang.sin()], -1)


def _inputs(B, S, H, hd, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3 * H * hd, generator=g, dtype=torch.float64) * 2
    gq = 1 + 0.5 * torch.randn(hd, generator=g, dtype=torch.float64)
    gk = 1 + 0.5 * torch.randn(hd, generator=g, dtype=torch.float64)
    return x, gq, gk


def _rope(kind, B, n_cls, Sp, hd, gw=3, G=4, seed=1):
    """(the op's Rope, the mirror's tuple) or (None, None)."""
    if kind is None:
        return None, None
    g = torch.Generator().manual_seed(seed)
    if kind == "order":
        pos = None
    elif kind == "shared":
        pos = torch.randperm(gw * gw, generator=g)[:Sp].to(torch.int32)
    else:
        pos = torch.stack([torch.randperm(gw * gw, generator=g)[:Sp] for _ in range(B)]).to(torch.int32)
    return (Rope(n_cls, gw, _exact_table(G, hd), pos),
            (n_cls, gw, THETA, None if pos is None else pos.numpy(), None))


CASES = [(8, 3, None), (16, 0, "shared"), (12, 3, "per-sample"), (32, 1, "order")]  # hd, n_cls, rope


@pytest.mark.parametrize("hd,n_cls,kind", CASES)
def test_qknorm_torch_matches_numpy_mirror(hd, n_cls, kind):
    B, H, Sp = 2, 3, 5
    x, gq, gk = _inputs(B, n_cls + Sp, H, hd)
    rope, rref = _rope(kind, B, n_cls, Sp, hd)
    got = qknorm_torch(x, H, gq, gk, rope)
    ref, _ = qknorm_np(x.numpy(), H, gq.numpy(), gk.numpy(), rref)
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-13)
    v5, g5 = x.view(B, -1, 3, H, hd), got.view(B, -1, 3, H, hd)
    assert torch.equal(v5[:, :, 2], g5[:, :, 2])  # v bit for bit
    # the written-out backward (what prims.qknorm_bwd_ runs on the CPU) against the mirror's
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    saved = v5[:, :, :2].reshape(B, n_cls + Sp, -1)
    dx, dg = qknorm_bwd_torch(w, saved, H, gq, gk, rope)
    rdx, rdq, rdk = qknorm_bwd_np(w.numpy(), x.numpy(), H, gq.numpy(), gk.numpy(), rref)
    np.testing.assert_allclose(dx.numpy(), rdx.reshape(B, -1, 3, H, hd)[:, :, :2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dg[0].numpy(), rdq, rtol=0, atol=1e-11)
    np.testing.assert_allclose(dg[1].numpy(), rdk, rtol=0, atol=1e-11)


def test_every_row_has_unit_rms_before_the_scale():
    B, S, H, hd = 2, 4, 2, 8
    x, _, _ = _inputs(B, S, H, hd)
    one = torch.ones(hd, dtype=torch.float64)
    y = qknorm_torch(x, H, one, one).view(B, S, 3, H, hd)[:, :, :2]
    assert (y.square().mean(-1) - 1).abs().max().item() < 1e-5  # (eps 1e-6 against mean(x^2) ~ 4)
    assert P.LN_EPS == QN.EPS == 1e-6


@pytest.mark.parametrize("kind", [None, "per-sample"])
def test_gradcheck(kind):
    B, H, hd, n_cls, Sp = 2, 2, 8, 1, 3
    x, gq, gk = _inputs(B, n_cls + Sp, H, hd, seed=3)
    rope, _ = _rope(kind, B, n_cls, Sp, hd)
    args = [t.requires_grad_(True) for t in (x, gq, gk)]
    assert torch.autograd.gradcheck(lambda a, b, c: qknorm_torch(a, H, b, c, rope), args, eps=1e-6, atol=1e-7)
    # and the written-out backward is that gradient
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    gx, ggq, ggk = torch.autograd.grad((qknorm_torch(x, H, gq, gk, rope) * w).sum(), args)
    saved = x.detach().view(B, -1, 3, H, hd)[:, :, :2].reshape(B, n_cls + Sp, -1)
    dx, dg = qknorm_bwd_torch(w, saved, H, gq.detach(), gk.detach(), rope)
    assert (dx - gx.view(B, -1, 3, H, hd)[:, :, :2]).abs().max().item() < 1e-13
    assert (dg[0] - ggq).abs().max().item() < 1e-12 and (dg[1] - ggk).abs().max().item() < 1e-12
    assert torch.equal(gx.view(B, -1, 3, H, hd)[:, :, 2], w.view(B, -1, 3, H, hd)[:, :, 2])  # v passes through


def test_zero_scale_and_zero_row():
    B, S, H, hd = 2, 3, 2, 8
    x, gq, gk = _inputs(B, S, H, hd, seed=4)
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    saved = x.view(B, S, 3, H, hd)[:, :, :2].reshape(B, S, -1)
    # g_q == 0: q is 0, no gradient reaches x through q, dg_q is finite and is what the mirror says
    zero = torch.zeros(hd, dtype=torch.float64)
    y = qknorm_torch(x, H, zero, gk).view(B, S, 3, H, hd)
    assert (y[:, :, 0] == 0).all() and (y[:, :, 1] != 0).any()
    dx, dg = qknorm_bwd_torch(w, saved, H, zero, gk)
    assert (dx[:, :, 0] == 0).all() and torch.isfinite(dg).all()
    _, rdq, _ = qknorm_bwd_np(w.numpy(), x.numpy(), H, zero.numpy(), gk.numpy())
    np.testing.assert_allclose(dg[0].numpy(), rdq, rtol=0, atol=1e-12)
    assert np.abs(rdq).max() > 0.1
    # an all-zero q row: y == 0 there, and every gradient is finite (r = 1 / sqrt(eps))
    x0 = x.clone()
    x0.view(B, S, 3, H, hd)[1, 2, 0, 1] = 0
    xr = x0.clone().requires_grad_(True)
    gqr, gkr = gq.clone().requires_grad_(True), gk.clone().requires_grad_(True)
    y0 = qknorm_torch(xr, H, gqr, gkr)
    assert (y0.view(B, S, 3, H, hd)[1, 2, 0, 1] == 0).all()
    (y0 * w).sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in (xr, gqr, gkr))
    row = xr.grad.view(B, S, 3, H, hd)[1, 2, 0, 1]
    want = w.view(B, S, 3, H, hd)[1, 2, 0, 1] * gq / np.sqrt(QN.EPS)
    assert (row - want).abs().max().item() < 1e-9 * want.abs().max().item()


def test_in_place_primitives_and_autograd_wrapper_on_cpu():
    """prims.qknorm_fwd_ / qknorm_bwd_ (in place) and functional.qknorm (autograd, the scales' gradients
    added into the store) on the CPU path, against autograd of the composition."""
    m = _ft("rope", qk_norm="rms")
    attn = m.encoder.layers[0].attn
    H, hd = attn.heads, attn.dim // attn.heads
    with torch.no_grad():
        attn.q_norm.master.copy_(1 + 0.5 * torch.randn(hd))
        attn.k_norm.master.copy_(1 + 0.5 * torch.randn(hd))
    B, n_cls, Sp = 2, 3, 5
    x = torch.randn(B, n_cls + Sp, 3 * H * hd) * 2
    rope, _ = _rope("per-sample", B, n_cls, Sp, hd)
    rope = rope._replace(table=rope.table.float())
    gq, gk = attn.q_norm.master.clone(), attn.k_norm.master.clone()
    want = qknorm_torch(x, H, gq, gk, rope)
    y = x.clone()
    saved = P.qknorm_fwd_(y, H, gq, gk, rope)
    assert torch.equal(y, want)
    assert torch.equal(saved.view(B, -1, 2, H, hd), x.view(B, -1, 3, H, hd)[:, :, :2])
    assert saved.data_ptr() != y.data_ptr() and saved.is_contiguous()
    w = torch.randn_like(x)
    xa, ga, ka = (t.clone().requires_grad_(True) for t in (x, gq, gk))
    gx, ggq, ggk = torch.autograd.grad((qknorm_torch(xa, H, ga, ka, rope) * w).sum(), (xa, ga, ka))
    d = w.clone()
    d2, dg = P.qknorm_bwd_(d, saved, H, gq, gk, rope)
    assert d2 is d and torch.allclose(d, gx, atol=1e-5) and torch.allclose(dg[0], ggq, atol=1e-4)
    assert torch.equal(d.view(B, -1, 3, H, hd)[:, :, 2], w.view(B, -1, 3, H, hd)[:, :, 2])
    # the autograd wrapper leaves its input alone and accumulates the scales' gradients into the store
    m.store.zero_grad()
    xr = x.clone().requires_grad_(True)
    out = Fn.qknorm(xr, attn.q_norm, attn.k_norm, H, rope)
    assert torch.equal(out, want) and torch.equal(xr.detach(), x)
    (out * w).sum().backward()
    assert torch.allclose(xr.grad, gx, atol=1e-5)
    assert torch.allclose(attn.q_norm.grad, ggq, atol=1e-4) and torch.allclose(attn.k_norm.grad, ggk, atol=1e-4)


def test_cli_flags():
    from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
    for parser in (pretrain_parser, finetune_parser):
        assert parser().parse_args([]).qk_norm == "none"
        assert parser().parse_args(["--qk-norm", "rms"]).qk_norm == "rms"
        with pytest.raises(SystemExit):
            parser().parse_args(["--qk-norm", "layernorm"])
    assert pretrain_parser().parse_args([]).dec_qk_norm == "none"
    assert pretrain_parser().parse_args(["--dec-qk-norm", "rms"]).dec_qk_norm == "rms"
    with pytest.raises(SystemExit):  # the finetune model has no decoder
        finetune_parser().parse_args(["--dec-qk-norm", "rms"])
    with pytest.raises(ValueError, match="qk_norm"):
        _ft("learnable", qk_norm="layernorm")


# ------------------------------------------------------------------------------ the model
def _ft(posemb, image_size=32, **kw):
    return FinetuneModel(ViTConfig(layers=1, dim=32, heads=4, labels=10, image_size=image_size, patch_size=8,
                                   posemb=posemb, image_mask_ratio=None, **kw)).to("cpu")


def _pre(qk="none", dqk="none", seed=0, posemb="sincos2d", **kw):
    vc = ViTConfig(layers=2, dim=32, heads=4, labels=0, image_size=32, patch_size=8, posemb=posemb, qk_norm=qk, **kw)
    dc = DecoderConfig(dec_layers=1, dec_dim=16, dec_heads=2, image_size=32, patch_size=8, dec_qk_norm=dqk)
    return PretrainModel(vc, dc).to("cpu", seed=seed)


def test_leaves_shapes_init_and_no_weight_decay():
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer, layer_index
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    m = _pre("rms", "rms")
    names = [f"model/layer_{i}/attn/{n}_norm/scale" for i in (0, 1) for n in ("q", "k")] + \
            [f"decoder_model/dec_layer_0/attn/{n}_norm/scale" for n in ("q", "k")]
    new = [s for s in m.store.segments if s.path[-2:-1] in (("q_norm",), ("k_norm",))]
    assert sorted(s.key for s in new) == sorted(names)
    for s in new:
        hd = 8
        assert s.shape == (hd,) and s.flax_shape == (hd,) and s.trainable and not s.is_kernel
        assert torch.equal(m.store.master[s.offset:s.offset + s.numel], torch.ones(hd))
    tree = m.flax_params()
    assert tree["model"]["layer_1"]["attn"]["q_norm"]["scale"].shape == (8,)
    assert tree["decoder_model"]["dec_layer_0"]["attn"]["k_norm"]["scale"].shape == (8,)
    # only the encoder / only the decoder
    assert not any("decoder" in s.key and "q_norm" in s.key for s in _pre("rms").store.segments)
    assert not any("layer_0/attn/q_norm" in s.key and s.key.startswith("model") for s in _pre(dqk="rms").store.segments)
    # LLRD: with their layer
    seg = m.store.by_key["model/layer_1/attn/q_norm/scale"]
    assert layer_index(seg.path, 2) == layer_index(m.store.by_key["model/layer_1/attn/wo/bias"].path, 2) == 2
    # the decay mask: a step with zero gradients and weight decay moves kernels, never the scales
    opt = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-2, 1e-2, 0, 10, 1e-2), weight_decay=0.5,
                        num_layers=2)
    before = m.store.master.clone()
    m.store.zero_grad()
    opt.step()
    k = m.store.by_key["model/layer_0/attn/wq/kernel"]
    assert not torch.equal(m.store.master[k.offset:k.offset + k.numel], before[k.offset:k.offset + k.numel])
    for s in new:
        assert torch.equal(m.store.master[s.offset:s.offset + s.numel], before[s.offset:s.offset + s.numel]), s.key


def test_flag_off_is_todays_model():
    """Without the option the leaf list, the parameter values and a forward are those of a model built
    before the option existed (ViTConfig / DecoderConfig defaults)."""
    vc = ViTConfig(layers=2, dim=32, heads=4, labels=0, image_size=32, patch_size=8, posemb="sincos2d")
    dc = DecoderConfig(dec_layers=1, dec_dim=16, dec_heads=2, image_size=32, patch_size=8)
    a = PretrainModel(vc, dc).to("cpu", seed=0)
    b = _pre("none", "none")
    assert [(s.key, s.offset, s.shape) for s in a.store.segments] == [(s.key, s.offset, s.shape) for s in b.store.segments]
    assert not any("q_norm" in s.key or "k_norm" in s.key for s in b.store.segments)
    assert torch.equal(a.store.master, b.store.master)
    imgs = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    noise = torch.rand(16, generator=torch.Generator().manual_seed(1))
    la, lb = a(imgs, noise=noise)["loss"], b(imgs, noise=noise)["loss"]
    assert torch.equal(la, lb)
    assert all(layer.attn.q_norm is None and layer.attn.k_norm is None for layer in b.encoder.layers + b.decoder.layers)


def _grads_match(store, tp, atol_scale=2e-4):  # as tests/test_model_oracle.py
    flat = oracle.flatten(tp)
    total = np.sqrt(sum(float((v.grad.numpy() ** 2).sum()) for v in flat.values() if v.grad is not None))
    for s in store.segments:
        g = s.to_flax(store.grad[s.offset:s.offset + s.numel].numpy().reshape(s.shape))
        r = flat[s.key].grad
        r = np.zeros_like(g) if r is None else r.numpy()
        err = np.abs(g - r).max()
        assert err <= atol_scale * total + 1e-4 * np.abs(r).max(), (s.key, err, np.abs(r).max())


@pytest.mark.parametrize("posemb,per_op,ckpt", [("rope", "0", False), ("rope", "1", False), ("sincos2d", "0", True),
                                                ("sincos2d", "1", True)])
def test_pretrain_step_matches_oracle(monkeypatch, posemb, per_op, ckpt):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    torch.manual_seed(0)
    vc = ViTConfig(layers=2, dim=32, heads=4, labels=0, image_size=32, patch_size=8, posemb=posemb, rope_theta=50.0,
                   layerscale=True, image_mask_ratio=0.75, grad_ckpt=ckpt, qk_norm="rms")
    dc = DecoderConfig(dec_layers=2, dec_dim=16, dec_heads=2, image_size=32, patch_size=8, dec_layerscale=True,
                       dec_qk_norm="rms", grad_ckpt=ckpt)
    m = PretrainModel(vc, dc, mask_mode="per-sample").to("cpu")
    m.store.master.add_(torch.randn_like(m.store.master) * 0.3)  # (the scales move off one as well)
    imgs = torch.randint(0, 256, (3, 3, 32, 32), dtype=torch.uint8)
    noise = torch.rand(3, 16)
    out = m(imgs, noise=noise)
    out["loss"].backward()
    tree = m.flax_params()
    tp = oracle.tree_to_torch(tree)
    kw = dict(layers=2, dim=32, heads=4, dec_layers=2, dec_dim=16, dec_heads=2, patch=8, mask_ratio=0.75)
    ref = oracle.mae_loss(tp, imgs, noise.double(), posemb=posemb, rope_theta=50.0, **kw)
    ref.backward()
    assert abs(out["loss"].item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    _grads_match(m.store, tp)
    g = oracle.flatten(tp)["model/layer_0/attn/q_norm/scale"].grad
    assert g is not None and g.abs().max().item() > 1e-6  # the scales are live
    # ... and so is the norm: the same weights without the scale leaves give another loss
    for name, sub in list(tree["model"].items()) + list(tree["decoder_model"].items()):
        if isinstance(sub, dict) and "attn" in sub:
            sub["attn"].pop("q_norm"), sub["attn"].pop("k_norm")
    with torch.no_grad():
        other = oracle.mae_loss(oracle.tree_to_torch(tree), imgs, noise.double(), posemb=posemb, rope_theta=50.0, **kw)
    assert abs(other.item() - ref.item()) > 1e-4


@pytest.mark.parametrize("per_op", ["0", "1"])
def test_finetune_step_matches_oracle(monkeypatch, per_op):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    torch.manual_seed(1)
    vc = ViTConfig(layers=2, dim=32, heads=2, labels=5, image_size=24, patch_size=8, posemb="rope",
                   image_mask_ratio=None, layerscale=True, qk_norm="rms")
    m = FinetuneModel(vc, label_smoothing=0.1).to("cpu")
    m.store.master.add_(torch.randn_like(m.store.master) * 0.05)
    imgs = torch.randint(0, 256, (4, 3, 24, 24), dtype=torch.uint8)
    labels = torch.tensor([0, 3, 1, 4])
    out = m(imgs, labels, rngs={}, det=False)
    out["loss"].backward()
    tp = oracle.tree_to_torch(m.flax_params())
    lg = oracle.classifier_logits(tp, oracle.normalize_nhwc(imgs), layers=2, dim=32, heads=2, patch=8, posemb="rope")
    onehot = torch.nn.functional.one_hot(labels, 5).double() * 0.9 + 0.1 / 5
    ref = -(onehot * torch.log_softmax(lg, -1)).sum(-1).mean()
    ref.backward()
    assert abs(out["loss"].item() - ref.item()) < 1e-5
    _grads_match(m.store, tp)


# ------------------------------------------------------------------------------ checkpoints
def _save(tmp_path, name, model):
    url = save_params(str(tmp_path), name, model.flax_params(), "last")
    writer().flush()
    return url


def test_msgpack_round_trip_and_mismatched_loads(tmp_path):
    quiet = lambda *a: None  # noqa: E731
    qk = _pre("rms", "rms", seed=3)
    with torch.no_grad():
        qk.store.master.add_(torch.randn_like(qk.store.master) * 0.1)
    url_qk = _save(tmp_path, "qk", qk)
    url_plain = _save(tmp_path, "plain", _pre(seed=4))
    url_dec = _save(tmp_path, "dec", _pre("none", "rms", seed=5))
    # round trip, bit for bit, the scales included
    back = _pre("rms", "rms")
    back.load_flax_params(load_params(url_qk))
    for seg in qk.store.segments:  # (the perturbation above also fell into the alignment padding: compare the leaves)
        sl = slice(seg.offset, seg.offset + seg.numel)
        assert torch.equal(back.store.master[sl], qk.store.master[sl]), seg.key
    s = qk.store.by_key["model/layer_0/attn/q_norm/scale"]
    assert not torch.equal(back.store.master[s.offset:s.offset + s.numel], torch.ones(8))
    # --pretrained-ckpt: a checkpoint without QK-norm is refused by a QK-norm finetune model (never ones) ...
    with pytest.raises(ValueError, match="--qk-norm"):
        load_pretrained_params(url_plain, _ft("sincos2d", qk_norm="rms").flax_params(), quiet)
    # ... and a checkpoint with it by a model without
    with pytest.raises(ValueError, match="--qk-norm"):
        load_pretrained_params(url_qk, _ft("sincos2d").flax_params(), quiet)
    # the decoder's choice does not matter to a finetune model, which has no decoder
    load_pretrained_params(url_dec, _ft("sincos2d").flax_params(), quiet)
    ft = _ft("sincos2d", qk_norm="rms")
    tree = load_pretrained_params(url_qk, ft.flax_params(), quiet)
    ft.store.load_flax_tree(tree, strict=True)
    a = ft.store.by_key["model/layer_0/attn/k_norm/scale"]
    b = qk.store.by_key["model/layer_0/attn/k_norm/scale"]
    assert torch.equal(ft.store.master[a.offset:a.offset + a.numel], qk.store.master[b.offset:b.offset + b.numel])
    # the strict loads (--resume, --teacher-ckpt, tools) name the flag both ways, for either stack
    with pytest.raises(KeyError, match="--qk-norm"):
        _pre("rms", "rms").load_flax_params(load_params(url_plain))
    with pytest.raises(KeyError, match="--qk-norm"):
        _pre().load_flax_params(load_params(url_qk))
    with pytest.raises(KeyError, match="--dec-qk-norm"):
        _pre().load_flax_params(load_params(url_dec))
    with pytest.raises(KeyError, match="--qk-norm"):
        _pre("rms", "none").load_flax_params(load_params(url_dec))


def test_timm_converter_round_trip_both_directions():
    from jumbo_mae_tpu_amd.ckpt.convert import flax_to_torch, torch_to_flax
    from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
    m = _ft("learnable", qk_norm="rms")
    with torch.no_grad():
        m.store.master.add_(torch.randn_like(m.store.master) * 0.1)
    tree = m.flax_params()
    sd = flax_to_torch(tree)
    want = tree["model"]["layer_0"]["attn"]
    assert np.array_equal(sd["blocks.0.attn.q_norm.weight"], want["q_norm"]["scale"])
    assert np.array_equal(sd["blocks.0.attn.k_norm.weight"], want["k_norm"]["scale"])
    assert not any(k.endswith("_norm.bias") and ".attn." in k for k in sd)
    back = torch_to_flax(sd, num_heads=4)
    a, b = flatten_tree(tree), flatten_tree(back)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], atol=1e-6, err_msg=str(k))
    # torch -> flax -> torch
    sd2 = flax_to_torch(back)
    assert set(sd2) == set(sd) and all(np.allclose(sd[k], sd2[k], atol=1e-6) for k in sd)
    # a tree without the leaves converts without them, and a biased (LayerNorm) QK-norm is refused
    plain = flax_to_torch(_ft("learnable").flax_params())
    assert not any("q_norm" in k or "k_norm" in k for k in plain)
    with pytest.raises(ValueError, match="scale only"):
        torch_to_flax({**sd, "blocks.0.attn.q_norm.bias": np.zeros(8, np.float32)}, num_heads=4)
