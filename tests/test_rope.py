"""Axial 2-D rotary position embedding (``--posemb rope``) on the CPU: the definition ``rope_torch``
(ops/rope.py) in fp64 against the complex-number formulation of tests/rope_ref.py, its algebraic
properties, the model against the fp64 oracle, the CLI and the checkpoint rules."""

import numpy as np
import pytest
import torch

from rope_ref import rope_complex

from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params, load_pretrained_params, save_params, writer
from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.models import oracle
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.ops.rope import rope_table, rope_torch

THETA = 100.0


def _exact_table(G, hd, theta=THETA):
    """The (cos, sin) table in fp64, unrounded: ``rope_torch`` in fp64 takes any table dtype."""
    n = hd // 4
    ang = torch.arange(G, dtype=torch.float64)[:, None] * theta ** (-torch.arange(n, dtype=torch.float64) / n)[None]
    return torch.stack([ang.cos(), ang.sin()], -1)


def _qkv(B, S, H, hd, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, 3 * H * hd, generator=g, dtype=torch.float64)


CASES = [  # hd, n_cls, pos kind
    (8, 3, None), (16, 0, "shared"), (12, 3, "per-sample"), (32, 1, "shared"),
]


def _pos(kind, B, Sp, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    if kind is None:
        return None
    if kind == "shared":
        return torch.randperm(n, generator=g)[:Sp].to(torch.int32)
    return torch.stack([torch.randperm(n, generator=g)[:Sp] for _ in range(B)]).to(torch.int32)


@pytest.mark.parametrize("hd,n_cls,kind", CASES)
@pytest.mark.parametrize("inverse", [False, True])
def test_rope_torch_matches_complex_reference(hd, n_cls, kind, inverse):
    B, H, gw, G, Sp = 2, 3, 3, 4, 5
    x = _qkv(B, n_cls + Sp, H, hd)
    pos = _pos(kind, B, Sp, 9)
    got = rope_torch(x, H, n_cls, gw, _exact_table(G, hd), pos, inverse)
    ref = rope_complex(x.numpy(), H, n_cls, gw, THETA, None if pos is None else pos.numpy(), inverse)
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-13)
    # the fp32 table the model uses is the fp64 one rounded once
    tab = rope_table(G, hd, THETA)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (G, hd // 4, 2)
    assert torch.equal(tab, _exact_table(G, hd).float())
    assert rope_table(G, hd, THETA) is tab  # cached


def test_norm_preserved_and_inverse_undoes_forward():
    B, H, hd, n_cls, gw, G, Sp = 2, 3, 16, 3, 3, 4, 5
    x = _qkv(B, n_cls + Sp, H, hd)
    tab = _exact_table(G, hd)
    pos = _pos("per-sample", B, Sp, 9)
    y = rope_torch(x, H, n_cls, gw, tab, pos)
    px = x.view(B, -1, 3, H, hd // 2, 2).square().sum(-1)
    py = y.view(B, -1, 3, H, hd // 2, 2).square().sum(-1)
    assert ((py - px).abs() <= 1e-12 * px).all()
    back = rope_torch(y, H, n_cls, gw, tab, pos, inverse=True)
    assert (back - x).abs().max().item() <= 1e-12
    # CLS rows and v come back bit for bit, and q / k of the patch rows did change
    v5x, v5y = x.view(B, -1, 3, H, hd), y.view(B, -1, 3, H, hd)
    assert torch.equal(v5x[:, :n_cls], v5y[:, :n_cls]) and torch.equal(v5x[:, :, 2], v5y[:, :, 2])
    assert not torch.equal(v5x[:, n_cls:, :2], v5y[:, n_cls:, :2])


def test_scores_depend_on_relative_offsets_only():
    """q_i . k_j after the rotation is unchanged when every position moves by the same (dy, dx)."""
    B, H, hd, n_cls, gw, G, Sp = 2, 2, 16, 0, 7, 7, 6
    x = _qkv(B, Sp, H, hd, seed=3)
    tab = _exact_table(G, hd)
    g = torch.Generator().manual_seed(5)
    ys, xs = torch.randint(0, 4, (Sp,), generator=g), torch.randint(0, 4, (Sp,), generator=g)

    def scores(dy, dx):
        pos = ((ys + dy) * gw + (xs + dx)).to(torch.int32)
        r = rope_torch(x, H, n_cls, gw, tab, pos).view(B, Sp, 3, H, hd)
        return torch.einsum("bqhd,bkhd->bhqk", r[:, :, 0], r[:, :, 1])

    base = scores(0, 0)
    for dy, dx in ((3, 0), (0, 2), (2, 3)):
        assert (scores(dy, dx) - base).abs().max().item() <= 1e-10
    ident = torch.einsum("bqhd,bkhd->bhqk", *x.view(B, Sp, 3, H, hd)[:, :, :2].unbind(2))
    assert (base - ident).abs().max().item() > 1e-3  # and the rotation is not the identity


def test_shared_and_per_sample_positions_agree():
    B, H, hd, n_cls, gw, G, Sp = 3, 2, 8, 3, 3, 4, 5
    x = _qkv(B, n_cls + Sp, H, hd)
    tab = rope_table(G, hd)
    pos = _pos("shared", B, Sp, 9)
    a = rope_torch(x, H, n_cls, gw, tab, pos)
    b = rope_torch(x, H, n_cls, gw, tab, pos[None].expand(B, Sp).contiguous())
    assert torch.equal(a, b)
    # pos None is the identity list
    c = rope_torch(x, H, n_cls, gw, tab, None)
    d = rope_torch(x, H, n_cls, gw, tab, torch.arange(Sp, dtype=torch.int32))
    assert torch.equal(c, d)


def test_in_place_primitive_and_autograd_wrapper_on_cpu():
    """prims.rope_ (in place) and functional.rope (autograd, the transpose as the gradient) on the CPU path."""
    from jumbo_mae_tpu_amd.ops import functional as Fn
    from jumbo_mae_tpu_amd.ops.rope import Rope
    B, H, hd, n_cls, gw, G, Sp = 2, 2, 8, 3, 3, 4, 5
    x = _qkv(B, n_cls + Sp, H, hd).float()
    tab = rope_table(G, hd)
    pos = _pos("per-sample", B, Sp, 9)
    want = rope_torch(x, H, n_cls, gw, tab, pos)
    y = x.clone()
    assert P.rope_(y, H, n_cls, gw, tab, pos) is y and torch.equal(y, want)
    xr = x.clone().requires_grad_(True)
    out = Fn.rope(xr, H, Rope(n_cls, gw, tab, pos))
    assert torch.equal(out, want) and torch.equal(xr.detach(), x)  # the input is left alone
    w = torch.randn_like(x)
    (out * w).sum().backward()
    xa = x.clone().requires_grad_(True)
    (rope_torch(xa, H, n_cls, gw, tab, pos) * w).sum().backward()
    assert torch.allclose(xr.grad, xa.grad, atol=1e-6)
    assert torch.equal(xr.grad, rope_torch(w, H, n_cls, gw, tab, pos, inverse=True))


def test_head_dim_must_be_a_multiple_of_four():
    with pytest.raises(ValueError, match="multiple of 4"):
        rope_table(4, 6)
    with pytest.raises(ValueError, match="multiple of 4"):
        rope_torch(torch.zeros(1, 2, 3 * 2 * 6), 2, 0, 2, torch.zeros(4, 1, 2))
    with pytest.raises(ValueError, match="multiple of 4"):  # at model construction: dim 36 / 6 heads = 6
        PretrainModel(ViTConfig(layers=1, dim=36, heads=6, labels=0, image_size=32, patch_size=8, posemb="rope"),
                      DecoderConfig(dec_layers=1, dec_dim=16, dec_heads=2, image_size=32, patch_size=8))
    with pytest.raises(IndexError):  # a position outside the table
        rope_torch(torch.zeros(1, 1, 3 * 8), 1, 0, 2, rope_table(2, 8), torch.tensor([4], dtype=torch.int32))


def test_cli_flags():
    from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
    for parser, default in ((pretrain_parser, "sincos2d"), (finetune_parser, "learnable")):
        a = parser().parse_args(["--posemb", "rope", "--rope-theta", "50"])
        assert a.posemb == "rope" and a.rope_theta == 50.0
        d = parser().parse_args([])
        assert d.posemb == default and d.rope_theta == 100.0


# ------------------------------------------------------------------------------ model vs the fp64 oracle
def _grads_match(store, tp, atol_scale=2e-4):  # as tests/test_model_oracle.py
    flat = oracle.flatten(tp)
    total = np.sqrt(sum(float((v.grad.numpy() ** 2).sum()) for v in flat.values() if v.grad is not None))
    for s in store.segments:
        g = s.to_flax(store.grad[s.offset:s.offset + s.numel].numpy().reshape(s.shape))
        r = flat[s.key].grad
        r = np.zeros_like(g) if r is None else r.numpy()
        err = np.abs(g - r).max()
        assert err <= atol_scale * total + 1e-4 * np.abs(r).max(), (s.key, err, np.abs(r).max())


@pytest.mark.parametrize("mode,per_op,ckpt",
                         [("shared", "0", False), ("per-sample", "0", True), ("per-sample", "1", False)])
def test_pretrain_step_matches_oracle(monkeypatch, mode, per_op, ckpt):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    torch.manual_seed(0)
    vc = ViTConfig(layers=2, dim=32, heads=4, labels=0, image_size=32, patch_size=8, posemb="rope", rope_theta=50.0,
                   layerscale=True, image_mask_ratio=0.75, grad_ckpt=ckpt)
    dc = DecoderConfig(dec_layers=2, dec_dim=16, dec_heads=2, image_size=32, patch_size=8, dec_layerscale=True)
    m = PretrainModel(vc, dc, mask_mode=mode).to("cpu")
    m.store.master.add_(torch.randn_like(m.store.master) * 0.3)  # (large enough for peaked attention)
    imgs = torch.randint(0, 256, (3, 3, 32, 32), dtype=torch.uint8)
    noise = torch.rand(16) if mode == "shared" else torch.rand(3, 16)
    out = m(imgs, noise=noise)
    out["loss"].backward()
    tp = oracle.tree_to_torch(m.flax_params())
    kw = dict(layers=2, dim=32, heads=4, dec_layers=2, dec_dim=16, dec_heads=2, patch=8, mask_ratio=0.75)
    ref = oracle.mae_loss(tp, imgs, noise.double(), posemb="rope", rope_theta=50.0, **kw)
    ref.backward()
    assert abs(out["loss"].item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    _grads_match(m.store, tp)
    # the rotation is live: the same weights without it give another loss
    with torch.no_grad():
        other = oracle.mae_loss(tp, imgs, noise.double(), posemb=None, **kw)
    assert abs(other.item() - ref.item()) > 1e-4


def test_finetune_step_matches_oracle():
    torch.manual_seed(1)
    vc = ViTConfig(layers=2, dim=32, heads=2, labels=5, image_size=24, patch_size=8, posemb="rope",
                   image_mask_ratio=None, layerscale=True)
    m = FinetuneModel(vc, label_smoothing=0.1).to("cpu")
    m.store.master.add_(torch.randn_like(m.store.master) * 0.05)
    imgs = torch.randint(0, 256, (4, 3, 24, 24), dtype=torch.uint8)
    labels = torch.tensor([0, 3, 1, 4])
    out = m(imgs, labels, rngs={}, det=False)
    out["loss"].backward()
    tp = oracle.tree_to_torch(m.flax_params())
    lg = oracle.classifier_logits(tp, oracle.normalize_nhwc(imgs), layers=2, dim=32, heads=2, patch=8, posemb="rope")
    logits, _ = m.logits(imgs, None, None, det=False)
    assert torch.allclose(logits.double(), lg.detach(), atol=2e-5)
    onehot = torch.nn.functional.one_hot(labels, 5).double() * 0.9 + 0.1 / 5
    ref = -(onehot * torch.log_softmax(lg, -1)).sum(-1).mean()
    ref.backward()
    assert abs(out["loss"].item() - ref.item()) < 1e-5
    _grads_match(m.store, tp)


# ------------------------------------------------------------------------------ checkpoints
def _ft(posemb, image_size=32, **kw):
    return FinetuneModel(ViTConfig(layers=1, dim=32, heads=4, labels=10, image_size=image_size, patch_size=8,
                                   posemb=posemb, image_mask_ratio=None, **kw)).to("cpu")


def _pre(posemb, image_size=32, seed=0, **kw):
    vc = ViTConfig(layers=1, dim=32, heads=4, labels=0, image_size=image_size, patch_size=8, posemb=posemb, **kw)
    dc = DecoderConfig(dec_layers=1, dec_dim=16, dec_heads=2, image_size=image_size, patch_size=8)
    return PretrainModel(vc, dc).to("cpu", seed=seed)


def _save(tmp_path, name, model):
    url = save_params(str(tmp_path), name, model.flax_params(), "last")
    writer().flush()
    return url


def test_checkpoint_tree_and_mismatched_loads(tmp_path):
    quiet = lambda *a: None  # noqa: E731
    rope = _pre("rope", seed=3)
    embed = rope.flax_params()["model"]["embed"]
    assert "wpe" not in embed and "pos_embed" not in embed
    assert float(np.asarray(embed["rope_theta"]).reshape(-1)[0]) == 100.0  # the frozen marker, not a parameter
    assert rope.store.num_params(trainable_only=True) == _pre("sincos2d").store.num_params(trainable_only=True)
    url_rope = _save(tmp_path, "rope", rope)
    url_tab = _save(tmp_path, "tab", _pre("learnable"))
    url_sin = _save(tmp_path, "sin", _pre("sincos2d"))
    # a rope checkpoint into a model that expects wpe, and a checkpoint with wpe into a rope model
    with pytest.raises(ValueError, match="--posemb"):
        load_pretrained_params(url_rope, _ft("learnable").flax_params(), quiet)
    with pytest.raises(ValueError, match="--posemb"):
        load_pretrained_params(url_tab, _ft("rope").flax_params(), quiet)
    with pytest.raises(ValueError, match="--posemb"):  # neither does a table-free sincos2d checkpoint pass for rope
        load_pretrained_params(url_sin, _ft("rope").flax_params(), quiet)
    with pytest.raises(ValueError, match="--rope-theta"):
        load_pretrained_params(url_rope, _ft("rope", rope_theta=10.0).flax_params(), quiet)
    # the strict loads (--resume, tools) name the flag too
    with pytest.raises(KeyError, match="--posemb"):
        _pre("learnable").load_flax_params(load_params(url_rope))
    with pytest.raises(KeyError, match="--posemb"):
        _pre("rope").load_flax_params(load_params(url_tab))
    # what worked before still works: sincos2d -> learnable keeps the table's init
    load_pretrained_params(url_sin, _ft("learnable").flax_params(), quiet)
    # rope -> rope round trip, bit for bit
    back = _pre("rope")
    assert not torch.equal(back.store.master, rope.store.master)
    back.load_flax_params(load_params(url_rope))
    assert torch.equal(back.store.master, rope.store.master)


def test_rope_checkpoint_loads_at_another_image_size(tmp_path):
    lines = []
    pre = _pre("rope", image_size=64, seed=3)
    url = _save(tmp_path, "p64", pre)
    ft = _ft("rope", image_size=96)
    tree = load_pretrained_params(url, ft.flax_params(), lines.append)
    ft.store.load_flax_tree(tree, strict=True)
    assert not any("resized" in line or "mismatch" in line for line in lines), lines
    src, dst = pre.flax_params()["model"], ft.flax_params()["model"]
    for k in ("embed", "layer_0", "jumbo_mlp", "cls_tokens", "norm"):
        a, b = oracle.flatten({k: src[k]}), oracle.flatten({k: dst[k]})
        assert set(a) == set(b)
        assert all(np.array_equal(a[n], b[n]) for n in a), k
    imgs = torch.randint(0, 256, (2, 3, 96, 96), dtype=torch.uint8)
    logits, _ = ft.logits(imgs, None, None, det=True)
    assert logits.shape == (2, 10) and torch.isfinite(logits).all()


def test_converters_pass_a_rope_tree_through_without_pos_embed():
    from jumbo_mae_tpu_amd.ckpt.convert import flax_to_torch, torch_to_flax
    from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
    tree = _ft("rope", rope_theta=50.0).flax_params()
    sd = flax_to_torch(tree)
    assert "pos_embed" not in sd and float(sd["rope_theta"][0]) == 50.0
    back = torch_to_flax(sd, num_heads=4)
    a, b = flatten_tree(tree), flatten_tree({"model": back} if "model" not in back else back)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], atol=1e-6, err_msg=str(k))
