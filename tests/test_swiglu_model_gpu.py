"""``--ffn swiglu`` / ``--dec-ffn swiglu`` end to end on the GPU (bf16 + HIP kernels), in the shape and at the
thresholds of tests/test_qknorm_model_gpu.py: loss and every gradient leaf -- the new ``w3`` leaves included --
against the fp64 oracle (models/oracle.py) evaluated on the GPU from the same weights, with rope and QK-norm on
(the whole modern recipe together), Jumbo and plain blocks, activation checkpointing, hidden dropout, the
number of gate launches, the untouched GELU path, and a HIP-graph capture and replay of a step."""

import pytest
import torch

pytestmark = pytest.mark.gpu

W3 = ("model/layer_0/ff", "model/jumbo_mlp", "decoder_model/dec_layer_1/ff")


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _pretrain(ffn, dec_ffn, grad_ckpt=False, dropout=0.0, per_scale=0.05):
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb="rope",
                   image_mask_ratio=0.75, qk_norm="rms", grad_ckpt=grad_ckpt, ffn=ffn, dropout=dropout)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16, dec_qk_norm="rms",
                       grad_ckpt=grad_ckpt, dec_ffn=dec_ffn, dec_dropout=dropout)
    m = PretrainModel(vc, dc, mask_mode="per-sample").to("cuda", torch.bfloat16, seed=0)
    with torch.no_grad():  # biases off zero, so that every leaf matters
        m.store.master.add_(torch.randn(m.store.master.shape, generator=torch.Generator().manual_seed(1)).cuda()
                            * per_scale)
    m.store.sync_shadow()
    return m


def _batch():
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 64, 64), dtype=torch.uint8, generator=g).cuda()
    return imgs, torch.rand(8, 16, generator=g).cuda()


def _against_oracle(m, loss, ref, tp):
    """tests/test_qknorm_model_gpu.py ``_against_oracle``: loss within 2 %, flat-gradient cosine > 0.99, every
    leaf that is not tiny > 0.95.  Returns the checked leaves."""
    from jumbo_mae_tpu_amd.models import oracle
    assert abs(loss.item() - ref.item()) / abs(ref.item()) < 2e-2, (loss.item(), ref.item())
    flat = oracle.flatten(tp)
    gg = m.store.grad.double()
    gr = torch.zeros_like(gg)
    for s in m.store.segments:
        r = flat[s.key].grad
        if r is not None:
            gr[s.offset:s.offset + s.numel] = torch.from_numpy(s.from_flax(r.cpu().numpy())).reshape(-1).cuda()
    assert _cos(gr, gg) > 0.99
    checked = []
    for s in m.store.segments:
        a, b = gr[s.offset:s.offset + s.numel], gg[s.offset:s.offset + s.numel]
        if a.norm() > 1e-3 * gr.norm() / len(m.store.segments) ** 0.5:
            assert _cos(a, b) > 0.95, (s.key, _cos(a, b))
            checked.append(s.key)
    return checked


@pytest.mark.parametrize("ffn,dec_ffn,grad_ckpt", [("swiglu", "swiglu", False), ("swiglu", "gelu", False),
                                                   ("gelu", "swiglu", False), ("swiglu", "swiglu", True)])
def test_pretrain_step_matches_fp64_oracle(ffn, dec_ffn, grad_ckpt):
    from jumbo_mae_tpu_amd.models import oracle
    m = _pretrain(ffn, dec_ffn, grad_ckpt=grad_ckpt)
    imgs, noise = _batch()
    loss = m(imgs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    tp = oracle.tree_to_torch(m.flax_params(), device="cuda")
    ref = oracle.mae_loss(tp, imgs, noise.double(), layers=2, dim=128, heads=2, dec_layers=2, dec_dim=64, dec_heads=2,
                          patch=16, mask_ratio=0.75, posemb="rope")
    ref.backward()
    checked = _against_oracle(m, loss, ref, tp)
    for node in W3:
        on = (dec_ffn if node.startswith("decoder") else ffn) == "swiglu"
        for leaf in ("kernel", "bias"):
            key = f"{node}/w3/{leaf}"
            assert (key in m.store.by_key) == on
            assert (key in checked) == on, (key, len(checked))


def test_finetune_step_matches_fp64_oracle():
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models import oracle
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=128, heads=4, labels=10, image_size=64, patch_size=8, posemb="rope", qk_norm="rms",
                   ffn="swiglu")
    m = FinetuneModel(vc).to("cuda", torch.bfloat16, seed=0)
    with torch.no_grad():
        m.store.master.add_(torch.randn(m.store.master.shape, generator=torch.Generator().manual_seed(2)).cuda() * 0.05)
    m.store.sync_shadow()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (4, 3, 64, 64), dtype=torch.uint8, generator=g).cuda()
    labels = torch.randint(0, 10, (4,), generator=g).cuda()
    loss = m(imgs, labels)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    tp = oracle.tree_to_torch(m.flax_params(), device="cuda")
    lg = oracle.classifier_logits(tp, oracle.normalize_nhwc(imgs).double(), layers=2, dim=128, heads=4, patch=8,
                                  posemb="rope")
    ref = torch.nn.functional.cross_entropy(lg, labels)
    ref.backward()
    checked = _against_oracle(m, loss, ref, tp)
    # (the last layer's patch feed-forward does not reach the CLS rows the head reads: layer_0's is the live one)
    assert "model/layer_0/ff/w3/kernel" in checked and "model/jumbo_mlp/w3/kernel" in checked


def _step(monkeypatch, per_op, ffn="swiglu", dec_ffn="swiglu", grad_ckpt=False, dropout=0.0):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    m = _pretrain(ffn, dec_ffn, grad_ckpt=grad_ckpt, dropout=dropout)
    imgs, noise = _batch()
    rngs = {"dropout": torch.Generator(device="cuda").manual_seed(3)} if dropout > 0 else None
    loss = m(imgs, rngs=rngs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return m, loss.item(), m.store.grad.clone()


def _fused_matches_per_op(monkeypatch, dropout):
    m, lf, gf = _step(monkeypatch, "0", dropout=dropout)
    _, lp, gp = _step(monkeypatch, "1", dropout=dropout)
    assert abs(lf - lp) <= 1e-3 * abs(lp), (lf, lp)
    floor = 1e-3 * gp.norm() / len(m.store.segments) ** 0.5  # the tiny-leaf rule of tests/test_rope_model_gpu.py
    checked = []
    for s in m.store.segments:
        a, b = gf[s.offset:s.offset + s.numel], gp[s.offset:s.offset + s.numel]
        if s.trainable and b.norm() > floor:
            assert _cos(a, b) > 0.999, (s.key, _cos(a, b))
            checked.append(s.key)
    for node in W3:
        assert f"{node}/w3/kernel" in checked and f"{node}/w3/bias" in checked, node


def test_fused_blocks_match_per_op(monkeypatch):
    _fused_matches_per_op(monkeypatch, 0.0)


def test_fused_blocks_match_per_op_with_dropout(monkeypatch):
    """Both paths draw the same seeds and regenerate the same masks."""
    _fused_matches_per_op(monkeypatch, 0.1)


def test_grad_ckpt_keeps_the_loss_bits(monkeypatch):
    _, l0, g0 = _step(monkeypatch, "0", grad_ckpt=False)
    _, l1, g1 = _step(monkeypatch, "0", grad_ckpt=True)
    assert l0 == l1
    assert torch.allclose(g0, g1, rtol=1e-5, atol=1e-6 * g0.abs().max().item())


def _count(monkeypatch):
    from jumbo_mae_tpu_amd.ops import prims as P
    names = ("swiglu_fwd", "swiglu_bwd", "linear_gelu_fwd_saved", "linear_gelu_fwd", "linear_gelu_bwd", "gelu_fwd",
             "gelu_bwd")
    calls = dict.fromkeys(names, 0)
    real = {n: getattr(P, n) for n in names}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    for n in names:
        monkeypatch.setattr(P, n, counted(n))
    return calls


def test_one_gate_launch_per_feed_forward_and_direction(monkeypatch):
    """Per Jumbo layer pair: the patch FF, the jumbo MLP and a decoder FF -- here two encoder and two decoder
    layers, so six gates each way; the GELU entry points never run in a fully gated model."""
    calls = _count(monkeypatch)
    _step(monkeypatch, "0")
    assert calls["swiglu_fwd"] == 6 and calls["swiglu_bwd"] == 6, calls
    assert not any(v for k, v in calls.items() if "gelu" in k), calls


def test_off_path_untouched(monkeypatch):
    calls = _count(monkeypatch)
    _, l0, g0 = _step(monkeypatch, "0", "gelu", "gelu")
    assert calls["swiglu_fwd"] == 0 and calls["swiglu_bwd"] == 0 and calls["linear_gelu_fwd_saved"] == 6, calls
    _, l1, g1 = _step(monkeypatch, "0", "gelu", "gelu")
    assert l0 == l1 and torch.equal(g0.view(torch.int32), g1.view(torch.int32))


def test_hip_graph_replay_matches_eager_steps():
    """Replayed pretrain steps against eager ones from the same weights and random streams (the comparison of
    tests/test_qknorm_model_gpu.py), gated feed-forwards in both stacks."""
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    from jumbo_mae_tpu_amd.runtime.graph import GraphedTrainStep
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    def make():
        vc = ViTConfig(layers=2, dim=256, heads=4, labels=0, image_size=64, patch_size=16, posemb="rope",
                       image_mask_ratio=0.75, droppath=0.1, qk_norm="rms", ffn="swiglu")
        dc = DecoderConfig(dec_layers=2, dec_dim=128, dec_heads=4, image_size=64, patch_size=16, dec_qk_norm="rms",
                           dec_ffn="swiglu")
        m = PretrainModel(vc, dc).to("cuda", torch.bfloat16, seed=0)
        opt = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 2e-3, 2, 40, 1e-5), b2=0.95,
                            weight_decay=0.05, num_layers=vc.layers)
        return m, Trainer(m, opt, None, RngStreams({"noise": 1, "dropout": 1}, 0, "cuda"))

    g = torch.Generator(device="cuda").manual_seed(0)
    data = [(torch.randint(0, 256, (32, 3, 64, 64), dtype=torch.uint8, device="cuda", generator=g),) for _ in range(4)]
    m1, t1 = make()
    m2, t2 = make()
    s = m2.store.by_key["model/layer_0/ff/w3/kernel"]
    init = m2.store.master[s.offset:s.offset + s.numel].clone()
    gs = GraphedTrainStep(t2, [data[0]], warmup=2, restore=True)
    assert torch.equal(m1.store.master, m2.store.master)
    t1.rngs.load_state_dict(t2.rngs.state_dict())  # the warm-up advanced the graphed trainer's streams
    for i in (1, 2, 3):
        a = t1.train_step([data[i]])
        b = gs([data[i]])
        assert abs(a["loss"].item() - b["loss"].item()) < 1e-4 * max(1.0, abs(a["loss"].item())), (i, a, b)
    assert gs.replays == 3
    assert not torch.equal(m2.store.master[s.offset:s.offset + s.numel], init)  # it trains
