"""``--qk-norm rms`` / ``--dec-qk-norm rms`` end to end on the GPU (bf16 + HIP kernels), in the shape and at
the thresholds of tests/test_rope_model_gpu.py: loss and every gradient leaf -- the new scale leaves
included -- against the fp64 oracle (models/oracle.py) evaluated on the GPU from the same weights, with and
without rope, Jumbo and plain blocks, activation checkpointing, one launch per layer and direction, and a
HIP-graph capture and replay of a step."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _pretrain(posemb, qk, dqk, mode="per-sample", grad_ckpt=False, per_scale=0.05):
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb=posemb,
                   image_mask_ratio=0.75, qk_norm=qk, grad_ckpt=grad_ckpt)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16, dec_qk_norm=dqk,
                       grad_ckpt=grad_ckpt)
    m = PretrainModel(vc, dc, mask_mode=mode).to("cuda", torch.bfloat16, seed=0)
    with torch.no_grad():  # biases, a QKV scale and QK-norm scales off one, so that every leaf matters
        m.store.master.add_(torch.randn(m.store.master.shape, generator=torch.Generator().manual_seed(1)).cuda()
                            * per_scale)
    m.store.sync_shadow()
    return m


def _batch(mode="per-sample"):
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 64, 64), dtype=torch.uint8, generator=g).cuda()
    noise = (torch.rand(8, 16, generator=g) if mode == "per-sample" else torch.rand(16, generator=g)).cuda()
    return imgs, noise


def _against_oracle(m, loss, ref, tp):
    """tests/test_rope_model_gpu.py ``_compare`` with the fp64 oracle's gradients in the CPU path's place: loss
    within 2 %, flat-gradient cosine > 0.99, every leaf that is not tiny > 0.95."""
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


@pytest.mark.parametrize("posemb,qk,dqk,grad_ckpt", [("rope", "rms", "rms", False), ("sincos2d", "rms", "none", False),
                                                     ("rope", "none", "rms", False), ("rope", "rms", "rms", True)])
def test_pretrain_step_matches_fp64_oracle(posemb, qk, dqk, grad_ckpt):
    """Jumbo blocks (encoder) and plain blocks (decoder), each with and without QK-norm, with and without rope."""
    from jumbo_mae_tpu_amd.models import oracle
    m = _pretrain(posemb, qk, dqk, grad_ckpt=grad_ckpt)
    imgs, noise = _batch()
    loss = m(imgs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    tp = oracle.tree_to_torch(m.flax_params(), device="cuda")
    ref = oracle.mae_loss(tp, imgs, noise.double(), layers=2, dim=128, heads=2, dec_layers=2, dec_dim=64, dec_heads=2,
                          patch=16, mask_ratio=0.75, posemb=posemb)
    ref.backward()
    checked = _against_oracle(m, loss, ref, tp)
    for stack, on in (("model/layer_0", qk == "rms"), ("decoder_model/dec_layer_1", dqk == "rms")):
        for n in ("q_norm", "k_norm"):
            key = f"{stack}/attn/{n}/scale"
            assert (key in m.store.by_key) == on
            assert (key in checked) == on, (key, len(checked))


def test_finetune_step_matches_fp64_oracle():
    """67 tokens at hd 32, every patch in order (pos None), labels and the head."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models import oracle
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=128, heads=4, labels=10, image_size=64, patch_size=8, posemb="rope", qk_norm="rms")
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
    assert "model/layer_1/attn/q_norm/scale" in checked and "model/layer_0/attn/k_norm/scale" in checked


def _step(monkeypatch, per_op, grad_ckpt=False, qk="rms", dqk="rms", posemb="rope"):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    m = _pretrain(posemb, qk, dqk, grad_ckpt=grad_ckpt)
    imgs, noise = _batch()
    loss = m(imgs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return m, loss.item(), m.store.grad.clone()


def test_fused_blocks_match_per_op(monkeypatch):
    m, lf, gf = _step(monkeypatch, "0")
    _, lp, gp = _step(monkeypatch, "1")
    assert abs(lf - lp) <= 1e-3 * abs(lp), (lf, lp)
    floor = 1e-3 * gp.norm() / len(m.store.segments) ** 0.5  # the tiny-leaf rule of tests/test_rope_model_gpu.py
    checked = []
    for s in m.store.segments:
        a, b = gf[s.offset:s.offset + s.numel], gp[s.offset:s.offset + s.numel]
        if s.trainable and b.norm() > floor:
            assert _cos(a, b) > 0.999, (s.key, _cos(a, b))
            checked.append(s.key)
    assert "model/layer_0/attn/q_norm/scale" in checked and "decoder_model/dec_layer_0/attn/k_norm/scale" in checked


def test_grad_ckpt_recomputes_saved(monkeypatch):
    """Under activation checkpointing the pre-norm q|k is recomputed: the loss and every attention leaf -- the
    scales included -- keep their bits.  (Not every leaf does, with or without QK-norm: unchecked blocks are
    linked, and a linked block's ff/w2 bias gradient is summed by the upper block's LayerNorm backward kernel,
    a checkpointed block's by the residual backward kernel, in another order; those agree to fp32 rounding.)"""
    m, l0, g0 = _step(monkeypatch, "0", grad_ckpt=False)
    _, l1, g1 = _step(monkeypatch, "0", grad_ckpt=True)
    assert l0 == l1
    n = 0
    for s in m.store.segments:
        a, b = g0[s.offset:s.offset + s.numel], g1[s.offset:s.offset + s.numel]
        if "attn" in s.path:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s.key
            n += 1
        else:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * g0.abs().max().item()), s.key
    assert n == 4 * 10  # four layers: wq wk wv wo kernels and biases, q_norm, k_norm


def test_one_launch_per_layer_and_direction_and_off_path_untouched(monkeypatch):
    """With rope and QK-norm the fused op is the only q|k pass: ``rope_`` is never called; without QK-norm the
    fused op is never called and ``rope_`` runs as before."""
    from jumbo_mae_tpu_amd.ops import prims as P
    calls = {"rope": 0, "fwd": 0, "bwd": 0}
    real = {"rope": P.rope_, "fwd": P.qknorm_fwd_, "bwd": P.qknorm_bwd_}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    monkeypatch.setattr(P, "rope_", counted("rope"))
    monkeypatch.setattr(P, "qknorm_fwd_", counted("fwd"))
    monkeypatch.setattr(P, "qknorm_bwd_", counted("bwd"))
    _step(monkeypatch, "0")
    assert calls == {"rope": 0, "fwd": 4, "bwd": 4}  # two encoder and two decoder layers
    calls.update(rope=0, fwd=0, bwd=0)
    _, l0, g0 = _step(monkeypatch, "0", qk="none", dqk="none")
    assert calls == {"rope": 4, "fwd": 0, "bwd": 0}
    _, l1, g1 = _step(monkeypatch, "0", qk="none", dqk="none")
    assert l0 == l1 and torch.equal(g0.view(torch.int32), g1.view(torch.int32))


def test_monitors_see_the_normalised_tensor():
    """--attn-stats observes what the softmax sees: with scales of 0.5 no logit can exceed hd 0.25 / sqrt(hd)."""
    from jumbo_mae_tpu_amd.ops import attn_stats as AS
    m = _pretrain("rope", "rms", "none")
    hd = 64
    for layer in m.encoder.layers:
        with torch.no_grad():
            layer.attn.q_norm.master.fill_(0.5)
            layer.attn.k_norm.master.fill_(0.5)
    seen = []
    real = AS.observe
    try:
        AS._COLLECTOR = object()
        AS.observe = lambda qkv, heads: seen.append(qkv.detach().float().clone())
        imgs, noise = _batch()
        with torch.no_grad():
            m(imgs, noise=noise)
    finally:
        AS._COLLECTOR = None
        AS.observe = real
    assert len(seen) >= 2
    for qkv in seen[:2]:
        qk = qkv.view(qkv.shape[0], qkv.shape[1], 3, 2, hd)[:, :, :2]
        rms = qk.square().mean(-1).sqrt()
        assert (rms - 0.5).abs().max().item() < 0.01, rms


def test_hip_graph_replay_matches_eager_steps():
    """Replayed pretrain steps against eager ones from the same weights and random streams (the comparison of
    tests/test_rope_model_gpu.py), QK-norm in both stacks, rope in the encoder."""
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    from jumbo_mae_tpu_amd.runtime.graph import GraphedTrainStep
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    def make():
        vc = ViTConfig(layers=2, dim=256, heads=4, labels=0, image_size=64, patch_size=16, posemb="rope",
                       image_mask_ratio=0.75, droppath=0.1, qk_norm="rms")
        dc = DecoderConfig(dec_layers=2, dec_dim=128, dec_heads=4, image_size=64, patch_size=16, dec_qk_norm="rms")
        m = PretrainModel(vc, dc).to("cuda", torch.bfloat16, seed=0)
        opt = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 2e-3, 2, 40, 1e-5), b2=0.95,
                            weight_decay=0.05, num_layers=vc.layers)
        return m, Trainer(m, opt, None, RngStreams({"noise": 1, "dropout": 1}, 0, "cuda"))

    g = torch.Generator(device="cuda").manual_seed(0)
    data = [(torch.randint(0, 256, (32, 3, 64, 64), dtype=torch.uint8, device="cuda", generator=g),) for _ in range(4)]
    m1, t1 = make()
    m2, t2 = make()
    gs = GraphedTrainStep(t2, [data[0]], warmup=2, restore=True)
    assert torch.equal(m1.store.master, m2.store.master)
    t1.rngs.load_state_dict(t2.rngs.state_dict())  # the warm-up advanced the graphed trainer's streams
    for i in (1, 2, 3):
        a = t1.train_step([data[i]])
        b = gs([data[i]])
        assert abs(a["loss"].item() - b["loss"].item()) < 1e-4 * max(1.0, abs(a["loss"].item())), (i, a, b)
    assert gs.replays == 3
    s = m2.store.by_key["model/layer_0/attn/q_norm/scale"]
    assert not torch.equal(m2.store.master[s.offset:s.offset + s.numel], torch.ones(64, device="cuda"))  # it trains
