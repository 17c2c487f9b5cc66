"""``posemb="rope"`` end to end on the GPU (bf16 + HIP kernels): against the fp32 CPU path at the
thresholds of tests/test_model_gpu.py, the fused blocks against the per-op graph, activation
checkpointing, HIP-graph replay, and the untouched sincos2d path."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _compare(cpu, gpu, lc, lg):
    """tests/test_model_gpu.py: loss within 2 %, flat-gradient cosine > 0.99, every 2-D leaf > 0.95 (as every
    other leaf that is not tiny)."""
    assert abs(lc.item() - lg.item()) / abs(lc.item()) < 2e-2, (lc.item(), lg.item())
    gc, gg = cpu.store.grad, gpu.store.grad.cpu()
    assert _cos(gc, gg) > 0.99
    for s in cpu.store.segments:
        a = gc[s.offset:s.offset + s.numel]
        b = gg[s.offset:s.offset + s.numel]
        if a.norm() > 1e-3 * gc.norm() / len(cpu.store.segments) ** 0.5:
            assert _cos(a, b) > 0.95, s.key


def _pretrain_pair(mode, **kw):
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb="rope",
                   image_mask_ratio=0.75, **kw)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16)
    cpu = PretrainModel(vc, dc, mask_mode=mode).to("cpu", torch.float32, seed=0)
    gpu = PretrainModel(vc, dc, mask_mode=mode).to("cuda", torch.bfloat16, seed=0)
    with torch.no_grad():  # biases and a QKV scale that make the attention (and its bias gradient) matter
        cpu.store.master.add_(torch.randn(cpu.store.master.shape, generator=torch.Generator().manual_seed(1)) * 0.05)
    gpu.store.master.copy_(cpu.store.master)
    gpu.store.sync_shadow()
    return cpu, gpu


def _qkv_bias_segments(store):
    return [s for s in store.segments if s.path[-3:-1] in (("attn", "wq"), ("attn", "wk")) and s.path[-1] == "bias"
            and s.path[1].startswith("layer_")]


@pytest.mark.parametrize("mode", ["shared", "per-sample"])
def test_pretrain_gpu_matches_cpu(mode):
    from jumbo_mae_tpu_amd.ops import _ext
    cpu, gpu = _pretrain_pair(mode)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 64, 64), dtype=torch.uint8, generator=g)
    noise = torch.rand(16, generator=g) if mode == "shared" else torch.rand(8, 16, generator=g)
    lc = cpu(imgs, noise=noise)["loss"]
    lc.backward()
    lg = gpu(imgs.cuda(), noise=noise.cuda())["loss"]
    lg.backward()
    torch.cuda.synchronize()
    _compare(cpu, gpu, lc, lg)
    # the QKV bias gradient where the whole-sequence attention backward could add it itself (hd 64, S = 7): with
    # rope it has to be the column sum of the UN-rotated dqkv (ops/blocks.py _attn_bwd)
    assert _ext.load(True).attn_fused_bias(3 + 4, 64)
    gc, gg = cpu.store.grad, gpu.store.grad.cpu()
    segs = _qkv_bias_segments(cpu.store)
    assert len(segs) == 4
    for s in segs:
        a, b = gc[s.offset:s.offset + s.numel], gg[s.offset:s.offset + s.numel]
        assert a.norm() > 0 and _cos(a, b) > 0.99, (s.key, _cos(a, b))


@pytest.mark.parametrize("heads", [2, 4])
def test_finetune_long_sequence_gpu_matches_cpu(heads):
    """403 tokens: the tile-streamed attention kernels, every patch in order (pos None)."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=128, heads=heads, labels=10, image_size=160, patch_size=8, posemb="rope")
    cpu = FinetuneModel(vc).to("cpu", torch.float32, seed=0)
    gpu = FinetuneModel(vc).to("cuda", torch.bfloat16, seed=0)
    gpu.store.master.copy_(cpu.store.master)
    gpu.store.sync_shadow()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (4, 3, 160, 160), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (4,), generator=g)
    lc = cpu(imgs, labels)["loss"]
    lc.backward()
    lg = gpu(imgs.cuda(), labels.cuda())["loss"]
    lg.backward()
    torch.cuda.synchronize()
    _compare(cpu, gpu, lc, lg)


def _gpu_step(monkeypatch, per_op, grad_ckpt=False, posemb="rope", mode="per-sample"):
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb=posemb,
                   image_mask_ratio=0.75, grad_ckpt=grad_ckpt)  # (no layerscale: the attention leaves carry weight)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16, grad_ckpt=grad_ckpt)
    m = PretrainModel(vc, dc, mask_mode=mode).to("cuda", torch.bfloat16, seed=0)
    with torch.no_grad():
        m.store.master.add_(torch.randn(m.store.master.shape, generator=torch.Generator().manual_seed(1)).cuda() * 0.05)
    m.store.sync_shadow()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 64, 64), dtype=torch.uint8, generator=g).cuda()
    noise = (torch.rand(8, 16, generator=g) if mode == "per-sample" else torch.rand(16, generator=g)).cuda()
    loss = m(imgs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return m, loss.item(), m.store.grad.clone()


def test_fused_blocks_match_per_op(monkeypatch):
    m, lf, gf = _gpu_step(monkeypatch, "0")
    _, lp, gp = _gpu_step(monkeypatch, "1")
    assert abs(lf - lp) <= 1e-3 * abs(lp), (lf, lp)
    # Leaves whose gradient is rounding noise have no direction to compare: the decoder's (non-rotary) attention
    # k bias has an identically zero gradient -- adding one vector to every key shifts each softmax row by a
    # constant -- and what both paths hold there is ~1e-7.  They are skipped by the tiny-leaf rule of
    # tests/test_model_gpu.py (below 1e-3 of the per-leaf RMS norm).
    floor = 1e-3 * gp.norm() / len(m.store.segments) ** 0.5
    checked = []
    for s in m.store.segments:
        a, b = gf[s.offset:s.offset + s.numel], gp[s.offset:s.offset + s.numel]
        if s.trainable and b.norm() > floor:
            assert _cos(a, b) > 0.999, (s.key, _cos(a, b))
            checked.append(s.key)
    assert "model/layer_0/attn/wq/kernel" in checked and "model/layer_1/attn/wk/kernel" in checked
    print(f"[rope] fused vs per-op: {len(checked)} of {len(m.store.segments)} leaves compared")


def test_grad_ckpt_is_bit_identical(monkeypatch):
    _, l0, g0 = _gpu_step(monkeypatch, "0", grad_ckpt=False)
    _, l1, g1 = _gpu_step(monkeypatch, "0", grad_ckpt=True)
    assert l0 == l1
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))


def test_sincos2d_step_unchanged_and_reproducible(monkeypatch):
    """The rope descriptor is None for the table modes: two runs give the same bits (what the non-rope path calls
    is unchanged -- ops/blocks.py passes ``hbias`` and skips ``rope_`` exactly as before)."""
    from jumbo_mae_tpu_amd.ops import prims as P
    calls = []
    real = P.rope_
    monkeypatch.setattr(P, "rope_", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m, l0, g0 = _gpu_step(monkeypatch, "0", posemb="sincos2d", mode="shared")
    _, l1, g1 = _gpu_step(monkeypatch, "0", posemb="sincos2d", mode="shared")
    assert m.encoder.rope(None, "cuda") is None and not calls
    assert l0 == l1 and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    _gpu_step(monkeypatch, "0", posemb="rope", mode="shared")
    assert len(calls) == 2 * 2  # two encoder layers, forward and backward; never the decoder


def test_hip_graph_replays_match_eager_steps():
    """Three replayed pretrain steps against three eager ones from the same weights and random streams
    (the comparison of tests/test_graph_gpu.py); ``pos`` is the mask kernel's static int32 tensor."""
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    from jumbo_mae_tpu_amd.runtime.graph import GraphedTrainStep
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    def make():
        vc = ViTConfig(layers=2, dim=256, heads=4, labels=0, image_size=64, patch_size=16, posemb="rope",
                       image_mask_ratio=0.75, droppath=0.1)
        dc = DecoderConfig(dec_layers=2, dec_dim=128, dec_heads=4, image_size=64, patch_size=16)
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
