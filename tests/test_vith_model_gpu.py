"""A miniature ViT-H/14-shaped Jumbo MAE and classifier (patch 14, head dim 80; decoder head dim
96): the bf16 HIP path, with the tile-streamed attention kernels at every sequence length and the
blocks' own QKV-bias column sums, against the fp32 CPU model."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _compare_leaves(cpu, gpu, lc, lg, strict=0.99, loose=0.95):
    """Loss within 2 %; flat-gradient cosine > 0.99; every 2-D (GEMM weight) leaf > ``strict``, the
    other leaves > ``loose`` (tiny gradients -- below 1e-3 of the per-leaf RMS norm -- are skipped)."""
    assert abs(lc.item() - lg.item()) / abs(lc.item()) < 2e-2, (lc.item(), lg.item())
    gc, gg = cpu.store.grad, gpu.store.grad.cpu()
    assert _cos(gc, gg) > 0.99
    bad = []
    for s in cpu.store.segments:
        a = gc[s.offset:s.offset + s.numel]
        b = gg[s.offset:s.offset + s.numel]
        if a.norm() <= 1e-3 * gc.norm() / len(cpu.store.segments) ** 0.5:
            continue
        c = _cos(a, b)
        if c < (strict if len(s.shape) == 2 else loose):
            bad.append((s.key, len(s.shape), round(c, 4)))
    assert not bad, bad


def _pretrain_pair():
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    vc = ViTConfig(layers=2, dim=160, heads=2, labels=0, image_size=56, patch_size=14, posemb="sincos2d")
    dc = DecoderConfig(dec_layers=2, dec_dim=96, dec_heads=1, image_size=56, patch_size=14)
    assert vc.head_dim == 80
    cpu = PretrainModel(vc, dc).to("cpu", torch.float32, seed=0)
    gpu = PretrainModel(vc, dc).to("cuda", torch.bfloat16, seed=0)
    gpu.store.master.copy_(cpu.store.master)
    gpu.store.sync_shadow()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 56, 56), dtype=torch.uint8, generator=g)
    noise = torch.rand(16, generator=g)
    return cpu, gpu, imgs, noise


def test_pretrain_vith_shaped_gpu_matches_cpu():
    """Encoder head dim 80 at S = 4 kept + 3 CLS, decoder head dim 96 at S = 16 + 3."""
    cpu, gpu, imgs, noise = _pretrain_pair()
    lc = cpu(imgs, noise=noise)["loss"]
    lc.backward()
    lg = gpu(imgs.cuda(), noise=noise.cuda())["loss"]
    lg.backward()
    torch.cuda.synchronize()
    _compare_leaves(cpu, gpu, lc, lg)


def test_finetune_vith_shaped_gpu_matches_cpu():
    """Classifier at 224 px, patch 14: S = 256 + 3 = 259, head dim 80."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=160, heads=2, labels=10, image_size=224, patch_size=14, posemb="learnable")
    cpu = FinetuneModel(vc).to("cpu", torch.float32, seed=0)
    gpu = FinetuneModel(vc).to("cuda", torch.bfloat16, seed=0)
    gpu.store.master.copy_(cpu.store.master)
    gpu.store.sync_shadow()
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (2, 3, 224, 224), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    lc = cpu(imgs, labels)["loss"]
    lc.backward()
    lg = gpu(imgs.cuda(), labels.cuda())["loss"]
    lg.backward()
    torch.cuda.synchronize()
    _compare_leaves(cpu, gpu, lc, lg)


def test_vith_shaped_step_takes_the_hip_attention(monkeypatch):
    """No torch.einsum during the GPU forward + backward: the PyTorch attention composition (the
    only einsum user of the training path) is not taken at head dims 80 / 96."""
    _, gpu, imgs, noise = _pretrain_pair()
    imgs, noise = imgs.cuda(), noise.cuda()
    calls = []
    real = torch.einsum

    def spy(*a, **k):
        calls.append(a[0] if a else None)
        return real(*a, **k)

    monkeypatch.setattr(torch, "einsum", spy)
    loss = gpu(imgs, noise=noise)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert torch.isfinite(loss).item()
    assert not calls, calls
