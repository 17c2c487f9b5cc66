"""The PyTorch attention composition (CPU path; GPU path of head dims without HIP kernels and of
dropout at head dims 80 / 96 / 128) at head dim 80 against an fp64 reference."""

import math

import torch


def _attn_ref(qkv, H):
    B, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = qkv.double().view(B, S, 3, H, hd).unbind(2)
    z = torch.einsum("bqhd,bkhd->bhqk", q / math.sqrt(hd), k)
    lse = torch.logsumexp(z, -1)
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(z, -1), v).reshape(B, S, D)
    return o, lse


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def test_composition_at_head_dim_80_matches_fp64():
    from jumbo_mae_tpu_amd.ops import prims as P
    torch.manual_seed(0)
    B, S, H, hd = 2, 67, 3, 80
    D = H * hd
    qkv = torch.randn(B, S, 3 * D) * 1.5
    do = torch.randn(B, S, D)
    o, lse = P.attn_fwd(qkv, H)
    qr = qkv.double().requires_grad_()
    orf, lser = _attn_ref(qr, H)
    assert o.dtype == torch.float32 and o.shape == (B, S, D) and lse.shape == (B, H, S)
    # fp32 arithmetic (eps 6e-8) over sums of at most 80 / 67 terms
    assert rel(o, orf) < 1e-5
    assert (lse.double() - lser).abs().max().item() < 1e-4
    dqkv, done = P.attn_bwd(do, qkv, o, lse, H)
    assert done is False
    orf.backward(do.double())
    g = qr.grad.view(B, S, 3, D)
    d = dqkv.view(B, S, 3, D)
    for i in range(3):
        assert rel(d[:, :, i], g[:, :, i]) < 1e-4, i


def test_vit_huge_preset_head_dim():
    from jumbo_mae_tpu_amd.config import vit_config
    assert vit_config("vit_huge_patch14").head_dim == 80
