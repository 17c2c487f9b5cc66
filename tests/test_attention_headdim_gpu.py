"""HIP attention at head dims 80 / 96 / 128 (ViT-H/14: 1280 / 16 = 80): the tile-streamed kernels
at every sequence length, against an fp64 reference incl. gradients; guarded reads, determinism,
the bindings that describe the dispatch, and the routing through ops/prims.py (MI355X)."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _attn_ref(qkv, H, mask=None):
    B, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    q, k, v = qkv.double().view(B, S, 3, H, hd).unbind(2)
    z = torch.einsum("bqhd,bkhd->bhqk", q / math.sqrt(hd), k)
    lse = torch.logsumexp(z, -1)
    p = torch.softmax(z, -1)
    if mask is not None:
        p = p * mask
    o = torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(B, S, D)
    return o, lse


def _nan_backed(t):
    """``t`` as the leading contiguous view of a larger buffer whose remaining elements are NaN:
    a read past the last row then lands in allocated memory and poisons the result."""
    n = t.numel()
    buf = torch.full((n + 64 * t.shape[-1] + 4096,), float("nan"), dtype=t.dtype, device=t.device)
    buf[:n] = t.reshape(-1)
    return buf[:n].view(t.shape)


@functools.lru_cache(maxsize=None)
def _case(B, S, H, hd):
    """Inputs and the fp64 reference (o, lse, dqkv) of one shape, computed once and left unchanged."""
    torch.manual_seed(0)
    D = H * hd
    qkv = (torch.randn(B, S, 3 * D, device="cuda") * 1.5).bfloat16()
    do = torch.randn(B, S, D, device="cuda").bfloat16()
    qr = qkv.double().requires_grad_()
    orf, lser = _attn_ref(qr, H)
    orf.backward(do.double())
    return qkv, do, orf.detach(), lser.detach(), qr.grad, _cancel_floor(qkv, do, H)


def _cancel_floor(qkv, do, H):
    """Denominators for dq / dk / dv where the exact gradient vanishes.  With a single token P = 1
    and dS = P (dP - delta) = dO.v - dO.o is exactly zero, so dq = dk = 0 and an error relative to
    the reference norm is undefined; the kernels read o in bf16, so their dS is the rounding
    residue of two equal terms.  The error is then taken relative to one of the two cancelling
    terms, dP k / sqrt(hd) for dq and dP q / sqrt(hd) for dk (same 2e-2).  Every other shape keeps
    the plain reference norm."""
    B, S, D3 = qkv.shape
    if S != 1:
        return (0.0, 0.0, 0.0)
    hd = D3 // 3 // H
    q, k, v = qkv.double().view(B, S, 3, H, hd).unbind(2)
    dp = (do.double().view(B, S, H, hd) * v).sum(-1, keepdim=True) / math.sqrt(hd)
    return ((dp * k).norm().item(), (dp * q).norm().item(), 0.0)


# one partial tile; one exactly filled tile with odd H (head offsets h * 80 are no multiples of 32
# elements); a second tile holding a single row; five tiles past the 224 of the whole-sequence
# kernels (ViT-H/14 finetune and decoder length); a single token; the ViT-H/14 encoder's sequence
# and head count
SHAPES = [(3, 52, 2), (2, 64, 3), (2, 65, 2), (1, 259, 2), (2, 1, 2)]
CASES = [(B, S, H, hd) for hd in (80, 96, 128) for B, S, H in SHAPES] + [(2, 67, 16, 80)]


@pytest.mark.parametrize("B,S,H,hd", CASES)
def test_attention_head_dims(ext, B, S, H, hd):
    D = H * hd
    qkv, do, orf, lser, gref, floor = _case(B, S, H, hd)
    qkv, do = _nan_backed(qkv), _nan_backed(do)
    o, lse = ext.attn_fwd(qkv, H)
    assert o.shape == (B, S, D) and lse.shape == (B, H, S)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    eo, el = rel(o, orf), (lse.double() - lser).abs().max().item()
    print(f"hd={hd} B={B} S={S} H={H}: rel(o)={eo:.3e} |lse-ref|={el:.3e}")
    assert eo < 1e-2
    assert el < 2e-2
    on = _nan_backed(o)
    dqkv = ext.attn_bwd(do, qkv, on, lse, H)
    assert torch.isfinite(dqkv.float()).all()
    g = gref.view(B, S, 3, D)
    d = dqkv.view(B, S, 3, D)
    for i in range(3):
        e = ((d[:, :, i].double() - g[:, :, i]).norm() / max(g[:, :, i].norm().item(), floor[i], 1e-12)).item()
        print(f"  rel(d{'qkv'[i]})={e:.3e}")
        assert e < 2e-2, i
    # one writer per element, no atomics: bit-identical reruns
    assert torch.equal(ext.attn_bwd(do, qkv, on, lse, H), dqkv)
    o2, lse2 = ext.attn_fwd(qkv, H)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


def test_bindings_describe_the_dispatch(ext):
    assert ext.attn_head_dims() == (32, 64, 80, 96, 128)
    assert ext.attn_fused_bias(67, 80) is False
    assert ext.attn_fused_bias(52, 64) is True
    assert ext.attn_fused_bias(224, 32) is True and ext.attn_fused_bias(225, 32) is False
    assert ext.attn_fused_bias(52, 128) is False and ext.attn_fused_bias(52, 88) is False


def test_no_fused_bias_gradient_at_new_head_dims(ext):
    """attn_bwd refuses dbias where the kernels cannot add it, instead of ignoring it."""
    qkv, do = _case(3, 52, 2, 80)[:2]
    o, lse = ext.attn_fwd(qkv, 2)
    dbias = torch.zeros(qkv.shape[2], device="cuda")
    with pytest.raises(RuntimeError, match="no fused bias gradient"):
        ext.attn_bwd(do, qkv, o, lse, 2, dbias)
    torch.cuda.synchronize()
    assert dbias.abs().max().item() == 0.0


def test_unsupported_head_dim_still_raises(ext):
    qkv = torch.randn(2, 52, 3 * 2 * 88, device="cuda").bfloat16()
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.attn_fwd(qkv, 2)


def test_prims_route_head_dim_80_to_hip(ext):
    """ops/prims.py at hd 80, S 67: bit-identical to the direct extension calls, and the QKV bias
    gradient is left to the caller."""
    from jumbo_mae_tpu_amd.ops import prims as P
    B, S, H, hd = 2, 67, 16, 80
    qkv, do = _case(B, S, H, hd)[:2]
    o, lse = ext.attn_fwd(qkv, H)
    dqkv = ext.attn_bwd(do, qkv, o, lse, H)
    po, plse = P.attn_fwd(qkv, H)
    assert torch.equal(po, o) and torch.equal(plse, lse)
    pd, done = P.attn_bwd(do, qkv, po, plse, H)
    assert done is False
    assert torch.equal(pd, dqkv)


def test_prims_dropout_at_head_dim_80_takes_the_composition(ext):
    """Attention-probability dropout at hd 80 stays on the PyTorch composition: fp64 reference with
    the mirrored mask (ops/dropout.py keep_mask_rows)."""
    from jumbo_mae_tpu_amd.ops import dropout as Dr
    from jumbo_mae_tpu_amd.ops import prims as P
    B, S, H, hd = 3, 52, 2, 80
    D = H * hd
    rate = 0.2
    qkv, do = _case(B, S, H, hd)[:2]
    seed = torch.tensor([0x5EED_1234_5678], dtype=torch.int64, device="cuda")
    o, lse = P.attn_fwd(qkv, H, drop=(seed, rate))
    m = Dr.keep_mask_rows(seed.cpu(), B * H * S, S, rate).view(B, H, S, S).cuda().double() / (1 - rate)
    qr = qkv.double().requires_grad_()
    orf, lser = _attn_ref(qr, H, m)
    assert rel(o, orf) < 1e-2
    assert (lse.double() - lser).abs().max().item() < 2e-2
    dqkv, done = P.attn_bwd(do, qkv, o, lse, H, drop=(seed, rate))
    assert done is False
    orf.backward(do.double())
    g = qr.grad.view(B, S, 3, D)
    d = dqkv.view(B, S, 3, D)
    for i in range(3):
        assert rel(d[:, :, i], g[:, :, i]) < 2e-2, i
    o0, _ = P.attn_fwd(qkv, H)
    assert rel(o0, orf) > 0.05  # the mask is live
