"""Attention-probability dropout inside the tile-streamed attention kernels (head dims 80 / 96 / 128
at every S, 32 / 64 past S = 224): fp64 reference with the mirrored mask, the mask read back bit
by bit through one-hot operands, a single token, the routing through ops/prims.py and a finetune
model against the composition with identical seeds (MI355X)."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

RATE = 0.2
KEEP = 1.0 - RATE
SEED = 0x5EED_1234_5678


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _seed(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def _mask(seed_value, B, H, S):
    """bool [B, H, S(q), S(k)] keep bits from the CPU mirror."""
    from jumbo_mae_tpu_amd.ops import dropout as Dr
    return Dr.keep_mask_rows(torch.tensor([seed_value], dtype=torch.int64), B * H * S, S, RATE).view(B, H, S, S)


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


def _cancel_floor(qkv, do, H):
    """Denominators for dq / dk where the exact gradient vanishes (a single token: P = 1 and
    dS = P (M dP / keep - delta) is the rounding residue of two equal terms, both zero when the
    key is dropped): the error is taken relative to one cancelling term of the undropped problem,
    dP k / sqrt(hd) for dq and dP q / sqrt(hd) for dk.  Every other shape keeps the reference norm."""
    B, S, D3 = qkv.shape
    if S != 1:
        return (0.0, 0.0, 0.0)
    hd = D3 // 3 // H
    q, k, v = qkv.double().view(B, S, 3, H, hd).unbind(2)
    dp = (do.double().view(B, S, H, hd) * v).sum(-1, keepdim=True) / math.sqrt(hd)
    return ((dp * k).norm().item(), (dp * q).norm().item(), 0.0)


@functools.lru_cache(maxsize=None)
def _case(B, S, H, hd, seed_value=SEED):
    """Inputs and the fp64 reference (o, lse, dqkv) with the mirrored mask / keep of one shape,
    computed once and left unchanged."""
    torch.manual_seed(0)
    D = H * hd
    qkv = (torch.randn(B, S, 3 * D, device="cuda") * 1.5).bfloat16()
    do = torch.randn(B, S, D, device="cuda").bfloat16()
    m = _mask(seed_value, B, H, S).cuda().double() / KEEP
    qr = qkv.double().requires_grad_()
    orf, lser = _attn_ref(qr, H, m)
    orf.backward(do.double())
    return qkv, do, orf.detach(), lser.detach(), qr.grad, _cancel_floor(qkv, do, H)


def _check_against_fp64(ext, B, S, H, hd, seed_value=SEED):
    D = H * hd
    qkv, do, orf, lser, gref, floor = _case(B, S, H, hd, seed_value)
    qkv, do = _nan_backed(qkv), _nan_backed(do)
    seed = _seed(seed_value)
    o, lse = ext.attn_fwd(qkv, H, seed, RATE)
    assert o.shape == (B, S, D) and lse.shape == (B, H, S)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    eo, el = rel(o, orf), (lse.double() - lser).abs().max().item()
    print(f"hd={hd} B={B} S={S} H={H}: rel(o)={eo:.3e} |lse-ref|={el:.3e}")
    assert eo < 1e-2
    assert el < 2e-2
    o0, lse0 = ext.attn_fwd(qkv, H)
    if S > 1:
        assert rel(o0, orf) > 0.05  # the mask is live
    assert torch.equal(lse, lse0)  # row statistics of the undropped P, bit for bit
    on = _nan_backed(o)
    dqkv = ext.attn_bwd(do, qkv, on, lse, H, None, seed, RATE)
    assert torch.isfinite(dqkv.float()).all()
    g = gref.view(B, S, 3, D)
    d = dqkv.view(B, S, 3, D)
    for i in range(3):
        e = ((d[:, :, i].double() - g[:, :, i]).norm() / max(g[:, :, i].norm().item(), floor[i], 1e-12)).item()
        print(f"  rel(d{'qkv'[i]})={e:.3e}")
        assert e < 2e-2, i
    # one writer per element, the mask a pure function of the seed: bit-identical reruns
    assert torch.equal(ext.attn_bwd(do, qkv, on, lse, H, None, seed, RATE), dqkv)
    o2, lse2 = ext.attn_fwd(qkv, H, seed, RATE)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    return o, d


# ------------------------------------------------------------------------ 1. kernels vs fp64
# one partial tile, even S; a full tile with odd H; a second tile of one row with odd S (SE = S + 1);
# five tiles.  Head dims 32 / 64: the first length past the whole-sequence kernels (odd), and five
# tiles with odd H at 64.
SHAPES = [(3, 52, 2), (2, 64, 3), (2, 65, 2), (1, 259, 2)]
CASES = [(B, S, H, hd) for hd in (80, 96, 128) for B, S, H in SHAPES] + \
        [(2, 225, 2, 32), (2, 225, 2, 64), (1, 259, 3, 64)]


@pytest.mark.parametrize("B,S,H,hd", CASES)
def test_stream_dropout_vs_fp64(ext, B, S, H, hd):
    _check_against_fp64(ext, B, S, H, hd)


# ------------------------------------------------------------------- 2. exact mask read-back
# Q = 0 makes P uniform (1 / S), so a one-hot operand copies single mask bits into the output: an
# fp64 norm can hide a few wrong bits at tile edges, a comparison of booleans cannot.
READBACK = [(2, 259, 2, 80), (2, 65, 2, 80), (2, 259, 2, 64), (2, 65, 2, 64)]


def _onehot(S, hd, j):
    """[S, hd]: 1 where row == hd * j + column."""
    r = torch.arange(S, device="cuda")[:, None]
    c = torch.arange(hd, device="cuda")[None, :]
    return (r == hd * j + c).float()


def _blocks(S, hd):
    return range((S + hd - 1) // hd)


def _qkv(B, S, H, hd, k=None, v=None):
    """qkv [B, S, 3 * H * hd] with Q = 0 and the given [S, hd] K / V in every (b, h)."""
    t = torch.zeros(B, S, 3, H, hd, device="cuda")
    t[:, :, 1] = (torch.randn(S, hd, device="cuda") if k is None else k)[None, :, None, :]
    t[:, :, 2] = (torch.randn(S, hd, device="cuda") if v is None else v)[None, :, None, :]
    return t.reshape(B, S, 3 * H * hd).bfloat16()


@pytest.mark.parametrize("B,S,H,hd", READBACK)
def test_forward_reads_back_the_mask(ext, B, S, H, hd):
    torch.manual_seed(1)
    mask = _mask(SEED, B, H, S).cuda()  # [B, H, q, k]
    seed = _seed()
    for j in _blocks(S, hd):
        n = min(hd, S - hd * j)  # key hd * j + d exists for d < n
        o, _ = ext.attn_fwd(_qkv(B, S, H, hd, v=_onehot(S, hd, j)), H, seed, RATE)
        got = o.view(B, S, H, hd).permute(0, 2, 1, 3) != 0  # [B, H, q, d]
        assert torch.equal(got[..., :n], mask[..., hd * j:hd * j + n]), j
        assert not got[..., n:].any(), j


@pytest.mark.parametrize("B,S,H,hd", READBACK)
def test_dkv_kernel_reads_back_the_mask(ext, B, S, H, hd):
    torch.manual_seed(2)
    mask = _mask(SEED, B, H, S).cuda()
    seed = _seed()
    qkv = _qkv(B, S, H, hd)
    o, lse = ext.attn_fwd(qkv, H, seed, RATE)
    for j in _blocks(S, hd):
        n = min(hd, S - hd * j)  # query hd * j + d exists for d < n
        do = _onehot(S, hd, j)[None, :, None, :].expand(B, S, H, hd).reshape(B, S, H * hd).bfloat16().contiguous()
        dqkv = ext.attn_bwd(do, qkv, o, lse, H, None, seed, RATE)
        dv = dqkv.view(B, S, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3) != 0  # [B, H, k, d]
        want = mask[:, :, hd * j:hd * j + n, :].transpose(2, 3)  # [B, H, k, q = hd * j + d]
        assert torch.equal(dv[..., :n], want), j
        assert not dv[..., n:].any(), j


@pytest.mark.parametrize("B,S,H,hd", READBACK)
def test_dq_kernel_reads_back_the_mask(ext, B, S, H, hd):
    """K one-hot, V and dO constant: dS[q, k] is proportional to M[q, k] - (kept fraction of row q),
    so the sign of dq[q, d] is the keep bit of key hd * j + d on every row with a dropped key."""
    mask_cpu = _mask(SEED, B, H, S)
    skipped = mask_cpu.all(-1)  # fully kept rows carry no sign
    assert skipped.float().mean().item() <= 1e-3
    assert not skipped.any()  # and with this seed there is none (probability < 1e-6 per row)
    mask = mask_cpu.cuda()
    seed = _seed()
    ones = torch.ones(S, hd, device="cuda")
    do = torch.ones(B, S, H * hd, device="cuda").bfloat16()
    for j in _blocks(S, hd):
        n = min(hd, S - hd * j)
        qkv = _qkv(B, S, H, hd, k=_onehot(S, hd, j), v=ones)
        o, lse = ext.attn_fwd(qkv, H, seed, RATE)
        dqkv = ext.attn_bwd(do, qkv, o, lse, H, None, seed, RATE)
        dq = dqkv.view(B, S, 3, H, hd)[:, :, 0].permute(0, 2, 1, 3) > 0  # [B, H, q, d]
        assert torch.equal(dq[..., :n], mask[..., hd * j:hd * j + n]), j


# --------------------------------------------------------------------------- 3. single token
def test_single_token(ext):
    """S = 1: o is v / keep or 0 per the mirror; dq / dk vanish exactly (cancelling-term floor)."""
    B, S, H, hd = 2, 1, 2, 80
    # the first seed from SEED on whose four (b, h) bits hold a kept and a dropped one
    sv = next(s for s in range(SEED, SEED + 64) if 0 < int(_mask(s, B, H, S).sum()) < B * H)
    o, d = _check_against_fp64(ext, B, S, H, hd, sv)
    kept = _mask(sv, B, H, S).view(B, H).cuda()
    qkv = _case(B, S, H, hd, sv)[0]
    v = qkv.view(B, S, 3, H, hd)[:, 0, 2]  # [B, H, hd]
    ov = o.view(B, H, hd)
    assert (ov[~kept] == 0).all()
    assert rel(ov[kept], v[kept].float() / KEEP) < 1e-2
    assert (d[:, :, 2].view(B, H, hd)[~kept] == 0).all()


# -------------------------------------------------------------------------------- 4. routing
@pytest.mark.parametrize("B,S,H,hd", [(2, 67, 16, 80), (1, 259, 2, 64)])
def test_prims_route_dropout_to_hip(ext, monkeypatch, B, S, H, hd):
    """ops/prims.py with ``drop`` on the tile-streamed shapes: the HIP kernels, bit-identical to the
    direct extension calls -- no CPU mask, no composition."""
    from jumbo_mae_tpu_amd.ops import dropout as Dr
    from jumbo_mae_tpu_amd.ops import prims as P
    torch.manual_seed(0)
    D = H * hd
    qkv = (torch.randn(B, S, 3 * D, device="cuda") * 1.5).bfloat16()
    do = torch.randn(B, S, D, device="cuda").bfloat16()
    seed = _seed()
    o, lse = ext.attn_fwd(qkv, H, seed, RATE)
    dqkv = ext.attn_bwd(do, qkv, o, lse, H, None, seed, RATE)

    def spy(*a, **k):
        raise AssertionError("the composition ran")

    monkeypatch.setattr(Dr, "keep_mask_rows", spy)
    monkeypatch.setattr(torch, "einsum", spy)
    po, plse = P.attn_fwd(qkv, H, drop=(seed, RATE))
    pd, done = P.attn_bwd(do, qkv, po, plse, H, drop=(seed, RATE))
    assert torch.equal(po, o) and torch.equal(plse, lse)
    assert done is False
    assert torch.equal(pd, dqkv)


def test_attn_dropout_binding(ext):
    assert ext.attn_dropout(259, 80) is True
    assert ext.attn_dropout(787, 64) is True
    assert ext.attn_dropout(52, 64) is True
    assert ext.attn_dropout(52, 88) is False


def test_no_fused_bias_gradient_with_a_seed(ext):
    B, S, H, hd = 3, 52, 2, 80
    qkv, do = _case(B, S, H, hd)[:2]
    seed = _seed()
    o, lse = ext.attn_fwd(qkv, H, seed, RATE)
    dbias = torch.zeros(qkv.shape[2], device="cuda")
    with pytest.raises(RuntimeError, match="no fused bias gradient"):
        ext.attn_bwd(do, qkv, o, lse, H, dbias, seed, RATE)
    torch.cuda.synchronize()
    assert dbias.abs().max().item() == 0.0


# ---------------------------------------------------------------------------- 5. model level
@pytest.mark.parametrize("dim,patch,image,n", [(160, 14, 56, 8), (128, 16, 256, 2)])
def test_finetune_model_matches_the_composition(monkeypatch, dim, patch, image, n):
    """Finetune ViT with dropout 0.1 at head dim 80, S 19 and at head dim 64, S 259: dropout inside
    the tile-streamed kernels == the composition with the same seeds, up to bf16 rounding."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.ops import prims as P

    res = []
    for tiled in (True, False):
        monkeypatch.setattr(P, "_ATTN_DROP_TILED", tiled)
        vc = ViTConfig(layers=2, dim=dim, heads=2, labels=16, image_size=image, patch_size=patch, posemb="sincos2d",
                       dropout=0.1)
        m = FinetuneModel(vc, label_smoothing=0.1).to("cuda", torch.bfloat16, seed=0)
        imgs = torch.randint(0, 256, (n, 3, image, image), dtype=torch.uint8,
                             generator=torch.Generator().manual_seed(2)).cuda()
        labels = torch.arange(n, device="cuda")
        m.store.zero_grad()
        out = m.forward(imgs, labels, rngs={"dropout": torch.Generator(device="cuda").manual_seed(3)}, det=False)
        out["loss"].backward()
        torch.cuda.synchronize()
        res.append((float(out["loss"]), m.store.grad.clone()))
    print(f"loss hip {res[0][0]:.5f} composition {res[1][0]:.5f}  "
          f"grad rel {float((res[0][1] - res[1][1]).norm() / res[1][1].norm()):.3e}")
    assert abs(res[0][0] - res[1][0]) < 2e-2 * abs(res[1][0])
    assert float((res[0][1] - res[1][1]).norm() / res[1][1].norm()) < 3e-2
