"""Shared by tests/test_swiglu.py and tests/test_swiglu_gpu.py: the inputs, the fp64 reference (``swiglu_torch``
/ ``swiglu_bwd_torch`` of ops/swiglu.py on the same bf16 bits -- never the kernel) and the per-element bounds of
csrc/swiglu.hip, derived in tests/test_swiglu_gpu.py's docstring from the kernel's operation order."""

import torch

from jumbo_mae_tpu_amd.ops.swiglu import drop_factors, swiglu_bwd_torch, swiglu_torch

U24 = 2.0 ** -24
C_FWD = 8      # forward, units of 2^-24 |ref|
C_GATE = 16    # backward gate half, units of 2^-24 |da| |u| sigma (1 + |g| (1 - sigma))
C_UP = 7       # backward up half, units of 2^-24 |da| |silu(g)|
C_DROP = 2     # added to each with dropout: the fp32 rounding of 1 / keep and the multiplication by it

# gate values planted in fixed columns: zeros of both signs, the zero crossing of silu' (-1.278..), sigmoid
# saturation and the range where exp(-g) or exp(g) leaves fp32's (no NaN from exp)
SPECIAL = (0.0, -0.0, 1.28, -1.28, 20.0, -20.0, 80.0, -80.0)


def inputs(M, Hs, seed=0, device="cpu"):
    """(pre [M, 2 Hs], da [M, Hs]) bf16: g = 4 randn with the SPECIAL columns, u and da = randn."""
    gen = torch.Generator().manual_seed(seed)
    g = 4.0 * torch.randn(M, Hs, generator=gen)
    for j, v in enumerate(SPECIAL):
        g[:, 3 + 11 * j] = v  # columns 3, 14, .., 80 (Hs >= 128)
    u = torch.randn(M, Hs, generator=gen)
    da = torch.randn(M, Hs, generator=gen)
    pre = torch.cat([g, u], 1).to(torch.bfloat16)
    assert torch.signbit(pre[0, 14].float())  # -0 survives
    return pre.to(device), da.to(torch.bfloat16).to(device)


def half_ulp_bf16(ref):
    """half a bf16 ulp (8 significant bits) of |ref|, fp64; the smallest normal's below it"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), e - 7)


def mask64(seed, M, Hs, rate, device):
    """fp64 keep / keep_p factors (the exact 1 / keep, not its fp32 rounding), or None at rate 0"""
    if seed is None or rate <= 0.0:
        return None
    keep = drop_factors(seed, M, Hs, rate, device, torch.float64) != 0
    return keep.double() / (1.0 - rate)


def fwd_ref(pre, mask=None):
    """(ref, bound) fp64 of the forward on the bits of pre"""
    ref = swiglu_torch(pre.double(), mask)
    c = C_FWD + (C_DROP if mask is not None else 0)
    return ref, half_ulp_bf16(ref) + c * U24 * ref.abs()


def bwd_ref(pre, da, mask=None):
    """(ref [M, 2 Hs], bound) fp64 of the backward on the bits of pre and da; the gate half's magnitude is
    |da| |u| sigma (1 + |g| (1 - sigma)) -- not |ref|, which cancels near g = -1.278 -- the up half's |da| |silu(g)|"""
    p, d = pre.double(), da.double()
    Hs = p.shape[1] // 2
    g, u = p[:, :Hs], p[:, Hs:]
    ref = swiglu_bwd_torch(p, d, mask)
    dm = d.abs() if mask is None else (d * mask).abs()
    sig = torch.sigmoid(g)
    one_minus = torch.sigmoid(-g)
    mag = torch.cat([dm * u.abs() * sig * (1.0 + g.abs() * one_minus), dm * (g * sig).abs()], 1)
    extra = C_DROP if mask is not None else 0
    c = torch.cat([torch.full_like(g, C_GATE + extra), torch.full_like(g, C_UP + extra)], 1)
    return ref, half_ulp_bf16(ref) + c * U24 * mag
