"""Reference of one attention-rollout step (ops/attn_maps.py) by plain loops in fp64, built from the bf16
values of ``qkv`` and independent of the torch composition: per (b, h, q) the logits one dot product at a
time, the softmax with ``math.exp`` / ``math.fsum``, the weighted sum over the queries key by key.  And the
structured inputs of the tests."""

import math

import numpy as np
import torch


def ref_probs(qkv: torch.Tensor, heads: int) -> np.ndarray:
    """float64 ``[B, H, S, S]``: softmax_k((q . k) / sqrt(hd)); a row with a NaN or +inf logit, or with nothing
    but -inf, is NaN."""
    B, S, D3 = qkv.shape
    hd = D3 // 3 // heads
    x = qkv.double().view(B, S, 3, heads, hd).numpy()
    p = np.zeros((B, heads, S, S))
    for b in range(B):
        for h in range(heads):
            for q in range(S):
                z = [float(np.dot(x[b, q, 0, h], x[b, k, 1, h])) / math.sqrt(hd) for k in range(S)]
                m = max((v for v in z if v == v), default=-math.inf)
                if any(v != v for v in z) or m == math.inf or m == -math.inf:
                    p[b, h, q] = math.nan
                    continue
                e = [math.exp(v - m) for v in z]
                l = math.fsum(e)
                p[b, h, q] = [v / l for v in e]
    return p


def ref_step(qkv: torch.Tensor, heads: int, r_in: torch.Tensor, alpha: float) -> np.ndarray:
    """float64 ``[B, C, S]``: alpha r_in + (1 - alpha) / H sum_h sum_q r_in[b, c, q] p[b, h, q, k]."""
    p = ref_probs(qkv, heads)
    r = r_in.double().numpy()
    B, C, S = r.shape
    out = np.zeros((B, C, S))
    for b in range(B):
        for c in range(C):
            for k in range(S):
                acc = 0.0
                for h in range(heads):
                    for q in range(S):
                        acc += r[b, c, q] * p[b, h, q, k]  # 0 * NaN stays NaN
                out[b, c, k] = alpha * r[b, c, k] + (1.0 - alpha) / heads * acc
    return out


def mean_matrix(qkv: torch.Tensor, heads: int, alpha: float) -> np.ndarray:
    """float64 ``[B, S, S]``: alpha I + (1 - alpha) mean_h P, the matrix one step multiplies by."""
    p = ref_probs(qkv, heads)
    return alpha * np.eye(p.shape[-1])[None] + (1.0 - alpha) * p.mean(1)


# ------------------------------------------------------------------------------ inputs
def dyadic_rows(B, C, S, seed=0):
    """fp32 ``[B, C, S]`` of multiples of 1/8 in [0, 1): sums of up to 2^20 of them are exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 8, (B, C, S), generator=g).float() / 8.0


def zero_query_qkv(B, S, H, hd, seed=0):
    """q = 0 and random keys: every logit is 0, attention is uniform, one step gives
    alpha r + (1 - alpha) mean_q r."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, H, hd, generator=g)
    x[:, :, 0] = 0.0
    return x.reshape(B, S, 3 * H * hd).to(torch.bfloat16)


def permutation_qkv(B, S, H, hd, seed=0, amp=128.0):
    """Every query (b, h, q) one-hot on key ``perm[b, h, q]``: key k carries the bits of k as +-amp in its first
    8 columns and +amp elsewhere, query q the code of its key.  The logit of the right key is
    amp^2 sqrt(hd), every other at least 2 amp^2 / sqrt(hd) >= 2896 below: exp underflows to an exact 0 in
    fp32 and fp64, so p is exactly the permutation matrix.  All products and sums are exact integers in fp32
    (hd amp^2 <= 2^21).  Returns (qkv bf16, perm int64 [B, H, S])."""
    assert S <= 256 and hd >= 8
    g = torch.Generator().manual_seed(seed)
    code = torch.full((S, hd), amp)
    bits = (torch.arange(S)[:, None] >> torch.arange(8)[None]) & 1
    code[:, :8] = torch.where(bits == 1, -amp, amp)
    perm = torch.stack([torch.randperm(S, generator=g) for _ in range(B * H)]).view(B, H, S)
    x = torch.zeros(B, S, 3, H, hd)
    x[:, :, 1] = code[None, :, None, :]
    x[:, :, 0] = code[perm].permute(0, 2, 1, 3)  # [B, H, S, hd] -> [B, S, H, hd]
    x[:, :, 2] = torch.randn(B, S, H, hd, generator=g)
    return x.reshape(B, S, 3 * H * hd).to(torch.bfloat16), perm


def permutation_step(r_in: torch.Tensor, perm: torch.Tensor, alpha: float) -> torch.Tensor:
    """float64: the step on ``permutation_qkv``: query q sends r[b, c, q] to key perm[b, h, q]."""
    B, H, S = perm.shape
    r = r_in.double()
    acc = torch.zeros_like(r)
    for h in range(H):
        acc.scatter_add_(2, perm[:, h].to(r.device)[:, None, :].expand_as(r), r)
    return alpha * r + (1.0 - alpha) / H * acc
