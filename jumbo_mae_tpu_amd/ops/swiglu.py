"""The gate of the gated feed-forward (SwiGLU), the definition csrc/swiglu.hip implements.

    FF(x) = W2 . drop( silu(W1 x + b1) * (W3 x + b3) ) + b2        silu(g) = g * sigmoid(g)

``pre`` = [gate | up] is the [M, 2 Hs] output of ONE FF1 GEMM over the adjacent w1 | w3 segments; the gate
turns it into the [M, Hs] input of FF2.  ``swiglu_torch`` and ``swiglu_bwd_torch`` are written operation by
operation in the kernels' order and run in the dtype they are given: fp64 on the inputs' bits they are the
GPU tests' reference, in fp32 they are the CPU / per-op path of the model (ops/prims.py).

The hidden width is the parameter-matched one: three [dim, Hs] matrices hold what two [dim, 4 dim] ones do at
Hs = 8 dim / 3, rounded up to a multiple of 128 so that every K stays on the 128-deep GEMM loop
(config.py ``ffn_hidden``).
"""

from __future__ import annotations

import torch

from . import dropout as Dr


def drop_factors(seed: torch.Tensor, M: int, Hs: int, rate: float, device=None, dtype=torch.float32) -> torch.Tensor:
    """[M, Hs] keep / keep_p factors of the hidden dropout: the keep bit of a[m, c] is that of element
    m Hs + c of ops/dropout.py's generator (common.h drop_keep), as the kernels regenerate it."""
    _, scale = Dr.keep_threshold(rate)
    keep = Dr.keep_mask(seed.cpu(), M * Hs, rate).view(M, Hs).to(device if device is not None else seed.device)
    return keep.to(dtype) * scale


def _sigmoid(g: torch.Tensor):
    """(sigma, e = exp(-g)): sigma = 1 / (1 + e) saturates cleanly (e = inf -> 0, e = 0 -> 1)."""
    e = torch.exp(-g)
    return 1.0 / (1.0 + e), e


def swiglu_torch(pre: torch.Tensor, drop_mask: torch.Tensor | None = None) -> torch.Tensor:
    """a [.., Hs] = silu(g) * u (* drop_mask) of pre [.., 2 Hs] = [g | u], computed in pre's dtype in the
    kernel's order; ``drop_mask``: the [.., Hs] keep / keep_p factors (``drop_factors``) or None."""
    Hs = pre.shape[-1] // 2
    g, u = pre[..., :Hs], pre[..., Hs:]
    sig, _ = _sigmoid(g)
    a = (g * sig) * u
    if drop_mask is not None:
        a = a * drop_mask.to(a.dtype)
    return a


def swiglu_bwd_torch(pre: torch.Tensor, da: torch.Tensor, drop_mask: torch.Tensor | None = None) -> torch.Tensor:
    """dpre [.., 2 Hs] of ``swiglu_torch`` for the incoming gradient da [.., Hs], in the kernel's order:
    gate half da u sigma (1 + g (1 - sigma)), up half da silu(g), with 1 - sigma taken as e sigma where
    g >= 0 (no cancellation at large g; e <= 1 there)."""
    Hs = pre.shape[-1] // 2
    g, u = pre[..., :Hs], pre[..., Hs:]
    d = da.to(pre.dtype)
    if drop_mask is not None:
        d = d * drop_mask.to(d.dtype)
    sig, e = _sigmoid(g)
    t = torch.where(g < 0, 1.0 - sig, e * sig)  # (an overflowed e = inf meets sigma = 0 only where g < 0)
    f = 1.0 + g * t
    return torch.cat([((d * u) * sig) * f, d * (g * sig)], -1)
