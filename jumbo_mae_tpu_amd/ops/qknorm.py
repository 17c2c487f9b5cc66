"""QK-norm of the attention layers (``--qk-norm rms`` / ``--dec-qk-norm rms``): q and k are
RMS-normalised per head before the softmax, fused with the rotary embedding into one pass.

Definition (csrc/qknorm.hip and models/oracle.py mirror it):

* **Operand.** The fused QKV tensor ``[B, S, 3*H*hd]``, viewed as ``[B, S, 3, H, hd]``. q and k of
  **every** row are normalised, CLS rows included. v is never read or written.
* **Norm.** Per (b, t, q|k, h) row ``x[hd]`` and scale ``g[hd]``, with one ``g_q`` and one ``g_k``
  per layer shared by the heads:

  * ``r = 1 / sqrt(mean(x^2) + 1e-6)``
  * ``y = x * r * g``
  * fp32 arithmetic (fp64 for fp64 tensors). The 1e-6 is ``prims.LN_EPS``.
  * The softmax scale ``1/sqrt(hd)`` stays.
* **With rope.** ``y`` of the patch rows ``t >= n_cls`` is then rotated exactly as ``ops/rope.py``
  defines. The result is rounded **once** to the tensor's dtype.
* **Backward.** Given ``dy``, the gradient of what the attention kernels consumed:

  * ``u = inverse-rotate(dy)`` on patch rows, ``u = dy`` elsewhere
  * ``xh = x * r``, ``t = u * g``, ``m = mean(t * xh)``
  * ``dx = r * (t - xh * m)``
  * ``dg += sum over (b, t, h) of u * xh``, separately for q and k
* The v third of ``dqkv`` passes through bit for bit.

The backward recomputes ``r`` from the saved pre-norm q|k (2/3 of ``qkv`` per layer); nothing is
ever divided by ``g``, so it is exact at ``g == 0``.
"""

from __future__ import annotations

import torch

from .rope import rope_torch

EPS = 1e-6  # == prims.LN_EPS (prims imports this module)
HEAD_DIMS = (32, 64, 80, 96, 128)  # what csrc/qknorm.hip instantiates: the head dims with attention kernels


def _ct(t: torch.Tensor):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _split(qkv: torch.Tensor, heads: int):
    B, S, W = qkv.shape
    hd = W // (3 * heads)
    if W != 3 * heads * hd:
        raise ValueError(f"qknorm: qkv {tuple(qkv.shape)} is not [B, S, 3 * {heads} * hd]")
    return B, S, W, hd


def _scales(g_q: torch.Tensor, g_k: torch.Tensor, hd: int, ct):
    if tuple(g_q.shape) != (hd,) or tuple(g_k.shape) != (hd,):
        raise ValueError(f"qknorm: scales {tuple(g_q.shape)}, {tuple(g_k.shape)} for head dim {hd}")
    return torch.stack([g_q, g_k]).to(ct)[:, None, :]  # [2, 1, hd] against [B, S, 2, H, hd]


def qknorm_torch(qkv: torch.Tensor, heads: int, g_q: torch.Tensor, g_k: torch.Tensor, rope=None) -> torch.Tensor:
    """The definition as a torch composition: a new tensor, qkv ``[B, S, 3 * heads * hd]`` with q and
    k normalised and (``rope``: an ``ops.rope.Rope``) the patch rows rotated; v is copied bit for
    bit.  Differentiable in qkv, g_q and g_k.  fp64 tensors are computed in fp64 (the kernels'
    oracle), everything else in fp32; the result is rounded once."""
    B, S, W, hd = _split(qkv, heads)
    ct = _ct(qkv)
    v5 = qkv.view(B, S, 3, heads, hd)
    x = v5[:, :, :2].to(ct)
    r = 1.0 / torch.sqrt(x.square().mean(-1, keepdim=True) + EPS)
    y = x * r * _scales(g_q, g_k, hd, ct)
    if rope is not None:  # rotated in ct, before the one rounding (v rides along as zeros)
        full = torch.cat([y, torch.zeros_like(y[:, :, :1])], 2).reshape(B, S, W)
        full = rope_torch(full, heads, rope.n_cls, rope.gw, rope.table, rope.pos)
        y = full.view(B, S, 3, heads, hd)[:, :, :2]
    return torch.cat([y.to(qkv.dtype), v5[:, :, 2:]], 2).reshape(B, S, W)


def qknorm_bwd_torch(dqkv: torch.Tensor, saved: torch.Tensor, heads: int, g_q: torch.Tensor, g_k: torch.Tensor,
                     rope=None):
    """The backward of the definition written out: (dx ``[B, S, 2, heads, hd]`` in dqkv's dtype, dg
    ``[2, hd]`` = (dg_q, dg_k) in fp32, or fp64 for fp64 tensors) from the gradient ``dqkv`` of the
    normalised (rotated) tensor and the forward's ``saved`` pre-norm q|k ``[B, S, 2 * heads * hd]``."""
    B, S, W, hd = _split(dqkv, heads)
    ct = _ct(dqkv)
    d = dqkv.to(ct)
    if rope is not None:
        d = rope_torch(d, heads, rope.n_cls, rope.gw, rope.table, rope.pos, inverse=True)
    u = d.view(B, S, 3, heads, hd)[:, :, :2]
    x = saved.view(B, S, 2, heads, hd).to(ct)
    r = 1.0 / torch.sqrt(x.square().mean(-1, keepdim=True) + EPS)
    xh = x * r
    t = u * _scales(g_q, g_k, hd, ct)
    dx = r * (t - xh * (t * xh).mean(-1, keepdim=True))
    dg = (u * xh).sum((0, 1, 3))
    return dx.to(dqkv.dtype), dg
