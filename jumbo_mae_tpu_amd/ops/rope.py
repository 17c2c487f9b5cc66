"""Axial 2-D rotary position embedding of the encoder's attention (``--posemb rope``).

Definition (csrc/rope.hip and models/oracle.py mirror it):

* the op works on the fused QKV tensor ``[B, S, 3 * H * hd]`` viewed as ``[B, S, 3, H, hd]``
  (ops/prims.py ``attn_fwd``); it rotates q and k, never v, and skips the first ``n_cls`` tokens of
  every sequence (the Jumbo CLS rows carry no position);
* the patch token at slot ``t >= n_cls`` has patch index ``p = t - n_cls`` (``pos is None``), or
  ``pos[t - n_cls]`` (shared ``[S_p]``) / ``pos[b, t - n_cls]`` (per-sample ``[B, S_p]``, int32) --
  a kept MAE patch keeps its grid coordinate wherever it lands -- at ``y = p // gw``, ``x = p % gw``;
* ``hd % 4 == 0``; channels ``[0, hd/2)`` of a head rotate by y, ``[hd/2, hd)`` by x; within an axis
  adjacent channels ``(2i, 2i + 1)`` are pair ``i = 0 .. hd/4 - 1`` with angle
  ``coord * theta ** (-i / (hd/4))``, coordinates unscaled integers, ``theta`` 100 by default (the
  axial RoPE-ViT value);
* the angles come from an fp32 table ``[G, hd/4, 2]`` of (cos, sin), computed in fp64 and rounded
  once (``rope_table``), ``G >= max(gh, gw)``;
* forward per pair ``o0 = x0 c - x1 s``, ``o1 = x1 c + x0 s`` in fp32 (fp64 for fp64 tensors),
  rounded once to the tensor's dtype; backward: the same with ``s -> -s`` (the transpose) on the
  gradient of the rotated tensor.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

DEFAULT_THETA = 100.0


class Rope(NamedTuple):
    """What an attention layer needs to rotate its q and k (the encoder builds one per forward)."""
    n_cls: int
    gw: int
    table: torch.Tensor  # fp32 [G, hd/4, 2]
    pos: torch.Tensor | None = None  # int32 [S_p] or [B, S_p]; None: patch t - n_cls


def check_head_dim(hd: int) -> None:
    if hd <= 0 or hd % 4 != 0:
        raise ValueError(f"--posemb rope needs a head dim that is a multiple of 4 (two axes of channel pairs), "
                         f"got {hd}")


_TABLES: dict = {}


def rope_table(G: int, hd: int, theta: float = DEFAULT_THETA, device="cpu") -> torch.Tensor:
    """fp32 [G, hd/4, 2]: (cos, sin) of ``coord * theta ** (-i / (hd/4))`` for coord < G, computed in
    fp64 and rounded once; cached per (G, hd, theta, device)."""
    check_head_dim(hd)
    if not theta > 0:
        raise ValueError(f"--rope-theta {theta}: expected > 0")
    key = (int(G), int(hd), float(theta), str(device))
    t = _TABLES.get(key)
    if t is None:
        n = hd // 4
        freq = float(theta) ** (-torch.arange(n, dtype=torch.float64) / n)
        ang = torch.arange(int(G), dtype=torch.float64)[:, None] * freq[None, :]
        t = torch.stack([ang.cos(), ang.sin()], -1).float().to(device).contiguous()
        _TABLES[key] = t
    return t


def _cos_sin(table: torch.Tensor, p: torch.Tensor, gw: int, dtype):
    """(cos, sin) [.., S_p, 1, 1, hd/2] of the patch indices p [.., S_p]: pairs [0, hd/4) by y, the rest by x."""
    p = p.long()
    G = table.shape[0]
    if not p.is_cuda and p.numel() and (int(p.min()) < 0 or int(p.max()) >= G * gw):  # (no host sync on the GPU)
        raise IndexError(f"rope: patch index outside the {G} x {gw} table")
    t = torch.cat([table[p // gw], table[p % gw]], -2).to(dtype)  # [.., S_p, hd/2, 2]
    return t[..., 0][..., None, None, :], t[..., 1][..., None, None, :]


def rope_torch(qkv: torch.Tensor, heads: int, n_cls: int, gw: int, table: torch.Tensor, pos: torch.Tensor | None = None,
               inverse: bool = False) -> torch.Tensor:
    """The definition as a torch composition: a new tensor, qkv ``[B, S, 3 * heads * hd]`` with q and k
    of the rows ``t >= n_cls`` rotated.  Differentiable.  fp64 tensors are rotated in fp64 (the
    kernel's oracle), everything else in fp32; v and the CLS rows are copied bit for bit."""
    B, S, W = qkv.shape
    hd = W // (3 * heads)
    check_head_dim(hd)
    if W != 3 * heads * hd or tuple(table.shape) != (table.shape[0], hd // 4, 2):
        raise ValueError(f"rope: qkv {tuple(qkv.shape)} with {heads} heads against table {tuple(table.shape)}")
    Sp = S - n_cls
    if pos is None:
        p = torch.arange(Sp, device=qkv.device)
    else:
        p = pos.to(qkv.device)
        if tuple(p.shape) not in ((Sp,), (B, Sp)):
            raise ValueError(f"rope: pos {tuple(p.shape)} for {Sp} patch rows of {B} sequences")
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    c, s = _cos_sin(table.to(qkv.device), p, gw, ct)
    if inverse:
        s = -s
    v5 = qkv.view(B, S, 3, heads, hd)
    x = v5[:, n_cls:, :2].to(ct)  # [B, S_p, 2, heads, hd]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    rot = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(x.shape).to(qkv.dtype)
    qk = torch.cat([v5[:, :n_cls, :2], rot], 1)
    return torch.cat([qk, v5[:, :, 2:]], 2).reshape(B, S, W)
