"""Attention maps: CLS attention rollout over the encoder's layers (``--attn-maps``).

For ``qkv_l [B, S, 3 D]`` (layout ``[B, S, 3, H, hd]``), layer ``l = 1..L``, with
``z = (q . k) / sqrt(hd)`` and ``p_l[b, h, q, k] = softmax_k z`` (no dropout) as in ``ops/attn_stats.py``:

**One step.**  ``r_in`` fp32 ``[B, C, S]``, ``alpha`` in ``[0, 1]``::

    step(qkv, r_in, alpha)[b, c, k] = alpha r_in[b, c, k]
                                    + (1 - alpha) / H  sum_h sum_q r_in[b, c, q] p[b, h, q, k]

a row vector times ``alpha I + (1 - alpha) mean_h P``; it preserves ``sum_k`` of every row.

**Rollout** (Abnar & Zuidema, the residual weight as ``alpha``, default 0.5): from ``r_L = one-hot(c)``,
``c < C = n_cls``, step from the last layer to the first, ``r_{l-1} = step(qkv_l, r_l, alpha)``;
``r_0[b, c, :]`` is row ``c`` of ``A_L ... A_1``.  The map of CLS token ``c`` is ``r_0[b, c, n_cls:]`` on
the patch grid, ``r_0[b, c, :n_cls]`` the mass that stays on the CLS tokens.  **Mode "last"**: one step
on layer ``L`` with ``alpha = 0``, the head-mean attention of the CLS rows of the last layer.

Rules shared by the kernel (``csrc/attn_rollout.hip``) and the composition ``rollout_step_torch``:

* a logit of ``-inf`` has ``p = 0``;
* a NaN or ``+inf`` logit anywhere in image ``b`` makes every ``out[b, :, :]`` NaN (``0 * NaN`` is not
  filtered); other images are unaffected;
* ``B == 0`` or ``S == 0`` returns an empty result (from the composition);
* the scale is applied to the dot product.

bf16 GPU tensors with a head dim of ``ext.attn_head_dims()`` and ``C <= 8`` run on the fused kernels (the
``[S, S]`` probabilities never reach memory); the CPU, fp32 inputs, other head dims, ``C > 8`` and
``prims._ATTN_MAPS_OURS = False`` take ``rollout_step_torch``, which in fp64 is the kernel's oracle.

``collecting()`` is the hook of the models: while the context is active every attention forward
(``ops/blocks.py _attn_fwd`` and the per-op ``models/vit.py Attention``) appends its detached ``qkv`` to
the collector, in layer order; outside it the cost is one ``is None`` test.  It is separate from the
collector of ``ops/attn_stats.py``: both may be active at once.
"""

from __future__ import annotations

import contextlib
import math

import torch

from . import _ext
from . import prims as P

MAX_ROWS = 8  # rows of r_in the kernel takes
MODES = ("rollout", "last")


def _check(qkv: torch.Tensor, heads: int, r_in: torch.Tensor, alpha: float):
    if qkv.dim() != 3:
        raise ValueError(f"attn_maps: qkv must be [B, S, 3 * heads * hd] (got {tuple(qkv.shape)})")
    B, S, D3 = qkv.shape
    if heads < 1 or D3 == 0 or D3 % (3 * heads):
        raise ValueError(f"attn_maps: the last dim ({D3}) must be a multiple of 3 * heads ({3 * heads})")
    if qkv.dtype not in (torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"attn_maps: qkv must be bf16, fp32 or fp64 (got {qkv.dtype})")
    if r_in.dim() != 3 or r_in.shape[0] != B or r_in.shape[2] != S or r_in.shape[1] < 1:
        raise ValueError(f"attn_maps: r_in must be [{B}, C >= 1, {S}] (got {tuple(r_in.shape)})")
    if r_in.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"attn_maps: r_in must be fp32 or fp64 (got {r_in.dtype})")
    if r_in.device != qkv.device:
        raise ValueError(f"attn_maps: r_in is on {r_in.device}, qkv on {qkv.device}")
    if not 0.0 <= alpha <= 1.0:  # a NaN fails both comparisons
        raise ValueError(f"attn_maps: alpha must be in [0, 1] (got {alpha})")
    return B, S, D3 // 3 // heads


def rollout_step_torch(qkv: torch.Tensor, heads: int, r_in: torch.Tensor, alpha: float,
                       dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One step (module docstring) as a torch composition in ``dtype``: the CPU path, the path of
    unsupported head dims, and in fp64 the kernel's oracle.  Returns ``[B, C, S]`` in ``dtype``."""
    heads, alpha = int(heads), float(alpha)
    B, S, hd = _check(qkv, heads, r_in, alpha)
    r = r_in.to(dtype)
    if B == 0 or S == 0:
        return torch.empty_like(r)
    q, k, _ = qkv.to(dtype).view(B, S, 3, heads, hd).unbind(2)
    z = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(hd)
    p = torch.softmax(z, -1)
    s = torch.einsum("bcq,bhqk->bck", r, p)
    return alpha * r + ((1.0 - alpha) / heads) * s


def _ours(qkv: torch.Tensor, hd: int, r_in: torch.Tensor) -> bool:
    return (P._ATTN_MAPS_OURS and qkv.is_cuda and qkv.dtype == torch.bfloat16 and r_in.dtype == torch.float32
            and P.hip(qkv) and r_in.shape[1] <= MAX_ROWS and hd in _ext.load().attn_head_dims())


def rollout_step(qkv: torch.Tensor, heads: int, r_in: torch.Tensor, alpha: float) -> torch.Tensor:
    """fp32 ``[B, C, S]``: one step (module docstring) of ``r_in`` through the attention of ``qkv``.  fp64 inputs
    are taken (by the composition) and computed in fp32; ``rollout_step_torch`` keeps fp64."""
    heads, alpha = int(heads), float(alpha)
    B, S, hd = _check(qkv, heads, r_in, alpha)
    if B == 0 or S == 0 or not _ours(qkv, hd, r_in):
        return rollout_step_torch(qkv, heads, r_in, alpha, torch.float32)
    x = qkv.contiguous()
    if x.data_ptr() % 16:  # a contiguous view at an odd offset
        x = x.clone(memory_format=torch.contiguous_format)
    return _ext.load().attn_rollout_step(x, heads, r_in.contiguous(), alpha)


def rollout(qkvs, heads: int, n_cls: int, alpha: float = 0.5, mode: str = "rollout") -> torch.Tensor:
    """fp32 ``[B, n_cls, S]``: the rollout of the CLS rows through the layers ``qkvs`` (first layer
    first), or with ``mode="last"`` the head-mean attention of the CLS rows in the last layer."""
    if mode not in MODES:
        raise ValueError(f"attn_maps: mode must be one of {MODES} (got {mode!r})")
    qkvs = list(qkvs)
    if not qkvs:
        raise ValueError("attn_maps: rollout needs at least one layer")
    n_cls, alpha = int(n_cls), float(alpha)
    B, S = qkvs[0].shape[0], qkvs[0].shape[1]
    if not 1 <= n_cls <= max(S, 1):
        raise ValueError(f"attn_maps: n_cls must be in 1..S (got {n_cls}, S = {S})")
    for x in qkvs:
        if x.dim() != 3 or x.shape[:2] != qkvs[0].shape[:2]:
            raise ValueError(f"attn_maps: every layer must be [{B}, {S}, 3 D] (got {tuple(x.shape)})")
    r = torch.zeros(B, n_cls, S, dtype=torch.float32, device=qkvs[0].device)
    if S:
        r[:, torch.arange(n_cls), torch.arange(n_cls)] = 1.0
    if mode == "last":
        return rollout_step(qkvs[-1], heads, r, 0.0)
    for x in reversed(qkvs):
        r = rollout_step(x, heads, r, alpha)
    return r


def patch_maps(r: torch.Tensor, n_cls: int, gh: int, gw: int) -> torch.Tensor:
    """``[B, n_cls, gh, gw]``: the patch columns of ``r [B, n_cls, n_cls + gh gw]`` on the patch grid."""
    if r.dim() != 3 or r.shape[1] != n_cls or r.shape[2] != n_cls + gh * gw:
        raise ValueError(f"attn_maps: r must be [B, {n_cls}, {n_cls} + {gh} * {gw}] (got {tuple(r.shape)})")
    return r[:, :, n_cls:].reshape(r.shape[0], n_cls, gh, gw)


def maps_and_mass(qkvs, heads: int, n_cls: int, gh: int, gw: int, alpha: float = 0.5, mode: str = "rollout") -> dict:
    """``{"maps": [B, n_cls, gh, gw], "cls_mass": [B, n_cls]}`` of the collected layers."""
    r = rollout(qkvs, heads, n_cls, alpha, mode)
    return {"maps": patch_maps(r, n_cls, gh, gw), "cls_mass": r[:, :, :n_cls].sum(-1)}


# ------------------------------------------------------------------------------ the models' hook
class Layers(list):
    """The collected qkv tensors in layer order; ``heads`` of the attention forwards that appended them."""
    heads: int | None = None


_COLLECTOR: Layers | None = None


@contextlib.contextmanager
def collecting():
    """While active, every attention forward appends its detached ``qkv [B, S, 3 D]`` to the yielded
    list, in layer order.  Not re-entrant; never active inside a captured graph."""
    global _COLLECTOR
    if _COLLECTOR is not None:
        raise RuntimeError("attn_maps.collecting is not re-entrant")
    out = Layers()
    _COLLECTOR = out
    try:
        yield out
    finally:
        _COLLECTOR = None


def observe(qkv: torch.Tensor, heads: int) -> None:
    """Called by the attention forwards when a collector is active (they test ``_COLLECTOR is None``)."""
    got = _COLLECTOR
    if got.heads is not None and got.heads != int(heads):
        raise RuntimeError(f"attention maps: layers with {got.heads} and {int(heads)} heads in one pass")
    got.heads = int(heads)
    got.append(qkv.detach())


def collect_layers(run, layers: int) -> Layers:
    """The qkv tensors of ``run()``'s attention forwards, one per layer."""
    with torch.no_grad(), collecting() as got:
        run()
    if len(got) != layers:
        raise RuntimeError(f"attention maps: {len(got)} attention forwards for {layers} layers")
    return got
