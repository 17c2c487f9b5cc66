"""Attention monitor: per-head statistics of the attention softmax (``--attn-stats``).

For ``qkv [B, S, 3 D]`` (layout ``[B, S, 3, H, hd]``), ``z[b, h, q, k] = (q . k) / sqrt(hd)`` and
``p = softmax_k(z)`` (no dropout: these are the statistics of the undropped softmax), every attention
row ``(b, h, q)`` has

* ``ENT  = -sum_k p log p`` in nats (``p = 0`` adds 0; uniform attention gives ``log S``),
* ``PMAX = max_k p``,
* ``CLS  = sum_{k < n_cls} p``, the attention mass on the leading CLS tokens (0 when ``n_cls == 0``),
* ``ZMAX = max_k z``.

``attn_stats(qkv, heads, n_cls, rows_out=None)`` returns the float64 ``[H, 6]`` table, reduced over
``b`` and ``q``: ``ENT_SUM``, ``PMAX_SUM``, ``CLS_SUM`` (sums over the good rows, each row value an
fp32 number widened to fp64 before it is added), ``ZMAX`` (the largest ``ZMAX`` of the good rows,
``-inf`` if there is none), ``BAD`` (rows that are not good) and ``N = B S``.  ``rows_out`` (fp32
``[B, H, S, 4]``) receives ``(ENT, PMAX, CLS, ZMAX)`` of every row, good or not, as computed.

Rules shared by the kernel (``csrc/attn_stats.hip``) and the composition ``attn_stats_torch``:

* a row is *good* when its ``ENT`` is finite, and a row that is not good adds nothing to columns 0-3;
* a logit of ``-inf`` has ``p = 0`` and adds nothing (a row of nothing but ``-inf`` is not good);
* a NaN or ``+inf`` logit makes the row's ``ENT`` NaN: the row is not good.  A NaN in one ``q`` row
  therefore spoils that one row of that head, a NaN in one ``k`` row every row of its ``(b, h)``;
* the maxima pass over NaN: ``ZMAX`` of a row is the largest logit that is not NaN (``-inf`` if there
  is none) and ``PMAX`` is 1 / sum_k exp(z - ZMAX), NaN whenever ``ENT`` is;
* equal logits need no rule: every quantity is symmetric in the keys, and ``PMAX`` / ``ZMAX`` are
  values, not positions;
* the scale is applied to the dot product (``(q . k) / sqrt(hd)``, not ``(q / sqrt(hd)) . k``), so
  inputs whose products are exactly summable have exact logits.

bf16 GPU tensors with a head dim of ``ext.attn_head_dims()`` run on the fused kernel (the ``[S, S]``
scores never reach memory); the CPU, fp32 inputs, other head dims and ``prims._ATTN_STATS_OURS = False``
take ``attn_stats_torch``, which in fp64 is the kernel's oracle.

``collecting(n_cls)`` is the hook of the models: while the context is active every attention forward
(``ops/blocks.py _attn_fwd`` and the per-op ``models/vit.py Attention``) appends the table of its
``qkv`` to the collector, in layer order; outside it the cost is one ``is None`` test.
"""

from __future__ import annotations

import contextlib
import math

import torch

from . import _ext
from . import prims as P

COLS = ("ENT_SUM", "PMAX_SUM", "CLS_SUM", "ZMAX", "BAD", "N")
ENT_SUM, PMAX_SUM, CLS_SUM, ZMAX, BAD, N = range(6)


def _check(qkv: torch.Tensor, heads: int, n_cls: int, rows_out: torch.Tensor | None):
    if qkv.dim() != 3:
        raise ValueError(f"attn_stats: qkv must be [B, S, 3 * heads * hd] (got {tuple(qkv.shape)})")
    B, S, D3 = qkv.shape
    if heads < 1 or D3 == 0 or D3 % (3 * heads):
        raise ValueError(f"attn_stats: the last dim ({D3}) must be a multiple of 3 * heads ({3 * heads})")
    if not 0 <= n_cls <= S:
        raise ValueError(f"attn_stats: n_cls must be in 0..S (got {n_cls}, S = {S})")
    if qkv.dtype not in (torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"attn_stats: qkv must be bf16 or fp32 (got {qkv.dtype})")
    if rows_out is not None and (tuple(rows_out.shape) != (B, heads, S, 4) or rows_out.dtype != torch.float32
                                 or rows_out.device != qkv.device or not rows_out.is_contiguous()):
        raise ValueError(f"attn_stats: rows_out must be a contiguous fp32 [{B}, {heads}, {S}, 4] tensor on "
                         f"qkv's device (got {rows_out.dtype} {tuple(rows_out.shape)})")
    return B, S, D3 // 3 // heads


def attn_rows_torch(qkv: torch.Tensor, heads: int, n_cls: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``[B, H, S, 4]`` in ``dtype``: (ENT, PMAX, CLS, ZMAX) of every row, the torch composition."""
    B, S, hd = _check(qkv, heads, n_cls, None)
    q, k, _ = qkv.to(dtype).view(B, S, 3, heads, hd).unbind(2)
    z = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(hd)
    neg = torch.full_like(z, float("-inf"))
    zmax = torch.where(torch.isnan(z), neg, z).amax(-1) if S else z.new_full((B, heads, 0), float("-inf"))
    d = z - zmax[..., None]
    e = torch.exp(d)
    l = e.sum(-1)
    t = torch.where(e > 0, e * d, torch.zeros_like(e)).sum(-1)  # e = 0 adds 0, not 0 * inf
    ent = torch.log(l) - t / l
    cls = e[..., :n_cls].sum(-1) / l
    return torch.stack([ent, 1.0 / l, cls, zmax], -1)


def table_from_rows(rows: torch.Tensor) -> torch.Tensor:
    """float64 ``[H, 6]`` from row values ``[B, H, S, 4]``: the reduction of the definition."""
    B, H, S, _ = rows.shape
    r = rows.double()
    good = torch.isfinite(r[..., 0])
    zero = torch.zeros_like(r[..., 0])
    out = torch.empty(H, 6, dtype=torch.float64, device=rows.device)
    for j in range(3):
        out[:, j] = torch.where(good, r[..., j], zero).sum((0, 2))
    out[:, ZMAX] = torch.where(good, r[..., 3], torch.full_like(zero, float("-inf"))).amax((0, 2))
    out[:, BAD] = (~good).sum((0, 2)).double()
    out[:, N] = float(B * S)
    return out


def attn_stats_torch(qkv: torch.Tensor, heads: int, n_cls: int, dtype: torch.dtype = torch.float32,
                     rows_out: torch.Tensor | None = None) -> torch.Tensor:
    """The definition as a torch composition in ``dtype`` (row values rounded to fp32 before they are
    added, like the kernel's): the CPU path, the path of unsupported head dims, and in fp64 the
    kernel's oracle."""
    _check(qkv, heads, n_cls, rows_out)
    rows = attn_rows_torch(qkv, heads, n_cls, dtype).float()
    if rows_out is not None:
        rows_out.copy_(rows)
    return table_from_rows(rows)


def _ours(qkv: torch.Tensor, hd: int) -> bool:
    return (P._ATTN_STATS_OURS and qkv.is_cuda and qkv.dtype == torch.bfloat16 and P.hip(qkv)
            and hd in _ext.load().attn_head_dims())


def attn_stats(qkv: torch.Tensor, heads: int, n_cls: int, rows_out: torch.Tensor | None = None) -> torch.Tensor:
    """float64 ``[H, 6]`` (module docstring) of ``qkv [B, S, 3 D]``; ``rows_out``: fp32 ``[B, H, S, 4]``
    to receive every row's (ENT, PMAX, CLS, ZMAX)."""
    heads, n_cls = int(heads), int(n_cls)
    B, S, hd = _check(qkv, heads, n_cls, rows_out)
    if B == 0 or S == 0 or not _ours(qkv, hd):
        return attn_stats_torch(qkv, heads, n_cls, torch.float32, rows_out)
    x = qkv.contiguous()
    if x.data_ptr() % 16:  # a contiguous view at an odd offset
        x = x.clone(memory_format=torch.contiguous_format)
    return _ext.load().attn_stats(x, heads, n_cls, rows_out)


# ------------------------------------------------------------------------------ the models' hook
_COLLECTOR: list | None = None
_N_CLS = 0


@contextlib.contextmanager
def collecting(n_cls: int):
    """While active, every attention forward appends ``attn_stats(qkv, heads, n_cls)`` to the yielded
    list, in layer order.  Not re-entrant; never active inside a captured graph."""
    global _COLLECTOR, _N_CLS
    if _COLLECTOR is not None:
        raise RuntimeError("attn_stats.collecting is not re-entrant")
    out: list = []
    _COLLECTOR, _N_CLS = out, int(n_cls)
    try:
        yield out
    finally:
        _COLLECTOR = None


def observe(qkv: torch.Tensor, heads: int) -> None:
    """Called by the attention forwards when a collector is active (they test ``_COLLECTOR is None``)."""
    with torch.no_grad():
        _COLLECTOR.append(attn_stats(qkv.detach(), heads, min(_N_CLS, qkv.shape[1])))


def collect_layers(names, run, n_cls: int) -> dict:
    """``{name: float64 [H, 6]}``: ``run()`` under the collector, one table per name in layer order."""
    with torch.no_grad(), collecting(n_cls) as got:
        run()
    if len(got) != len(names):
        raise RuntimeError(f"attention monitor: {len(got)} attention forwards for {len(names)} layers")
    return dict(zip(names, got))


# ------------------------------------------------------------------------------ reading a table
def summarize(tables: dict) -> tuple[dict, list]:
    """(log values, lines) of ``{layer: [H, 6]}``: per layer ``attn/entropy`` (mean over heads of
    ``ENT_SUM`` / good rows), ``attn/entropy_min`` (the lowest head), ``attn/max_logit``,
    ``attn/max_prob``, ``attn/cls_mass``; over the layers ``val/attn_entropy_min`` and
    ``val/attn_max_logit``.  One line per (layer, head) with bad rows.  A head without a good row
    counts as NaN."""
    vals, lines = {}, []
    ent_min, z_max = float("inf"), float("-inf")
    for name, tab in tables.items():
        t = tab.detach().double().cpu()
        good = t[:, N] - t[:, BAD]
        ent, pmax, cls = (t[:, j] / good for j in (ENT_SUM, PMAX_SUM, CLS_SUM))
        vals[f"attn/entropy/{name}"] = float(ent.mean())
        vals[f"attn/entropy_min/{name}"] = float(ent.min())
        vals[f"attn/max_logit/{name}"] = float(t[:, ZMAX].max())
        vals[f"attn/max_prob/{name}"] = float(pmax.mean())
        vals[f"attn/cls_mass/{name}"] = float(cls.mean())
        e, z = vals[f"attn/entropy_min/{name}"], vals[f"attn/max_logit/{name}"]
        ent_min = e if e != e or e < ent_min else ent_min
        z_max = z if z > z_max else z_max
        for h in (t[:, BAD] > 0).nonzero().flatten().tolist():
            lines.append(f"attention monitor: {name} head {h}: {int(t[h, BAD])} of {int(t[h, N])} rows "
                         f"have no finite entropy")
    if tables:
        vals["val/attn_entropy_min"] = ent_min
        vals["val/attn_max_logit"] = z_max
    return vals, lines
