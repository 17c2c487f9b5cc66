"""Label-free statistics of encoder features (the ``main_pretrain`` representation monitor).

``feat_gram`` adds a batch of fp32 rows to a resident fp64 state (Gram matrix ``G = sum x x^T``,
column sums ``s``, row count ``n``); ``feat_uniformity`` returns per query the fp64 sum of
``exp(-2 t (1 - q . bank_j))`` over the eligible bank rows without ever storing a score matrix.
Both run on the kernels of ``csrc/feat_stats.hip`` for GPU inputs and on the torch compositions
``feat_gram_torch`` / ``feat_uniformity_torch`` otherwise (CPU, ``prims._FEAT_STATS_OURS`` off, and
for the uniformity a feature width that is no multiple of 32 or rows that are not bf16; the
uniformity's composition runs in fp64 on the CPU and in fp32 on a GPU).  Run in fp64 the compositions
are the oracle of the kernels, so they implement the same rules:

* a row with ``valid == 0`` is selected out, not multiplied by zero: it may hold NaN;
* ``bank_valid == 0`` removes a bank row, ``self_idx[i]`` (-1: none) the bank row that IS query ``i``.

``summary`` turns the (all-reduced) state into the logged metrics on the CPU in fp64.
"""

from __future__ import annotations

import math

import torch

from . import _ext
from . import prims as P
from .knn import _kernel_rows


def new_state(D: int, device) -> dict:
    """The empty state of ``feat_gram``: ``G`` fp64 [D, D], ``s`` fp64 [D], ``n`` fp64 [1] (valid rows)."""
    z = dict(dtype=torch.float64, device=device)
    return {"G": torch.zeros(D, D, **z), "s": torch.zeros(D, **z), "n": torch.zeros(1, **z)}


def finite_rows(x: torch.Tensor) -> torch.Tensor:
    """bool [n]: the rows of ``x`` whose entries are all finite."""
    return torch.isfinite(x).all(dim=1)


# ------------------------------------------------------------------------------ Gram
def feat_gram_torch(x: torch.Tensor, valid: torch.Tensor | None, state: dict,
                    dtype: torch.dtype = torch.float64) -> dict:
    """``state`` += the valid rows of ``x`` [n, D]: the torch composition (a ``dtype`` copy of the
    selected rows and one matmul)."""
    xs = x if valid is None else x[valid.bool()]
    xd = xs.to(dtype)
    state["G"] += (xd.t() @ xd).double()
    state["s"] += xd.sum(0).double()
    state["n"] += xs.shape[0]
    return state


def feat_gram(x: torch.Tensor, valid: torch.Tensor | None, state: dict) -> dict:
    """``state`` (``new_state``) += the rows of ``x`` fp32 [n, D] with ``valid`` (bool / uint8 [n],
    None: all) set; in place.  Every product enters ``G`` as the exact fp64 product of two fp32
    values, rows are added in ascending order: two calls equal one call on the concatenated rows (on the
    kernel bit for bit when the first call holds a multiple of 4 rows or every partial sum is exact)."""
    if x.dim() != 2 or x.shape[1] != state["s"].shape[0]:
        raise ValueError(f"feat_gram: x must be [n, {state['s'].shape[0]}] (got {tuple(x.shape)})")
    if not (P._FEAT_STATS_OURS and x.is_cuda and P.hip(x)):
        return feat_gram_torch(x, valid, state)
    x = x.float()
    if x.shape[1] > 1 and x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    v = None if valid is None else valid.to(torch.bool).contiguous()
    _ext.load().feat_gram(x, v, state["G"], state["s"])
    state["n"] += x.shape[0] if v is None else v.sum()
    return state


# ------------------------------------------------------------------------------ uniformity
def feat_uniformity_torch(q: torch.Tensor, bank: torch.Tensor, self_idx: torch.Tensor | None = None,
                          bank_valid: torch.Tensor | None = None, t: float = 2.0,
                          dtype: torch.dtype = torch.float32, block_elems: int = 1 << 24) -> torch.Tensor:
    """fp64 [Nq]: the chunked torch composition; scores, ``exp`` and the row sums in ``dtype``."""
    Nq, Nb = q.shape[0], bank.shape[0]
    e = torch.zeros(Nq, dtype=torch.float64, device=q.device)
    if Nq == 0 or Nb == 0:
        return e
    bt = bank.to(dtype).t()
    cols = torch.arange(Nb, device=q.device)
    ok = None if bank_valid is None else bank_valid.bool()
    rows = max(1, block_elems // Nb)
    for r0 in range(0, Nq, rows):
        sc = q[r0:r0 + rows].to(dtype) @ bt
        ev = torch.exp(-2.0 * t * (1.0 - sc))
        keep = torch.ones_like(ev, dtype=torch.bool)
        if self_idx is not None:
            keep &= cols[None, :] != self_idx[r0:r0 + rows].long()[:, None]
        if ok is not None:
            keep &= ok[None, :]
        e[r0:r0 + rows] = torch.where(keep, ev, torch.zeros_like(ev)).sum(1).double()
    return e


def feat_uniformity(q: torch.Tensor, bank: torch.Tensor, self_idx: torch.Tensor | None = None,
                    bank_valid: torch.Tensor | None = None, t: float = 2.0, splits: int = 0,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """fp64 [Nq]: ``e_i = sum_j exp(-2 t (1 - q_i . bank_j))`` over the bank rows with ``bank_valid``
    set (None: all) other than ``self_idx[i]`` (-1 / None: none).  ``splits``: how the kernel deals
    its bank segments to workgroups (0: one each; the result does not depend on it).  ``out``: an
    fp64 [Nq] tensor to write into."""
    if not (t > 0):
        raise ValueError(f"feat_uniformity: t must be positive (got {t})")
    ours = (P._FEAT_STATS_OURS and q.is_cuda and q.dtype == torch.bfloat16 and bank.dtype == torch.bfloat16
            and q.shape[1] % 32 == 0 and bank.shape[0] > 0 and P.hip(q))
    if not ours:  # fp64 on the CPU (the rank count must not show in a logged value), fp32 on a GPU
        e = feat_uniformity_torch(q, bank, self_idx, bank_valid, t,
                                  dtype=torch.float32 if q.is_cuda else torch.float64)
        if out is not None:
            out.copy_(e)
            return out
        return e
    si = None if self_idx is None else self_idx.to(torch.int32).contiguous()
    bv = None if bank_valid is None else bank_valid.to(torch.bool).contiguous()
    return _ext.load().feat_uniformity(_kernel_rows(q), _kernel_rows(bank), si, bv, float(t), int(splits), out)


# ------------------------------------------------------------------------------ metrics
RANKME_EPS = 1e-7  # the published definition's epsilon
KEYS = ("val/feat_rows", "val/feat_nonfinite", "val/feat_rankme", "val/feat_pr", "val/feat_top1_var",
        "val/feat_std", "val/feat_rms_norm", "val/feat_uniformity")  # everything ``summary`` may return


def summary(G: torch.Tensor, s: torch.Tensor, n: int, e_sum: float = 0.0, pairs: float = 0.0,
            nonfinite: int = 0) -> dict:
    """The logged metrics from the state of ``n`` rows, on the CPU in fp64.

    * ``val/feat_rankme``: ``exp(-sum p_k log p_k)``, ``p_k = sigma_k / sum sigma + 1e-7``, over the
      largest ``min(n, D)`` singular values ``sigma_k = sqrt(max(eig_k(G), 0))`` of the UNCENTRED
      feature matrix; left out when every sigma is 0.
    * from the centred covariance ``C = G / n - mu mu^T``, ``mu = s / n``, with eigenvalues
      ``lambda``: ``val/feat_pr = (sum lambda)^2 / sum lambda^2``, ``val/feat_top1_var = lambda_max /
      sum lambda``, ``val/feat_std`` = mean over dimensions of ``sqrt(C_dd)``.  ``C`` is a difference
      of two terms of the size of ``G / n``, so what lies at its rounding level counts as zero:
      an eigenvalue not above ``D 2^-52 trace(G) / n`` and a ``C_dd`` not above ``8 2^-52 G_dd / n``.
      ``feat_pr`` and ``feat_top1_var`` are left out when no eigenvalue remains (identical rows).
    * ``val/feat_rms_norm = sqrt(trace(G) / n)``; ``val/feat_uniformity = log(e_sum / pairs)``, left
      out when ``pairs == 0`` or ``e_sum == 0`` (every term underflowed: no finite value to log); ``val/feat_rows = n``; ``val/feat_nonfinite``.
    With ``n == 0`` only the two counts are returned."""
    n = int(n)
    out = {"val/feat_rows": float(n), "val/feat_nonfinite": float(nonfinite)}
    if n == 0:
        return out
    G = G.detach().to("cpu", torch.float64)
    s = s.detach().to("cpu", torch.float64)
    D = G.shape[0]
    u = 2.0 ** -52
    sig = torch.linalg.eigvalsh(G).clamp_(min=0).sqrt_().flip(0)[:min(n, D)]
    tot = float(sig.sum())
    if tot > 0:
        p = sig / tot + RANKME_EPS
        out["val/feat_rankme"] = math.exp(-float((p * p.log()).sum()))
    mu = s / n
    C = G / n - torch.outer(mu, mu)
    gd = torch.diagonal(G) / n
    tr = float(gd.sum())
    lam = torch.linalg.eigvalsh(C)
    lam = lam[lam > D * u * tr]
    if lam.numel() > 0:
        ls = float(lam.sum())
        out["val/feat_pr"] = ls * ls / float((lam * lam).sum())
        out["val/feat_top1_var"] = float(lam.max()) / ls
    var = torch.diagonal(C)
    var = torch.where(var > 8 * u * gd, var, torch.zeros_like(var))
    out["val/feat_std"] = float(var.sqrt().mean())
    out["val/feat_rms_norm"] = math.sqrt(max(tr, 0.0))
    if pairs > 0 and e_sum > 0:
        out["val/feat_uniformity"] = math.log(e_sum / pairs)
    return out
