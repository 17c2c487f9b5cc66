"""Weighted k-NN classification of encoder features (the ``main_pretrain`` k-NN monitor).

``knn_topk`` / ``knn_vote`` run on the fused kernels of ``csrc/knn.hip`` for bf16 GPU inputs and on
the torch compositions ``knn_topk_torch`` / ``knn_vote_torch`` otherwise (CPU, a feature width that
is no multiple of 32, or ``prims._KNN_OURS`` off).  Run in fp64 the compositions are the oracle of
the kernels, so they implement the same rules:

* neighbours are ordered by (similarity descending, bank index ascending); missing ones (fewer
  than ``k`` eligible bank rows) are ``idx = -1``, ``sim = -inf``;
* neighbour ``j`` votes for its class with ``exp((sim_j - sim_0) / T)``, class scores are added in
  ascending ``j`` and ranked by (score descending, class id ascending).

The similarity is a plain dot product: callers pass L2-normalised rows (``normalize_features``).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ext
from . import prims as P

K_MAX = 64  # one list entry per lane of a wave (csrc/knn.hip KMAX)


def check_k(k: int) -> None:
    if not 1 <= int(k) <= K_MAX:
        raise ValueError(f"k-NN: k must be in 1..{K_MAX} (got {k})")


def normalize_features(f: torch.Tensor) -> torch.Tensor:
    """fp32 L2 normalisation over the last dim, then bf16 (the kernels' operand type)."""
    return F.normalize(f.float(), dim=-1).to(torch.bfloat16)


# ------------------------------------------------------------------------------ top-k
def knn_topk_torch(q: torch.Tensor, bank: torch.Tensor, k: int, self_idx: torch.Tensor | None = None,
                   dtype: torch.dtype = torch.float32, block_elems: int = 1 << 24):
    """(idx int32 [Nq, k], sim [Nq, k] in ``dtype``): the chunked torch composition.  A stable
    descending sort keeps equal similarities in ascending bank index (``torch.topk`` promises no
    order among equal values)."""
    check_k(k)
    Nq, Nb = q.shape[0], bank.shape[0]
    idx = torch.full((Nq, k), -1, dtype=torch.int32, device=q.device)
    sim = torch.full((Nq, k), float("-inf"), dtype=dtype, device=q.device)
    if Nq == 0 or Nb == 0:
        return idx, sim
    bt = bank.to(dtype).t()
    rows = max(1, block_elems // Nb)
    kk = min(k, Nb)
    for r0 in range(0, Nq, rows):
        s = q[r0:r0 + rows].to(dtype) @ bt
        if self_idx is not None:
            si = self_idx[r0:r0 + rows].long()
            has = si >= 0
            s[has.nonzero().squeeze(1), si[has]] = float("-inf")
        v, i = torch.sort(s, dim=1, descending=True, stable=True)
        v, i = v[:, :kk], i[:, :kk].to(torch.int32)
        sim[r0:r0 + rows, :kk] = v
        idx[r0:r0 + rows, :kk] = torch.where(torch.isinf(v) & (v < 0), torch.full_like(i, -1), i)
    return idx, sim


def _kernel_rows(t: torch.Tensor) -> torch.Tensor:
    """Rows the kernel can read: unit column stride, 16-byte aligned rows."""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) % 8) or t.data_ptr() % 16:
        t = t.contiguous()
        if t.data_ptr() % 16:  # a contiguous view at an odd offset
            t = t.clone(memory_format=torch.contiguous_format)
    return t


def knn_topk(q: torch.Tensor, bank: torch.Tensor, k: int, self_idx: torch.Tensor | None = None, splits: int = 0,
             out: tuple | None = None):
    """(idx int32 [Nq, k], sim fp32 [Nq, k]) of the ``k`` largest ``q @ bank.T`` per query.
    ``self_idx`` int [Nq]: the bank row each query skips (-1: none) -- leave-one-out.  ``splits``:
    bank slices of the kernel (0: chosen from the shape; the result does not depend on it).
    ``out``: (idx, sim) tensors to write into."""
    check_k(k)
    ours = (P._KNN_OURS and q.is_cuda and q.dtype == torch.bfloat16 and bank.dtype == torch.bfloat16
            and q.shape[1] % 32 == 0 and bank.shape[0] > 0 and P.hip(q))
    if not ours:
        idx, sim = knn_topk_torch(q, bank, k, self_idx)
        if out is not None:
            out[0].copy_(idx)
            out[1].copy_(sim)
            return out[0], out[1]
        return idx, sim
    si = None if self_idx is None else self_idx.to(torch.int32).contiguous()
    o_idx, o_sim = out if out is not None else (None, None)
    idx, sim = _ext.load().knn_topk(_kernel_rows(q), _kernel_rows(bank), int(k), si, int(splits), o_idx, o_sim)
    return idx, sim


# ------------------------------------------------------------------------------ vote
def knn_vote_torch(idx: torch.Tensor, sim: torch.Tensor, bank_labels: torch.Tensor, labels: torch.Tensor, T: float,
                   dtype: torch.dtype = torch.float64, block_rows: int = 4096):
    """(pred int32 [Nq, 5], hit1, hit5 bool [Nq]): the torch composition of the weighted vote, a
    ``k x k`` comparison per query (no [Nq, classes] tensor)."""
    Nq, k = idx.shape
    pred = torch.full((Nq, 5), -1, dtype=torch.int32, device=idx.device)
    hit1 = torch.zeros(Nq, dtype=torch.bool, device=idx.device)
    hit5 = torch.zeros(Nq, dtype=torch.bool, device=idx.device)
    bl = bank_labels.long()
    for r0 in range(0, Nq, block_rows):
        sl = slice(r0, r0 + block_rows)
        ix = idx[sl].long()
        valid = ix >= 0
        lab = torch.where(valid, bl[ix.clamp(min=0)], torch.full_like(ix, -1))
        s = sim[sl].to(dtype)
        w = torch.where(valid, torch.exp((s - s[:, :1]) / T), torch.zeros_like(s))
        same = (lab[:, :, None] == lab[:, None, :]) & valid[:, :, None] & valid[:, None, :]  # [n, i, j]
        score = torch.zeros_like(w)
        for i in range(k):  # ascending i: the order the kernel adds in
            score = score + torch.where(same[:, i, :], w[:, i:i + 1], torch.zeros_like(w))
        earlier = torch.tril(torch.ones(k, k, dtype=torch.bool, device=idx.device), -1).t()  # [i, j]: i < j
        rep = valid & ~(same & earlier).any(1)
        si, sj = score[:, :, None], score[:, None, :]
        before = rep[:, :, None] & ((si > sj) | ((si == sj) & (lab[:, :, None] < lab[:, None, :])))
        rank = before.sum(1)
        top = rep & (rank < 5)
        n, j = top.nonzero(as_tuple=True)
        p = pred[sl]
        p[n, rank[n, j]] = lab[n, j].to(torch.int32)
        pred[sl] = p
        y = labels[sl].long()
        mine = rep & (lab == y[:, None]) & (y[:, None] >= 0)
        hit1[sl] = (mine & (rank == 0)).any(1)
        hit5[sl] = (mine & (rank < 5)).any(1)
    return pred, hit1, hit5


def knn_vote(idx: torch.Tensor, sim: torch.Tensor, bank_labels: torch.Tensor, labels: torch.Tensor, T: float):
    """(pred int32 [Nq, 5], hit1, hit5 bool [Nq]) of the weighted vote over the lists of ``knn_topk``."""
    check_k(idx.shape[1])
    if not (T > 0):
        raise ValueError(f"k-NN: the temperature must be positive (got {T})")
    if not (P._KNN_OURS and idx.is_cuda and bank_labels.numel() > 0 and P.hip(idx)):
        return knn_vote_torch(idx, sim, bank_labels, labels, T)
    return _ext.load().knn_vote(idx.to(torch.int32).contiguous(), sim.float().contiguous(),
                                bank_labels.to(torch.int32).contiguous(), labels.to(torch.int32).contiguous(),
                                float(T))


# ------------------------------------------------------------------------------ classification
def knn_classify(feats: torch.Tensor, labels: torch.Tensor, k: int, T: float, bank: torch.Tensor | None = None,
                 bank_labels: torch.Tensor | None = None, self_idx: torch.Tensor | None = None):
    """Per-query (hit1, hit5) bool [N] of the weighted k-NN vote on normalised rows ``feats``.

    Without a bank: leave-one-out over ``feats`` itself.  With one: ``feats`` against ``bank``;
    ``self_idx`` [N] then names the bank row that IS the query (-1: none) and is left out.  Bank
    rows whose label is -1 (padding) are dropped before the search; a query whose label is -1
    never hits."""
    check_k(k)
    if bank is None:
        bank, bank_labels = feats, labels
        self_idx = torch.arange(feats.shape[0], device=feats.device)
    keep = bank_labels != -1
    if not bool(keep.all()):
        if self_idx is not None:
            pos = torch.cumsum(keep.long(), 0) - 1
            s = self_idx.long()
            ok = (s >= 0) & keep[s.clamp(min=0)]
            self_idx = torch.where(ok, pos[s.clamp(min=0)], torch.full_like(s, -1))
        bank, bank_labels = bank[keep], bank_labels[keep]
    N = feats.shape[0]
    if N == 0 or bank.shape[0] == 0:
        z = torch.zeros(N, dtype=torch.bool, device=feats.device)
        return z, z.clone()
    idx, sim = knn_topk(feats, bank, k, self_idx)
    _, hit1, hit5 = knn_vote(idx, sim, bank_labels, labels, T)
    return hit1, hit5
