"""Evaluation report (``--eval-report``): per-class accuracy, calibration and confusion of a classifier from
the logits of its validation pass.

Per row with logits ``z`` (``L`` classes, bf16 or fp32, widened exactly) and an integer label ``y``:
  * ``y == -1`` is a padded row: counted in ``padded`` and nothing else; any other out-of-range label is
    clamped to ``[0, L - 1]`` as ``cls_loss`` does;
  * a row with a NaN, or whose maximum is not finite, is non-finite: counted in ``nonfinite`` and left out of
    everything else (single ``-inf`` elements are legal and contribute 0);
  * ``pred`` = arg-max, lowest index on a tie; ``rank`` = #{c : z_c > z_y or (z_c == z_y and c < y)}, the rule
    of csrc/loss.hip, so ``hit1 = rank == 0`` and ``hit5 = rank < min(5, L)`` are ``cls_loss``'s hits;
  * ``conf`` = the probability of ``pred`` in fp64, rounded once to fp32: ``1 / sum_c exp(z_c - max)`` (ce) or
    ``sigmoid(z_pred)`` (bce);
  * ``q = llrint(conf * 2^32)`` (exact) and ``bin = min(n_bins - 1, floor(conf * n_bins))`` (the product is
    exact in fp64): bins are ``[lo, hi)``, the last one closed.
Padded and non-finite rows carry ``pred = rank = -1, conf = 0``.

Everything accumulated is an integer (one flat int64 tensor, ``layout``), so the state is bit-identical for
any batch size, batch order and rank count, and the ranks combine with one exact int64 all-reduce.  The
metrics are computed from it in fp64 on the host (``EvalReport.summary``).

``eval_rows_torch`` / ``eval_accumulate_torch`` are the definition and the CPU path; on the GPU
``eval_rows`` / ``eval_accumulate`` run csrc/eval_report.hip unless ``prims._EVAL_REPORT_OURS`` is off.
"""

from __future__ import annotations

import json

import numpy as np
import torch

from ..parallel import dist as pdist
from . import functional as Fn
from . import prims as P

MODES = ("ce", "bce")
MAX_BINS = 64  # JM_EVAL_MAX_BINS
MATRIX_MAX_L = 4096  # JM_EVAL_MATRIX_MAX_L: the [L, L] matrix is kept up to here (134 MB)
Q_ONE = 1 << 32
TOP_PAIRS = 20


def layout(L: int, n_bins: int) -> dict:
    """``{view: (offset, shape)}`` of the flat int64 state, and its length under ``"words"`` (jm_api.h)."""
    if L < 1 or not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"eval report: labels {L}, bins {n_bins}: expected labels >= 1 and 1 <= bins <= {MAX_BINS}")
    lay, off = {}, 0
    for name, shape in (("rows", ()), ("nonfinite", ()), ("padded", ()), ("bins", (n_bins, 3)), ("count", (L,)),
                        ("hit1", (L,)), ("hit5", (L,)), ("predicted", (L,))) + \
            ((("confusion", (L, L)),) if L <= MATRIX_MAX_L else ()):
        lay[name] = (off, shape)
        off += int(np.prod(shape, dtype=np.int64))
    lay["words"] = off
    return lay


def views(state: torch.Tensor, L: int, n_bins: int) -> dict:
    """Named views into ``state`` (no copies)."""
    lay = layout(L, n_bins)
    assert state.dtype == torch.int64 and state.shape == (lay["words"],)
    names = [k for k in lay if k != "words"]
    return {k: state[lay[k][0]:lay[k][0] + int(np.prod(lay[k][1], dtype=np.int64))].view(lay[k][1]) for k in names}


# ------------------------------------------------------------------------------------ definition
def eval_rows_torch(logits: torch.Tensor, labels: torch.Tensor, mode: str = "ce", dtype=torch.float64,
                    round_conf: bool = True):
    """(pred int32 [B], rank int32 [B], conf [B]) as the module docstring defines them, evaluated in
    ``dtype``.  fp64 with ``round_conf`` is the definition (conf fp32); fp64 without it is the unrounded
    value the kernels are tested against; fp32 is the composition whose error sets their bound."""
    if mode not in MODES:
        raise KeyError(mode)
    B, L = logits.shape
    z = logits.detach().to(dtype)
    y = labels.long()
    padded = y == -1
    a = y.clamp(0, L - 1)
    bad = padded | torch.isnan(z).any(-1) | ~torch.isfinite(z.max(-1).values)
    z = torch.where(bad.unsqueeze(-1), torch.zeros_like(z), z)
    pred = Fn.argmax_first(z)
    za = z.gather(1, a.view(-1, 1))
    idx = torch.arange(L, device=z.device).expand(B, L)
    rank = ((z > za) | ((z == za) & (idx < a.view(-1, 1)))).sum(-1)
    m = z.max(-1, keepdim=True).values
    if mode == "ce":
        conf = 1.0 / torch.exp(z - m).sum(-1)
    else:
        conf = torch.sigmoid(m.squeeze(-1))
    neg = torch.full_like(pred, -1)
    conf = torch.where(bad, torch.zeros_like(conf), conf)
    return (torch.where(bad, neg, pred).int(), torch.where(bad, neg, rank).int(), conf.float() if round_conf else conf)


def row_terms(labels, pred, rank, conf, L: int, n_bins: int):
    """What a row adds, as the accumulation reads the per-row outputs: (padded, finite, a, hit1, hit5, q, bin).
    A row whose ``pred`` is outside [0, L) is non-finite; a confidence outside [0, 1] (never produced by
    ``eval_rows``) counts as 0."""
    y = labels.long()
    padded = y == -1
    a = y.clamp(0, L - 1)
    p = pred.long()
    finite = ~padded & (p >= 0) & (p < L)
    rk = rank.long()
    c = conf.float()
    c = torch.where((c >= 0) & (c <= 1), c, torch.zeros_like(c)).double()
    q = (c * float(Q_ONE)).round().long()
    b = torch.floor(c * n_bins).long().clamp(max=n_bins - 1)
    return padded, finite, a, rk == 0, (rk >= 0) & (rk < min(5, L)), q, b


def eval_accumulate_torch(labels, pred, rank, conf, L: int, n_bins: int, state: torch.Tensor) -> torch.Tensor:
    """``state`` (flat int64, ``layout``) += the batch, in place."""
    v = views(state, L, n_bins)
    padded, finite, a, h1, h5, q, b = row_terms(labels, pred, rank, conf, L, n_bins)
    v["rows"] += finite.sum()
    v["padded"] += padded.sum()
    v["nonfinite"] += (~finite & ~padded).sum()
    a, p, h1, h5, q, b = (t[finite] for t in (a, pred.long(), h1.long(), h5.long(), q, b))
    one = torch.ones_like(a)
    bins = v["bins"]
    bins[:, 0].index_add_(0, b, one)
    bins[:, 1].index_add_(0, b, h1)
    bins[:, 2].index_add_(0, b, q)
    v["count"].index_add_(0, a, one)
    v["hit1"].index_add_(0, a, h1)
    v["hit5"].index_add_(0, a, h5)
    v["predicted"].index_add_(0, p, one)
    if "confusion" in v:
        v["confusion"].view(-1).index_add_(0, a * L + p, one)
    return state


# ------------------------------------------------------------------------------------ dispatch
def eval_rows(logits: torch.Tensor, labels: torch.Tensor, mode: str = "ce"):
    """(pred int32, rank int32, conf fp32), [B] each.  On the GPU one kernel (a strided row view is taken
    without a copy, as in ``Fn.kd_loss``); on the CPU, or with ``prims._EVAL_REPORT_OURS`` off, the fp64
    torch composition."""
    if mode not in MODES:
        raise KeyError(mode)
    if logits.dtype not in (torch.bfloat16, torch.float32):
        logits = logits.float()
    if not (P._EVAL_REPORT_OURS and P.hip(logits)):
        return eval_rows_torch(logits, labels, mode)
    z = logits.detach()
    z = z if Fn._rows_ok(z) else z.contiguous()
    return tuple(P._ext.load().eval_rows(z, labels.long().contiguous(), MODES.index(mode)))


def eval_accumulate(labels, pred, rank, conf, L: int, n_bins: int, state: torch.Tensor) -> torch.Tensor:
    """``state`` += the batch: one kernel without atomics on the GPU, else ``eval_accumulate_torch``."""
    if not (P._EVAL_REPORT_OURS and P.hip(state)):
        return eval_accumulate_torch(labels, pred, rank, conf, L, n_bins, state)
    P._ext.load().eval_accumulate(labels.long().contiguous(), pred.contiguous(), rank.contiguous(),
                                  conf.contiguous(), L, n_bins, state)
    return state


# ------------------------------------------------------------------------------------ the report
class EvalReport:
    """One evaluation's report: ``update`` per batch, ``all_reduce`` once, then ``summary`` / ``to_json`` /
    ``confusion``."""

    def __init__(self, labels: int, n_bins: int = 15, mode: str = "ce", device="cpu"):
        if mode not in MODES:
            raise KeyError(mode)
        self.labels, self.n_bins, self.mode = int(labels), int(n_bins), mode
        self.state = torch.zeros(layout(self.labels, self.n_bins)["words"], dtype=torch.int64, device=device)
        self.v = views(self.state, self.labels, self.n_bins)

    @torch.no_grad()
    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        if logits.dim() != 2 or logits.shape[1] != self.labels or labels.shape != logits.shape[:1]:
            raise ValueError(f"eval report: logits {tuple(logits.shape)} / labels {tuple(labels.shape)} for "
                             f"{self.labels} classes")
        if logits.shape[0] == 0:
            return
        pred, rank, conf = eval_rows(logits, labels, self.mode)
        eval_accumulate(labels, pred, rank, conf, self.labels, self.n_bins, self.state)

    def all_reduce(self, group=None) -> None:
        """One int64 SUM over the process group; nothing at world size 1."""
        pdist.all_reduce_sum_(self.state, group)

    def confusion(self):
        """int64 [L, L] numpy array, true x predicted; ``None`` above ``MATRIX_MAX_L`` classes."""
        return self.v["confusion"].cpu().numpy() if "confusion" in self.v else None

    def _host(self) -> dict:
        return {k: self.v[k].cpu().numpy() for k in self.v if k != "confusion"}

    @staticmethod
    def _metrics(h: dict) -> dict:
        """fp64 on the host, from the integers."""
        n = int(h["rows"])
        cnt = h["count"].astype(np.float64)
        seen = h["count"] > 0
        acc1 = h["hit1"][seen] / cnt[seen]
        acc5 = h["hit5"][seen] / cnt[seen]
        nb, hb, qb = (h["bins"][:, i] for i in range(3))
        full = nb > 0
        acc_b = hb[full] / nb[full].astype(np.float64)
        conf_b = qb[full] / (float(Q_ONE) * nb[full].astype(np.float64))
        gap = np.abs(acc_b - conf_b)
        worst = int(np.flatnonzero(seen)[np.argmin(acc1)]) if seen.any() else -1  # argmin: the first minimum
        return {"mean_class_acc1": float(acc1.mean()) if seen.any() else 0.0,
                "mean_class_acc5": float(acc5.mean()) if seen.any() else 0.0,
                "worst_class_acc1": float(acc1.min()) if seen.any() else 0.0,
                "ece": float((nb[full] / float(n) * gap).sum()) if n else 0.0,
                "mce": float(gap.max()) if n else 0.0,
                "mean_conf": float(int(qb.sum()) / (float(Q_ONE) * n)) if n else 0.0,
                "classes_seen": float(seen.sum()), "nonfinite_rows": float(int(h["nonfinite"])),
                "_worst_class": worst}

    def summary(self, prefix: str = "val/") -> dict:
        """``{prefix}mean_class_acc1``, ``mean_class_acc5``, ``worst_class_acc1``, ``ece``, ``mce``,
        ``mean_conf``, ``classes_seen``, ``nonfinite_rows``."""
        return {prefix + k: v for k, v in self._metrics(self._host()).items() if not k.startswith("_")}

    def to_json(self, step: int | None = None, prefix: str = "val/") -> dict:
        """The report as plain Python: counts, metrics, bins, per-class rows and the ``TOP_PAIRS`` largest
        off-diagonal cells (count descending, then true ascending, then pred ascending)."""
        h = self._host()
        m = self._metrics(h)
        L, nb = self.labels, self.n_bins
        cm = self.confusion()
        out = {"step": step, "labels": L, "mode": self.mode, "rows": int(h["rows"]), "padded": int(h["padded"]),
               "nonfinite": int(h["nonfinite"]), "worst_class": m.pop("_worst_class"),
               "metrics": {prefix + k: v for k, v in m.items()}, "bins": [], "per_class": [], "confused_pairs": []}
        for b in range(nb):
            n, hit, q = (int(x) for x in h["bins"][b])
            out["bins"].append({"lo": b / nb, "hi": (b + 1) / nb, "count": n, "acc": hit / n if n else None,
                                "conf": q / (float(Q_ONE) * n) if n else None})
        off = None
        if cm is not None:
            off = cm.copy()
            np.fill_diagonal(off, 0)
            wrong, wrong_n = off.argmax(1), off.max(1)  # argmax: the lowest class among equal counts
        for c in range(L):
            n = int(h["count"][c])
            row = {"id": c, "count": n, "acc1": int(h["hit1"][c]) / n if n else None,
                   "acc5": int(h["hit5"][c]) / n if n else None, "predicted": int(h["predicted"][c]),
                   "top_confusion": None}
            if off is not None and wrong_n[c] > 0:
                row["top_confusion"] = {"pred": int(wrong[c]), "count": int(wrong_n[c])}
            out["per_class"].append(row)
        if off is not None:
            t, p = np.nonzero(off)
            order = np.lexsort((p, t, -off[t, p]))[:TOP_PAIRS]
            out["confused_pairs"] = [{"true": int(t[i]), "pred": int(p[i]), "count": int(off[t[i], p[i]])}
                                     for i in order]
        return out

    def dumps(self, step: int | None = None, prefix: str = "val/") -> str:
        return json.dumps(self.to_json(step, prefix), indent=1)
