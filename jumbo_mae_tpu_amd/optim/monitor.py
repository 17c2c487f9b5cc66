"""Norm monitor: per-leaf gradient / weight / update statistics of one optimizer step, from one pass.

``seg_stats`` returns a float64 ``[segments, 7]`` tensor over the elements a chunk table covers
(``optim/flat.py``: rows ``[start, length, segment]``, sorted by segment), one row per Flax leaf:

    col 0  G2    sum of g^2 over finite g
    col 1  P2    sum of p^2 over finite p
    col 2  D2    sum of (p - p_old)^2 where both are finite; 0 without p_old
    col 3  GMAX  max |g| over finite g (0 if none)
    col 4  GBAD  number of non-finite g
    col 5  PBAD  number of non-finite p
    col 6  N     covered elements

Every fp32 value is widened to float64 before it is squared or subtracted.  A non-finite value is
counted and adds nothing to any sum.  For a frozen segment (``meta[seg][3] == 0``) columns 0, 2, 3 and 4
are 0 and ``g`` / ``p_old`` are not read: the model never writes a frozen gradient.  A segment without a
row gets zeros.  On the GPU this is ``csrc/optim.hip`` ``seg_stats_kernel`` (one workgroup per row, 7
partials) and ``seg_stats_finish_kernel`` (per segment, in chunk order with a fixed tree): no atomics, the
same bits on every run.  ``seg_stats_torch`` is the same definition as a float64 torch composition: the
CPU path, the ``ops/prims.py _NORMS_OURS = False`` path and the kernels' oracle.

``NormMonitor(opt, level)`` wraps it for the drivers (``--log-norms global|layer``): ``begin()`` before a
step that will be logged copies ``store.master`` into a flat fp32 snapshot (allocated on first use, the
size of the store); ``collect()`` after the step runs the pass on the updated master, the step's gradient
(reduced, accumulated, unclipped: it stays in ``store.grad`` until the next ``zero_grad``) and the
snapshot; ``summary(stats)`` copies the table to the host once and returns Python floats.  Both calls
run outside ``Trainer.device_step``: unlogged steps cost nothing and a captured HIP graph holds no new
node.  Under ZeRO-1 each rank visits its owned rows and ``collect()`` is COLLECTIVE (one fp64 SUM
all-reduce of the sums and counts, one MAX all-reduce of GMAX); frozen segments belong to no rank's
pieces there and report zeros.  Without sharding every rank holds the same values and nothing is
exchanged.  Nothing here writes to the store, the optimizer state or a random stream.
"""

from __future__ import annotations

import math

import torch

from ..ops import _ext

COLS = ("G2", "P2", "D2", "GMAX", "GBAD", "PBAD", "N")
NCOL = len(COLS)
SUM_COLS = (0, 1, 2, 4, 5, 6)
LEVELS = ("global", "layer")
MAX_BAD_LINES = 8


def row_elements(rows: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(flat index, segment) of every element the chunk table covers, int64, in table order."""
    r = rows.to(torch.int64)
    start, length, seg = r[:, 0], r[:, 1], r[:, 2]
    first = torch.cumsum(length, 0) - length  # position of each row's first element in the output
    pos = torch.arange(int(length.sum()), device=r.device)
    return (start - first).repeat_interleave(length) + pos, seg.repeat_interleave(length)


@torch.no_grad()
def seg_stats_torch(p, g, p_old, rows, meta, nseg: int, elements=None) -> torch.Tensor:
    """The definition above as a float64 torch composition on the device of ``p``.  ``elements``: a
    cached ``row_elements(rows)``."""
    dev = p.device
    out = torch.zeros(nseg, NCOL, dtype=torch.float64, device=dev)
    if rows is None or rows.numel() == 0:
        return out
    idx, seg = elements if elements is not None else row_elements(rows.to(dev))
    live = (meta.to(dev)[:, 3] != 0)[seg]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    pv = p[idx]
    pf = torch.isfinite(pv)
    pd = torch.where(pf, pv.double(), zero)
    gv = torch.where(live, g[idx], torch.zeros((), dtype=g.dtype, device=dev))  # a frozen gradient is not looked at
    gf = torch.isfinite(gv)
    gd = torch.where(gf, gv.double(), zero)
    out[:, 0].index_add_(0, seg, gd * gd)
    out[:, 1].index_add_(0, seg, pd * pd)
    if p_old is not None:
        ov = p_old[idx]
        both = live & pf & torch.isfinite(ov)
        d = torch.where(both, pd - torch.where(both, ov.double(), zero), zero)
        out[:, 2].index_add_(0, seg, d * d)
    out[:, 3] = torch.zeros(nseg, dtype=torch.float64, device=dev).scatter_reduce(0, seg, gd.abs(), "amax")
    out[:, 4].index_add_(0, seg, (live & ~gf).double())
    out[:, 5].index_add_(0, seg, (~pf).double())
    out[:, 6].index_add_(0, seg, torch.ones_like(pd))
    return out


def seg_stats(p, g, p_old, rows, meta, out=None, elements=None) -> torch.Tensor:
    """The HIP pass for flat fp32 GPU buffers, ``seg_stats_torch`` elsewhere."""
    from ..ops import prims as P
    if P._NORMS_OURS and p.is_cuda and _ext.use_hip(p):
        return _ext.load().opt_seg_stats(p, g, p_old, rows, meta, out)
    res = seg_stats_torch(p, g, p_old, rows, meta, meta.shape[0], elements)
    if out is not None:
        out.copy_(res)
        return out
    return res


def group_name(path: tuple[str, ...]) -> str:
    """The log group of a leaf: the leaves sharing a path prefix -- ``embed``, ``cls_tokens``,
    ``jumbo_mlp``, ``layer_<i>``, ``norm``, ``head`` (the ``model`` subtree), ``decoder/<name>`` (the
    ``decoder_model`` subtree: ``dec_layer_<i>``, ``dec_norm``, ...) and the top-level leaves'
    own names (``image_mask_embedding``, ``decoder_proj``, ``decoder_image_output``)."""
    if path[0] == "model" and len(path) > 1:
        return path[1]
    if path[0] == "decoder_model" and len(path) > 1:
        return "decoder/" + path[1]
    return path[0]


class NormMonitor:
    def __init__(self, opt, level: str = "global"):
        if level not in LEVELS:
            raise ValueError(f"norm monitor level {level!r}: expected one of {LEVELS}")
        self.opt, self.store, self.level = opt, opt.store, level
        self.groups: list[str] = []
        gid = []
        for s in self.store.segments:
            name = group_name(s.path)
            if name not in self.groups:
                self.groups.append(name)
            gid.append(self.groups.index(name))
        self.group_of = torch.tensor(gid, dtype=torch.int64)
        self.snapshot: torch.Tensor | None = None
        self._armed = False       # begin() ran for the step being collected
        self._elements = None     # (rows, row_elements(rows)) of the torch path
        self._empty_rows = None
        self.last: torch.Tensor | None = None  # host copy of the last summarised table

    # ---------------------------------------------------------------- the logged step
    @torch.no_grad()
    def begin(self) -> None:
        """Before a step that will be logged: keep the weights it starts from."""
        m = self.store.master
        if self.snapshot is None:
            self.snapshot = torch.empty_like(m)
        self.snapshot.copy_(m)
        self._armed = True

    def _rows(self) -> torch.Tensor:
        opt = self.opt
        rows = opt.chunks if opt._shard is None else opt._owned_rows
        if rows is None:  # a rank that owns nothing
            if self._empty_rows is None:
                self._empty_rows = torch.zeros(0, 3, dtype=torch.int32, device=self.store.master.device)
            rows = self._empty_rows
        return rows

    @torch.no_grad()
    def collect(self) -> torch.Tensor:
        """After that step: the float64 ``[segments, 7]`` table, on the device.  COLLECTIVE under ZeRO-1
        (every rank, on the same steps).  Without a ``begin()`` for this step D2 is 0."""
        s, opt = self.store, self.opt
        rows = self._rows()
        old = self.snapshot if self._armed else None
        self._armed = False
        from ..ops import prims as P
        elements = None
        if not (P._NORMS_OURS and s.master.is_cuda and _ext.use_hip(s.master)) and rows.numel() > 0:
            if self._elements is None or self._elements[0] is not rows:
                self._elements = (rows, row_elements(rows))
            elements = self._elements[1]
        stats = seg_stats(s.master, s.grad, old, rows, opt.meta, elements=elements)
        red = opt._shard
        if red is not None:
            import torch.distributed as dist
            sums = stats[:, list(SUM_COLS)].contiguous()
            gmax = stats[:, 3].contiguous()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=red.group)
            dist.all_reduce(gmax, op=dist.ReduceOp.MAX, group=red.group)
            stats[:, list(SUM_COLS)] = sums
            stats[:, 3] = gmax
        return stats

    # ---------------------------------------------------------------- host side
    def summary(self, stats: torch.Tensor) -> dict[str, float]:
        """One device-to-host copy; the log keys of the level as Python floats."""
        t = stats.detach().to("cpu", torch.float64)
        self.last = t
        tot = t.sum(0)
        g2, p2, d2 = float(tot[0]), float(tot[1]), float(tot[2])
        gn = math.sqrt(g2)
        out = {"train/grad_norm": gn, "train/param_norm": math.sqrt(p2), "train/update_norm": math.sqrt(d2),
               "train/update_ratio": math.sqrt(d2 / p2) if p2 > 0 else 0.0,
               "train/grad_absmax": float(t[:, 3].max()) if t.shape[0] else 0.0,
               "train/nonfinite_grads": float(tot[4]), "train/nonfinite_params": float(tot[5])}
        c = float(getattr(self.opt, "clip_grad", 0.0) or 0.0)
        if c > 0:
            out["train/clip_scale"] = min(1.0, c / gn) if gn > 0 else 1.0
        if self.level == "layer":
            per = torch.zeros(len(self.groups), 3, dtype=torch.float64).index_add_(0, self.group_of, t[:, :3])
            for name, (a, b, d) in zip(self.groups, per.tolist()):
                out[f"norms/grad/{name}"] = math.sqrt(a)
                out[f"norms/param/{name}"] = math.sqrt(b)
                out[f"norms/update_ratio/{name}"] = math.sqrt(d / b) if b > 0 else 0.0
        return out

    def bad_leaves(self, limit: int = MAX_BAD_LINES) -> list[str]:
        """Up to ``limit`` lines ``leaf/path: G non-finite grads, P non-finite params of N`` for the leaves
        of the last summarised table that hold a non-finite value, in store order."""
        if self.last is None:
            return []
        lines = []
        for s, row in zip(self.store.segments, self.last.tolist()):
            if row[4] > 0 or row[5] > 0:
                lines.append(f"{s.key}: {int(row[4])} non-finite grads, {int(row[5])} non-finite params of {int(row[6])}")
                if len(lines) >= limit:
                    break
        return lines


def make_monitor(args, opt) -> NormMonitor | None:
    """--log-norms global | layer: the monitor of a driver; None with the flag off."""
    level = getattr(args, "log_norms", "off") or "off"
    return None if level == "off" else NormMonitor(opt, level)


def log_norms(monitor: NormMonitor, summ: dict, log=print) -> None:
    """A driver's logged step: the step's statistics into ``summ`` (COLLECTIVE under ZeRO-1) and, when
    something is not finite, the leaves that hold it (``log``: rank 0's print)."""
    summ.update(monitor.summary(monitor.collect()))
    if summ["train/nonfinite_grads"] > 0 or summ["train/nonfinite_params"] > 0:
        for line in monitor.bad_leaves():
            log(line)
