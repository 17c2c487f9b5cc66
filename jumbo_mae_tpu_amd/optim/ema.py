"""Exponential moving average of the weights over the flat parameter store.

``WeightEma(store, decay)`` keeps ``ema``, a flat fp32 buffer laid out like ``store.master``, created
as a copy of it.  Attached to the optimizer (``FlatOptimizer.attach_ema``) it follows every parameter
update, on exactly the rows that update touched:

    e <- e + omd_t (p - e),   omd_t = float32(1 - d_t),   d_t = min(decay, (1 + t) / (10 + t))

for update t = 0, 1, ... (``updates`` counts them; the warm-up of d_t is timm's / TF's).  All math is
fp32; an update whose increment is zero (p == e, omd == 0) keeps the bits of e.  Segments that are not
trainable are never touched: their average stays the copy of the master it started as.  On the GPU
the update is ``csrc/optim.hip`` ``ema_kernel``, with omd_t read from the step feeder's static
``"ema_hyper"`` buffer, so a HIP-graph step carries it; elsewhere the same formula runs in torch.

``with ema.swapped():`` evaluates or exports the averaged weights without a second store or model:
the ``ema_swap`` kernel exchanges ``master`` and ``ema`` in place, bit for bit, and rewrites the bf16
shadow; every handle is a view of the store, so every kernel then reads the average.  Leaving the block
exchanges them back.  With the ZeRO-1 sharded optimizer each rank averages its owned pieces only and
``gather()`` (collective) makes ``ema`` and the master whole first.

BatchNorm running statistics (linear-probe head) are not averaged.
"""

from __future__ import annotations

import contextlib

import numpy as np
import torch

from ..models.params import ParamStore
from ..ops import _ext


def decay_at(decay: float, t: int) -> float:
    """d_t of update t (0-based)."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def omd_at(decay: float, t: int) -> float:
    """float32(1 - d_t) as a Python float: the factor every path multiplies by."""
    return float(np.float32(1.0 - decay_at(decay, t)))


class WeightEma:
    def __init__(self, store: ParamStore, decay: float):
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"EMA decay {decay}: expected 0 <= decay < 1")
        self.store, self.decay = store, float(decay)
        self.ema = store.master.detach().clone()
        self.updates = 0
        self.omd = omd_at(self.decay, 0)  # of the update being prepared
        self.hyper: torch.Tensor | None = None  # the feeder's device buffer (GPU)
        self.opt = None  # FlatOptimizer this average follows (attach_ema)
        self._all_rows = None

    def _hip(self) -> bool:
        m = self.store.master
        return m.is_cuda and _ext.use_hip(m)

    # ---------------------------------------------------------------- the step (called by FlatOptimizer)
    def prepare(self) -> None:
        self.omd = omd_at(self.decay, self.updates)
        if self._hip():
            from ..runtime.feeder import feeder
            self.hyper = feeder(self.store.master.device).put("ema_hyper", [self.omd])

    def update_rows(self, rows: torch.Tensor, meta: torch.Tensor) -> None:
        """GPU: the update on chunk-table ``rows`` (trainable segments by ``meta[:, 3]``)."""
        _ext.load().opt_ema(self.store.master, self.ema, rows, meta, self.hyper)

    @torch.no_grad()
    def update_torch(self, mask: torch.Tensor, sl: slice = slice(None)) -> None:
        """Torch path: the update on the elements of ``master[sl]`` where ``mask`` is set."""
        p, e = self.store.master[sl], self.ema[sl]
        t = (p - e) * self.omd
        e.copy_(torch.where(mask & (t != 0), e + t, e))

    def finish(self) -> None:
        self.updates += 1

    # ---------------------------------------------------------------- evaluation / export
    def gather(self) -> None:
        """COLLECTIVE under ZeRO-1 (every rank, same step): ``ema`` -- and the fp32 master, when the
        steps gather only the bf16 shadow -- made whole on every rank.  No-op without sharding."""
        red = getattr(self.opt, "_shard", None)
        if red is not None:
            red.gather_state([self.ema])

    def _rows(self) -> torch.Tensor:
        if self.opt is not None:
            return self.opt.chunks
        if self._all_rows is None:
            from .flat import CHUNK
            rows = [(s.offset + st, min(CHUNK, s.numel - st), i) for i, s in enumerate(self.store.segments)
                    for st in range(0, s.numel, CHUNK)]
            self._all_rows = torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(self.store.master.device)
        return self._all_rows

    @torch.no_grad()
    def swap(self) -> None:
        """Exchange ``master`` and ``ema`` on every segment and re-cast the shadow."""
        s = self.store
        if self._hip():
            _ext.load().ema_swap(s.master, self.ema, s.shadow if s.shadow is not s.master else None, self._rows())
        else:
            for sg in s.segments:
                sl = slice(sg.offset, sg.offset + sg.numel)
                tmp = s.master[sl].clone()
                s.master[sl].copy_(self.ema[sl])
                self.ema[sl].copy_(tmp)
                if s.shadow is not s.master:
                    s.shadow[sl].copy_(s.master[sl])
        s.version += 1  # shadow rewritten: transposed weight copies are stale

    @contextlib.contextmanager
    def swapped(self):
        """The store holds the averaged weights inside the block (COLLECTIVE under ZeRO-1)."""
        self.gather()
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---------------------------------------------------------------- state io
    def state_dict(self) -> dict:
        return {"ema": self.ema.detach().cpu(), "updates": self.updates, "decay": self.decay}

    def load_state_dict(self, d: dict) -> None:
        src = d["ema"].reshape(-1).to(torch.float32)
        dst = self.ema
        # the optimizer moments' rule (FlatOptimizer.load_state_dict): segment offsets do not depend
        # on the padding of the flat total; copy the common prefix, the rest is padding
        n = min(src.numel(), dst.numel())
        if src.numel() > n and bool(src[n:].any()):
            raise ValueError(f"EMA state has {src.numel()} elements with non-zero entries past this store's "
                             f"{dst.numel()}")
        if n < self.store.used_numel():
            raise ValueError(f"EMA state has {src.numel()} elements; the parameters span {self.store.used_numel()}")
        dst[:n].copy_(src[:n])
        dst[n:].zero_()
        self.updates = int(d["updates"])
