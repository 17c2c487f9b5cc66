"""float64 oracle of the weight EMA (tests/test_ema.py, tests/test_ema_gpu.py).

Restates the definition without importing ``jumbo_mae_tpu_amd.optim.ema``:

    d_t   = min(decay, (1 + t) / (10 + t))            decay of update t = 0, 1, ...
    omd_t = float32(1 - d_t)                          the factor every implementation multiplies by
    e    <- e + omd_t (p - e)                         on the covered elements of trainable segments

The recurrence runs in float64 over the fp32 inputs an implementation gets.  ``bound`` is the fp32 error
one update may add: at most three roundings -- the subtraction, the product, the sum; a contracted FMA
only removes one -- each at most u = 2^-24 relative to a quantity no larger than |omd (p - e)| + |e|,
plus 2^-126 for a result in the subnormal range.
"""

from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24


def decay_at(decay: float, t: int) -> float:
    return min(float(decay), (1.0 + t) / (10.0 + t))


def omd_at(decay: float, t: int) -> float:
    return float(np.float32(1.0 - decay_at(decay, t)))


def _d(t) -> torch.Tensor:
    return t.detach().cpu().to(F64)


def step(e, p, omd: float, live) -> tuple[torch.Tensor, torch.Tensor]:
    """(new e, bound) in float64: one update of ``e`` (any float dtype) towards fp32 ``p`` where the
    bool mask ``live`` is set; elsewhere e stays and the bound is 0."""
    E, P = _d(e), _d(p)
    inc = omd * (P - E)
    live = live.cpu()
    new = torch.where(live, E + inc, E)
    bnd = torch.where(live, 3 * U * (inc.abs() + E.abs()) + 2.0 ** -126, torch.zeros_like(E))
    return new, bnd


def run(e0, masters, decay: float, live, t0: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """The recurrence over the fp32 snapshots ``masters`` (updates t0, t0 + 1, ...) from ``e0``:
    (e, accumulated bound).  An error already in e is carried on by at most a factor 1, so the
    bounds of the updates add."""
    e, tot = _d(e0), torch.zeros(e0.numel(), dtype=F64)
    for k, p in enumerate(masters):
        e, b = step(e, p, omd_at(decay, t0 + k), live)
        tot = tot + b
    return e, tot


def bits(t: torch.Tensor) -> torch.Tensor:
    """The words of an fp32 / bf16 tensor as integers on the CPU (NaNs compare by their bits)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
