"""Cross-replica BatchNorm for the linear-probe head.

Reference: ``nn.BatchNorm(use_running_average=det, axis_name="batch")`` inside ``LinearCLS``
(/root/reference/src/modeling.py:216-217).  Flax semantics: batch statistics
are ``pmean`` of per-device ``mean(x)`` and ``mean(x^2)``, ``var = max(0, mean2 - mean^2)``
(biased), eps 1e-5, running stats updated with momentum 0.99 (``ra = m*ra + (1-m)*stat``).
One packed all-reduce of ``[sum x, sum x^2]`` (2*J floats) in forward and one of
``[sum g, sum g*xhat]`` in backward.

On the GPU (``ops.prims._BN_OURS``) the arithmetic runs on the kernels of csrc/batchnorm.hip
(``_SyncBNFused``): statistics, normalisation straight into the compute dtype, running-statistics
update, and a backward that rebuilds ``xhat`` from ``x``; the two packed all-reduces stay the torch
calls they are here, on the same fp32 ``[2 J]`` tensors.  The CPU, and the switch off, keep the torch
composition below.
"""

from __future__ import annotations

import torch
import torch.distributed as dist

from ..models.params import Handle


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


class _SyncBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sp, bp, hs: Handle, hb: Handle, eps: float, group, stats_out):
        n_local = x.shape[0]
        world = _world(group)
        packed = torch.cat([x.sum(0), (x * x).sum(0)]) / n_local
        if world > 1:
            dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
            packed /= world
        mean, mean2 = packed.chunk(2)
        var = torch.clamp(mean2 - mean * mean, min=0.0)
        rstd = torch.rsqrt(var + eps)
        xhat = (x - mean) * rstd
        y = xhat * hs.master + hb.master
        ctx.save_for_backward(xhat, rstd)
        ctx.hs, ctx.hb, ctx.group, ctx.world, ctx.n = hs, hb, group, world, n_local
        stats_out.append((mean, var))
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd = ctx.saved_tensors
        hs, hb = ctx.hs, ctx.hb
        if hs.segs[0].trainable:
            hs.grad.add_((dy * xhat).sum(0))
            hb.grad.add_(dy.sum(0))
            hs.ready()
            hb.ready()
        dx = None
        if ctx.needs_input_grad[0]:
            g = dy * hs.master
            packed = torch.cat([g.sum(0), (g * xhat).sum(0)])
            if ctx.world > 1:
                dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=ctx.group)
            n = ctx.n * ctx.world
            sg, sgx = packed.chunk(2)
            dx = rstd * (g - sg / n - xhat * sgx / n)
        return dx, None, None, None, None, None, None, None


@torch.no_grad()
def _update_running(running_mean, running_var, mean, var, momentum):
    running_mean.mul_(momentum).add_((1 - momentum) * mean)
    running_var.mul_(momentum).add_((1 - momentum) * var)


class _SyncBNFused(torch.autograd.Function):
    """The same op on csrc/batchnorm.hip.  Saves ``x`` and the fp32 ``[2, J]`` (mean, rstd); ``y`` comes
    back in ``out_dtype``; the running statistics move inside the forward kernel."""

    @staticmethod
    def forward(ctx, x, sp, bp, hs: Handle, hb: Handle, running_mean, running_var, eps: float, momentum: float,
                group, out_dtype):
        from ..ops import _ext
        ext = _ext.load()
        world = _world(group)
        packed = ext.bn_stats(x)
        if world > 1:
            dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
            packed /= world
        y, stats = ext.bn_apply(x, packed, hs.master, hb.master, running_mean, running_var, eps, momentum, out_dtype)
        ctx.save_for_backward(x, stats)
        ctx.hs, ctx.hb, ctx.group, ctx.world, ctx.n = hs, hb, group, world, x.shape[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        from ..ops import _ext
        ext = _ext.load()
        x, stats = ctx.saved_tensors
        hs, hb = ctx.hs, ctx.hb
        trainable, need_dx = hs.segs[0].trainable, ctx.needs_input_grad[0]
        dx = None
        if trainable or need_dx:
            if dy.dtype not in (torch.bfloat16, torch.float32):
                dy = dy.float()
            dy = _rows(dy)
            if trainable:
                packed = ext.bn_bwd_reduce(dy, x, stats, hs.master, hs.grad, hb.grad)[2]
                hs.ready()
                hb.ready()
            else:
                packed = ext.bn_bwd_reduce(dy, x, stats, hs.master)[2]
            if need_dx:
                if ctx.world > 1:
                    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=ctx.group)
                dx = ext.bn_bwd_dx(dy, x, stats, hs.master, packed, float(ctx.n * ctx.world))
        return (dx,) + (None,) * 10


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` as the kernels take it: unit column stride, rows that do not overlap (else a copy)."""
    if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def _fused(x: torch.Tensor) -> bool:
    from ..ops import prims as P
    return P._BN_OURS and x.dim() == 2 and P.hip(x)


def sync_batch_norm(x: torch.Tensor, hs: Handle, hb: Handle, running_mean: torch.Tensor,
                    running_var: torch.Tensor, training: bool, momentum: float = 0.99, eps: float = 1e-5,
                    group=None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """fp32 result; on the fused GPU path the result comes back in ``out_dtype`` (bf16 or fp32) when given."""
    x = x.float()
    if _fused(x):
        odt = out_dtype if out_dtype in (torch.bfloat16, torch.float32) else torch.float32
        if not training:
            if not (torch.is_grad_enabled() and x.requires_grad):
                from ..ops import _ext
                return _ext.load().bn_apply_eval(_rows(x), running_mean, running_var, hs.master, hb.master, eps, odt)
        else:
            hs.note_use()
            hb.note_use()
            return _SyncBNFused.apply(_rows(x), hs.param, hb.param, hs, hb, running_mean, running_var, eps, momentum,
                                      group, odt)
    if not training:
        return (x - running_mean) * torch.rsqrt(running_var + eps) * hs.master + hb.master
    hs.note_use()
    hb.note_use()
    stats: list = []
    y = _SyncBN.apply(x, hs.param, hb.param, hs, hb, eps, group, stats)
    mean, var = stats[0]
    _update_running(running_mean, running_var, mean, var, momentum)
    return y
