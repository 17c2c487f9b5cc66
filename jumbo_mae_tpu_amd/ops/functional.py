"""Per-op autograd wrappers of the hot-path primitives (ops/prims.py).

Used for the parts of the model that are not fused transformer blocks (patch embedding,
decoder projection / prediction head, final norms, the finetune head) and as the generic path
for configurations the fused blocks do not cover (dropout > 0).  Parameter gradients never travel
through autograd: each op accumulates them straight into the flat fp32 gradient buffer of the
``ParamStore`` and signals the data-parallel reducer; parameters are passed as autograd inputs
only so that the graph records the ops that own them.

Reference semantics (file:line in /root/reference/src):
  Dense/DenseGeneral + bias ........... modeling.py:30-31,127-148
  LayerNorm (eps 1e-6, Flax default) .. modeling.py:155-156,177-179,238,282
  gelu (tanh approximation) ........... modeling.py:148 (flax nn.gelu approximate=True)
  softmax attention, no mask .......... modeling.py:135-138
  droppath = per-sample Dropout ....... modeling.py:157,181-183 (broadcast_dims)
"""

from __future__ import annotations

import torch

from ..models.params import Handle
from . import prims as P
from .prims import LN_EPS, wgrad_split  # noqa: F401  (re-exported)


# ---------------------------------------------------------------------------------- linear
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wp, bp, hw: Handle, hb: Handle | None, gelu: bool):
        x2 = x.reshape(-1, x.shape[-1])
        if gelu:
            h, out = P.linear_gelu_fwd(x2, hw, hb)
            ctx.save_for_backward(x2, h)
        else:
            out = h = P.linear_fwd(x2, hw, hb)
            ctx.save_for_backward(x2)
        ctx.hw, ctx.hb, ctx.gelu = hw, hb, gelu
        ctx.xshape = x.shape
        ctx.x_requires_grad = x.requires_grad
        return out.reshape(*x.shape[:-1], out.shape[-1])

    @staticmethod
    def backward(ctx, dout):
        hw, hb = ctx.hw, ctx.hb
        dout = dout.reshape(-1, dout.shape[-1]).contiguous()
        bias_done = False
        if ctx.gelu:
            x2, h = ctx.saved_tensors
            dy, bias_done = P.gelu_bwd(h, dout, hb if hw.segs[0].trainable else None)
        else:
            (x2,) = ctx.saved_tensors
            dy = dout
        dx = P.linear_bwd(dy, x2, hw, hb, need_dx=ctx.x_requires_grad, bias_done=bias_done)
        if dx is not None:
            dx = dx.reshape(ctx.xshape)
        return dx, None, None, None, None, None


def linear(x: torch.Tensor, hw: Handle, hb: Handle | None = None, gelu: bool = False) -> torch.Tensor:
    hw.note_use()
    if hb is not None:
        hb.note_use()
    return _Linear.apply(x, hw.param, hb.param if hb is not None else None, hw, hb, gelu)


def gelu_fwd(h: torch.Tensor) -> torch.Tensor:
    return P.gelu_fwd(h)


def gelu_bwd(h: torch.Tensor, da: torch.Tensor) -> torch.Tensor:
    return P.gelu_bwd(h, da)[0]


# ------------------------------------------------------------------------------- layernorm
class _LayerNorm(torch.autograd.Function):
    """x: fp32 [B, T, D] (any strides, last dim contiguous) -> y [B*(T-row0), D] in ``out_dtype``,
    the LayerNorm of rows t >= row0.  With row0 > 0 the gradient of the whole x is returned
    directly -- LN' written into rows >= row0 of a fresh tensor, zeros into the few rows below --
    instead of autograd's slice backward (a full-size zero fill plus a copy of the rows)."""

    @staticmethod
    def forward(ctx, x, gp, bp, hg: Handle, hb: Handle, out_dtype, row0=0):
        y, mean, rstd = P.ln_fwd(x[:, row0:] if row0 else x, hg, hb, out_dtype)
        ctx.save_for_backward(x, mean, rstd)
        ctx.hg, ctx.hb, ctx.row0 = hg, hb, row0
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        r0 = ctx.row0
        if not r0:
            return P.ln_bwd(dy, x, mean, rstd, ctx.hg, ctx.hb), None, None, None, None, None, None
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dx[:, :r0].zero_()
        P.ln_bwd(dy, x[:, r0:], mean, rstd, ctx.hg, ctx.hb, out=dx[:, r0:])
        return dx, None, None, None, None, None, None


def layer_norm(x: torch.Tensor, hg: Handle, hb: Handle, out_dtype=None, row0: int = 0) -> torch.Tensor:
    """LayerNorm of x (rows t >= ``row0`` of a [B, T, D] x only, when given)."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    out_dtype = out_dtype or hg.store.compute_dtype
    hg.note_use()
    hb.note_use()
    return _LayerNorm.apply(x, hg.param, hb.param, hg, hb, out_dtype, row0)


# -------------------------------------------------------------------------------- residual
class _Residual(torch.autograd.Function):
    """out[b,t,:] = x[b,t,:] + mask[b] * scale[:] * y[b*T+t, :]  (x fp32 view, out fp32 contiguous).

    ``mask`` is the per-sample droppath keep mask already divided by the keep probability
    (Flax ``Dropout(broadcast_dims=...)`` semantics), ``scale`` the LayerScale vector.
    """

    @staticmethod
    def forward(ctx, x, y, sp, hs: Handle | None, mask):
        B, T, D = x.shape
        y2 = y.reshape(B * T, D)
        out = P.residual_fwd(x, y2, hs, mask)
        ctx.save_for_backward(y2 if hs is not None else None, mask)
        ctx.hs = hs
        ctx.ydtype = y.dtype
        ctx.yshape = y.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        y2, mask = ctx.saved_tensors
        dout = dout.contiguous()
        dy, _ = P.residual_bwd(dout, y2, ctx.hs, mask, ctx.ydtype)
        return dout, dy.reshape(ctx.yshape), None, None, None


def residual(x: torch.Tensor, y: torch.Tensor, hs: Handle | None = None, mask: torch.Tensor | None = None):
    if hs is not None:
        hs.note_use()
    return _Residual.apply(x, y, hs.param if hs is not None else None, hs, mask)


# ------------------------------------------------------------------------------- attention
class _Attention(torch.autograd.Function):
    """qkv: [B, S, 3, H, hd] (compute dtype) -> o: [B, S, H*hd]."""

    @staticmethod
    def forward(ctx, qkv, heads: int):
        o, lse = P.attn_fwd(qkv, heads)
        ctx.save_for_backward(qkv, o, lse)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        return P.attn_bwd(do, qkv, o, lse, ctx.heads)[0], None


def attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    return _Attention.apply(qkv, heads)


# ------------------------------------------------------------------ rotary position embedding
class _Rope(torch.autograd.Function):
    """qkv [B, S, 3 * H * hd] -> a copy with q and k of the patch rows rotated (ops/rope.py); the
    gradient is the transpose applied to a copy of the incoming one."""

    @staticmethod
    def forward(ctx, qkv, heads: int, rope):
        ctx.heads, ctx.rope = heads, rope
        return P.rope_(qkv.clone(memory_format=torch.contiguous_format), heads, rope.n_cls, rope.gw, rope.table,
                       rope.pos)

    @staticmethod
    def backward(ctx, dout):
        r = ctx.rope
        d = dout.clone(memory_format=torch.contiguous_format)
        return P.rope_(d, ctx.heads, r.n_cls, r.gw, r.table, r.pos, inverse=True), None, None


def rope(qkv: torch.Tensor, heads: int, rope) -> torch.Tensor:
    """The per-op path's rotary embedding (``rope``: an ``ops.rope.Rope``); the fused blocks rotate
    their own qkv in place (ops/blocks.py)."""
    return _Rope.apply(qkv, heads, rope)


# ------------------------------------------------------------------------------------ QK-norm
class _QKNorm(torch.autograd.Function):
    """qkv [B, S, 3 * H * hd] -> a copy with q and k normalised per head (and rotated, with
    ``rope``); saves the pre-norm q|k, from which the backward recomputes r (ops/qknorm.py)."""

    @staticmethod
    def forward(ctx, qkv, qp, kp, hq: Handle, hk: Handle, heads: int, rope):
        out = qkv.clone(memory_format=torch.contiguous_format)
        saved = P.qknorm_fwd_(out, heads, hq.master, hk.master, rope)
        ctx.save_for_backward(saved)
        ctx.hq, ctx.hk, ctx.heads, ctx.rope = hq, hk, heads, rope
        return out

    @staticmethod
    def backward(ctx, dout):
        (saved,) = ctx.saved_tensors
        d = dout.clone(memory_format=torch.contiguous_format)
        d, dg = P.qknorm_bwd_(d, saved, ctx.heads, ctx.hq.master, ctx.hk.master, ctx.rope)
        ctx.hq.accumulate_grad(dg[0])
        ctx.hk.accumulate_grad(dg[1])
        return d, None, None, None, None, None, None


def qknorm(qkv: torch.Tensor, hq: Handle, hk: Handle, heads: int, rope=None) -> torch.Tensor:
    """The per-op path's QK-norm (``hq`` / ``hk``: the layer's q_norm / k_norm scale handles;
    ``rope``: an ``ops.rope.Rope`` or None); the fused blocks normalise their own qkv in place."""
    hq.note_use()
    hk.note_use()
    return _QKNorm.apply(qkv, hq.param, hk.param, hq, hk, heads, rope)


# ------------------------------------------------------------------------------- SwiGLU gate
class _SwiGLU(torch.autograd.Function):
    """pre [.., 2 Hs] = [gate | up] -> a [.., Hs] = silu(gate) * up with the hidden dropout ``drop`` = (seed,
    rate) applied inside (ops/swiglu.py); the backward regenerates the mask from the seed."""

    @staticmethod
    def forward(ctx, pre, drop):
        p2 = pre.reshape(-1, pre.shape[-1]).contiguous()
        ctx.save_for_backward(p2)
        ctx.drop, ctx.shape = drop, pre.shape
        return P.swiglu_fwd(p2, drop).reshape(*pre.shape[:-1], pre.shape[-1] // 2)

    @staticmethod
    def backward(ctx, da):
        (p2,) = ctx.saved_tensors
        dpre, _ = P.swiglu_bwd(p2, da.reshape(-1, da.shape[-1]).contiguous(), None, ctx.drop)
        return dpre.reshape(ctx.shape), None


def swiglu(pre: torch.Tensor, drop=None) -> torch.Tensor:
    """The per-op path's gate of the gated feed-forward (the fused blocks call the primitives themselves); the
    bias gradients of w1 | w3 are the column sums the FF1 Dense's own backward takes of the returned dpre."""
    return _SwiGLU.apply(pre, drop)


# ---------------------------------------------------------------- classification loss + accuracy
def cls_loss_torch(logits, labels_int, plan=None, smoothing: float = 0.0, criterion: str = "ce"):
    """The torch composition of models/classifier.py on integer labels: scattered one-hot ->
    ``smooth_labels`` -> ``Mixup.mix_labels`` -> criterion and top-1 / top-5 membership in the
    arg-max label set.  The CPU path of ``cls_loss``, and what defines the kernels' semantics."""
    from ..models.classifier import CRITERION_COLLECTION, FinetuneModel  # (imports this module)
    from ..utils.mixup import Mixup, smooth_labels

    B, L = logits.shape
    idx = labels_int.long().clamp(0, L - 1).view(-1, 1)
    t = torch.zeros(B, L, device=logits.device).scatter_(1, idx, 1.0)
    t = Mixup.mix_labels(smooth_labels(t, smoothing), plan)
    logits = logits.float()
    acc1, acc5 = FinetuneModel.accuracy(logits, t)
    return CRITERION_COLLECTION[criterion](logits, t), acc1, acc5


class _ClsLoss(torch.autograd.Function):
    """logits [B, L] (bf16 or fp32, unit column stride) -> per-row loss and the bool [B, 2] hits
    (csrc/loss.hip); the dense targets exist only as (labels, perm, w)."""

    @staticmethod
    def forward(ctx, logits, labels, perm, w, smoothing: float, mode: int):
        loss, hit, lse = P._ext.load().cls_loss_fwd(logits, labels, perm, w, smoothing, mode)
        ctx.save_for_backward(logits, labels, perm, w, lse)
        ctx.smoothing, ctx.mode = smoothing, mode
        ctx.mark_non_differentiable(hit)
        return loss, hit

    @staticmethod
    def backward(ctx, dloss, _dhit):
        logits, labels, perm, w, lse = ctx.saved_tensors
        dz = P._ext.load().cls_loss_bwd(dloss.float().contiguous(), logits, labels, perm, w, ctx.smoothing, ctx.mode,
                                        lse)
        return dz, None, None, None, None, None


def _plan_buffers(plan, device):
    """(perm int32 [B], w fp32 [1]) of a Mixup plan on the device: its static buffers when it has them."""
    if plan is None:
        return None, None
    dev = plan.get("dev")
    if dev is not None:
        return dev["perm"], dev["params"][2:3]
    perm = torch.as_tensor(plan["perm"]).to(device=device, dtype=torch.int32).contiguous()
    return perm, torch.as_tensor(plan["label_w_t"], dtype=torch.float32).to(device).reshape(1)


def cls_loss(logits: torch.Tensor, labels_int: torch.Tensor, plan: dict | None = None, smoothing: float = 0.0,
             criterion: str = "ce"):
    """(loss [B] fp32, acc1 [B] bool, acc5 [B] bool) of integer class ids against ``logits`` [B, L]:
    ``criterion`` ("ce" | "bce") on the one-hot targets smoothed by ``smoothing`` and mixed per the
    Mixup ``plan``.  On the GPU one fused kernel each way (the accuracies carry no gradient); on the
    CPU, or with ``prims._CLS_LOSS_OURS`` off, the torch composition ``cls_loss_torch``."""
    if not (P._CLS_LOSS_OURS and P.hip(logits)):
        return cls_loss_torch(logits, labels_int, plan, smoothing, criterion)
    if criterion not in ("ce", "bce"):
        raise KeyError(criterion)
    if logits.stride(-1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        logits = logits.contiguous()  # strided columns or overlapping rows (an expanded batch)
    perm, w = _plan_buffers(plan, logits.device)
    loss, hit = _ClsLoss.apply(logits, labels_int.long().contiguous(), perm, w, float(smoothing),
                               0 if criterion == "ce" else 1)
    return loss, hit[:, 0], hit[:, 1]


# ---------------------------------------------------------------- distillation loss + agreement
KD_MODES = ("soft", "hard")


def argmax_first(x: torch.Tensor) -> torch.Tensor:
    """arg-max over the last dim, the lowest index among ties -- by construction, not by the backend's
    tie rule."""
    L = x.shape[-1]
    idx = torch.arange(L, device=x.device).expand(x.shape)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, L).min(-1).values.clamp_(max=L - 1)


class _KdSoftTorch(torch.autograd.Function):
    """T^2 KL(softmax(u / T) || softmax(z / T)) per row with the gradient written out, T (p - q): the
    autograd of the composition would leave T^2 q (sum q - 1) where p == q."""

    @staticmethod
    def forward(ctx, z, u, T: float):
        lp, lq = torch.log_softmax(z / T, -1), torch.log_softmax(u / T, -1)
        p, q = lp.exp(), lq.exp()
        ctx.save_for_backward(p, q)
        ctx.T = T
        return (T * T) * (q * (lq - lp)).sum(-1)

    @staticmethod
    def backward(ctx, dkd):
        p, q = ctx.saved_tensors
        return dkd.unsqueeze(-1) * (ctx.T * (p - q)), None, None


def kd_loss_torch(z: torch.Tensor, u: torch.Tensor, T: float = 1.0, mode: str = "soft"):
    """(kd [B], agree [B] bool) of student logits ``z`` against teacher logits ``u`` ([B, L]):
      soft  kd = T^2 sum_c q_c (log q_c - log p_c), q = softmax(u / T), p = softmax(z / T); d kd / d z = T (p - q);
      hard  kd = -log softmax(z)_t, t = the teacher's arg-max (DeiT; T unused); d kd / d z = softmax(z) - onehot(t);
      agree = the two arg-maxima coincide; every arg-max is the lowest index among ties.
    ``u`` takes no gradient.  Runs in the logits' dtype (bf16 / fp16 logits in fp32).  The CPU path of
    ``kd_loss``, and what defines the kernels' semantics."""
    if mode not in KD_MODES:
        raise KeyError(mode)
    if not T > 0:
        raise ValueError(f"distillation temperature {T}: expected > 0")
    u = u.detach()
    if z.dtype in (torch.bfloat16, torch.float16):
        z, u = z.float(), u.float()
    t = argmax_first(u)
    agree = argmax_first(z.detach()) == t
    if mode == "soft":
        return _KdSoftTorch.apply(z, u, float(T)), agree
    return -torch.log_softmax(z, -1).gather(1, t.view(-1, 1)).squeeze(1), agree


class _KdLoss(torch.autograd.Function):
    """z, u [B, L] (bf16 or fp32, unit column stride) -> per-row kd fp32 and the bool agreement
    (csrc/distill.hip); the backward reads u in soft mode and the saved teacher arg-max in hard mode."""

    @staticmethod
    def forward(ctx, z, u, T: float, mode: int):
        kd, agree, lse, t = P._ext.load().kd_loss_fwd(z, u, T, mode)
        ctx.save_for_backward(z, u if mode == 0 else None, lse, t if mode == 1 else None)
        ctx.T, ctx.mode = T, mode
        ctx.mark_non_differentiable(agree)
        return kd, agree

    @staticmethod
    def backward(ctx, dkd, _dagree):
        z, u, lse, t = ctx.saved_tensors
        dz = P._ext.load().kd_loss_bwd(dkd.float().contiguous(), z, u, ctx.T, ctx.mode, lse, t)
        return dz, None, None, None


def _rows_ok(x: torch.Tensor) -> bool:
    return x.stride(-1) == 1 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1])


def kd_loss(z: torch.Tensor, u: torch.Tensor, T: float = 1.0, mode: str = "soft"):
    """(kd [B] fp32, agree [B] bool) as ``kd_loss_torch`` defines them.  On the GPU one fused kernel each
    way (u and the agreement carry no gradient); on the CPU, or with ``prims._KD_OURS`` off, the torch
    composition."""
    if not (P._KD_OURS and P.hip(z)):
        return kd_loss_torch(z, u, T, mode)
    if mode not in KD_MODES:
        raise KeyError(mode)
    if z.shape != u.shape or z.dtype != u.dtype:
        raise ValueError(f"kd_loss: student {tuple(z.shape)} {z.dtype} against teacher {tuple(u.shape)} {u.dtype}")
    z = z if _rows_ok(z) else z.contiguous()  # strided columns or overlapping rows (an expanded batch)
    u = u.detach()
    u = u if _rows_ok(u) else u.contiguous()
    return _KdLoss.apply(z, u, float(T), KD_MODES.index(mode))
