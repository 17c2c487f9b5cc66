"""Finetune / linear-probe task module.

Parity: ``FinetuneModule`` (/root/reference/src/finetuning.py:78-106), ``CRITERION_COLLECTION``
(:39-42), the classifier branch of ``ViT.__call__`` (modeling.py:268-274) and ``validation_step``
(finetuning.py:157-165).

* labels: int -> one-hot; training applies label smoothing then Mixup/CutMix;
* logits = head(LN(x)[:, :3].reshape(B, 3D)) -- only the 3 CLS rows go through the final LN
  (per-row op, identical result);
* linear probing: the encoder runs without autograd (== ``stop_gradient``) and the head is
  SyncBatchNorm + Dense;
* accuracy = membership of the top-1 / top-5 predictions in the arg-max label set.
Fixes: RNG streams advance every step (quirk Q4); validation loss is the true per-sample masked
mean (the reference multiplies the batch-mean loss, padded samples included, by the valid count).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from ..config import ViTConfig
from ..ops import attn_maps as AM
from ..ops import attn_stats as AS
from ..ops import functional as Fn
from ..ops import mae as mae_ops
from ..ops import prims as P
from ..utils.mixup import Mixup, smooth_labels
from .params import ParamStore
from .vit import JumboViT, LinearCLS, cls_features


def softmax_cross_entropy(logits, labels):
    return -(labels * F.log_softmax(logits, -1)).sum(-1)


def sigmoid_bce(logits, labels):
    t = (labels > 0).to(logits.dtype)
    return F.binary_cross_entropy_with_logits(logits, t, reduction="none").mean(-1)


CRITERION_COLLECTION = {"ce": softmax_cross_entropy, "bce": sigmoid_bce}


_DRAW = object()  # patches / logits: take the batch's plan from step_plan


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class FinetuneModel:
    def __init__(self, cfg: ViTConfig, mixup: Mixup | None = None, label_smoothing: float = 0.0,
                 criterion: str = "ce", group=None):
        assert cfg.labels > 0
        self.cfg = cfg
        self.store = ParamStore()
        s = self.store
        trainable_encoder = not cfg.linear_probing
        self.encoder = JumboViT(s, cfg, ("model",), trainable=trainable_encoder)
        self.head = LinearCLS(s, ("model", "head"), cfg.jumbo_dim, cfg.labels, cfg.batch_norm)
        self.mixup = mixup or Mixup(0.0, 0.0)
        self.label_smoothing = label_smoothing if criterion == "ce" else 0.0
        self.criterion = CRITERION_COLLECTION[criterion]
        self.criterion_name = criterion
        self.group = group
        self.teacher: FinetuneModel | None = None  # attach_teacher
        self.frozen = False

    def freeze(self):
        """Before ``to``: every segment frozen -- no gradient buffer is allocated and no op writes one
        (a distillation teacher: outside the optimizer, the reducer and the EMA, which see the
        student's store only)."""
        assert not self.store.finalized
        for s in self.store.segments:
            s.trainable = False
        self.frozen = True
        return self

    def to(self, device, compute_dtype=torch.float32, seed: int = 0):
        g = torch.Generator(device=device).manual_seed(seed)
        self.store.finalize(device, compute_dtype, g, with_grad=not self.frozen)
        self.head.init_stats(device)
        return self

    def attach_teacher(self, teacher: "FinetuneModel", alpha: float = 0.5, temperature: float = 1.0,
                       mode: str = "soft") -> None:
        """Distillation: ``forward(det=False)`` then returns ``(1 - alpha) * base + alpha * mean kd`` with
        ``kd`` = ``Fn.kd_loss`` of the student's logits against those of ``teacher`` (a frozen
        FinetuneModel without BatchNorm head, dropout, droppath or Mixup, run on the same mixed patch
        rows under ``no_grad``).  ``evaluate`` stays the student alone."""
        tc, sc = teacher.cfg, self.cfg
        if not (teacher.frozen and teacher.store.finalized and teacher.store.num_params(True) == 0):
            raise ValueError("the teacher must be frozen (FinetuneModel.freeze) and on its device")
        if tc.linear_probing or tc.batch_norm or tc.dropout or tc.droppath or teacher.mixup.active:
            raise ValueError("the teacher runs without BatchNorm head, dropout, droppath and Mixup")
        for k in ("patch_size", "image_size", "labels"):
            if getattr(tc, k) != getattr(sc, k):
                raise ValueError(f"teacher {k} {getattr(tc, k)} != student {k} {getattr(sc, k)}")
        if teacher.store.compute_dtype != self.store.compute_dtype or teacher.device != self.device:
            raise ValueError("teacher and student must share the compute dtype and the device")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"distillation alpha {alpha}: expected 0 <= alpha <= 1")
        if not temperature > 0.0:
            raise ValueError(f"distillation temperature {temperature}: expected > 0")
        if mode not in Fn.KD_MODES:
            raise ValueError(f"distillation mode {mode!r}: expected one of {Fn.KD_MODES}")
        self.teacher, self.kd_alpha, self.kd_temperature, self.kd_mode = teacher, float(alpha), float(temperature), mode

    @property
    def device(self):
        return self.store.master.device

    # ---------------------------------------------------------------- pieces
    micro_index = 0

    def prepare_step(self, i: int, images_u8, labels=None) -> None:
        """Host part of a train step (engine.Trainer.host_prepare): draw micro-batch ``i``'s Mixup /
        CutMix decision; its device buffers are what the (possibly graph-replayed) forward reads."""
        if not self.mixup.active:
            return
        if not hasattr(self, "_plans"):
            self._plans = {}
        B, _, H, W = images_u8.shape
        self._plans[i] = self.mixup.plan(B, H, W, images_u8.device, tag=str(i))

    def step_plan(self, images_u8, rngs, det):
        """This batch's Mixup / CutMix plan (None when not training or mixing is off): the one
        ``prepare_step`` drew for the current micro-batch, or a fresh draw for a direct call."""
        if det or not self.mixup.active:
            return None
        B, _, H, W = images_u8.shape
        plans = getattr(self, "_plans", {})
        plan = plans.pop(self.micro_index, None) if not _capturing() else plans.get(self.micro_index)
        if plan is None:  # direct forward call without a prepared step: draw here
            plan = self.mixup.plan(B, H, W, images_u8.device, rngs.get("mixup") if rngs else None)
        return plan

    def patches(self, images_u8, labels, rngs, det, plan=_DRAW):
        """(patch rows [B*N, p*p*3] in the compute dtype, labels) -- Mixup / CutMix applied when
        training (one plan per batch, ``step_plan`` unless the caller passes the plan it took; the
        blend is fused into the patch gather on the GPU)."""
        if plan is _DRAW:
            plan = self.step_plan(images_u8, rngs, det)
        if labels is not None:
            labels = Mixup.mix_labels(labels, plan)
        rows = mae_ops.mixed_patches(images_u8, plan, self.cfg.patch_size, self.store.compute_dtype)
        return rows, labels

    def features(self, rows, B, rngs=None, det=True):
        return cls_features(self.encoder, rows, B, rngs.get("dropout") if rngs else None, det)

    def logits(self, images_u8, labels=None, rngs=None, det=True, raw=False, plan=_DRAW):
        """(logits, mixed labels); ``raw``: the head's output in the compute dtype instead of fp32;
        ``plan``: as in ``patches``."""
        rows, labels = self.patches(images_u8, labels, rngs, det, plan)
        return self.logits_of_rows(rows, images_u8.shape[0], rngs, det, raw), labels

    def logits_of_rows(self, rows, B, rngs=None, det=True, raw=False):
        """Encoder + head on prepared patch rows (``patches``)."""
        if self.cfg.linear_probing:
            with torch.no_grad():
                feats = self.features(rows, B, rngs, det)
        else:
            feats = self.features(rows, B, rngs, det)
        return self.head(feats, det, self.group, raw)

    # ---------------------------------------------------------------- train / eval
    def _fused_loss(self, images_u8, labels) -> bool:
        """Integer class ids on the GPU: loss and accuracies come from ``Fn.cls_loss`` on the head's own
        (bf16) logits and the plan's device buffers; no dense target is built.  Dense soft labels and
        the CPU keep the torch composition below."""
        return (labels.dim() == 1 and not labels.is_floating_point() and labels.is_cuda and P._CLS_LOSS_OURS
                and P.hip(images_u8))

    def forward(self, images_u8, labels, rngs=None, det=False):
        if self.teacher is not None and not det:
            return self._forward_distill(images_u8, labels, rngs)
        if self._fused_loss(images_u8, labels):
            plan = self.step_plan(images_u8, rngs, det)
            logits, _ = self.logits(images_u8, None, rngs, det, raw=True, plan=plan)
            loss, acc1, acc5 = Fn.cls_loss(logits, labels, plan, 0.0 if det else self.label_smoothing,
                                           self.criterion_name)
            return {"loss": loss.mean(), "acc1": acc1.float().mean(), "acc5": acc5.float().mean()}
        labels = self._prep_labels(labels)
        if not det:
            labels = smooth_labels(labels, self.label_smoothing)
        logits, labels = self.logits(images_u8, labels, rngs, det)
        loss = self.criterion(logits, labels).mean()
        acc1, acc5 = self.accuracy(logits, labels)
        return {"loss": loss, "acc1": acc1.float().mean(), "acc5": acc5.float().mean()}

    def _forward_distill(self, images_u8, labels, rngs):
        """The train step with a teacher: one plan and one set of mixed patch rows feed both networks
        (the teacher takes nothing from ``rngs``); the base loss is the one ``forward`` computes without
        a teacher, on the same path (fused or dense)."""
        B = images_u8.shape[0]
        plan = self.step_plan(images_u8, rngs, False)
        rows, _ = self.patches(images_u8, None, rngs, False, plan)
        with torch.no_grad():
            u = self.teacher.logits_of_rows(rows, B, None, True, raw=True)
        if self._fused_loss(images_u8, labels):
            z = self.logits_of_rows(rows, B, rngs, False, raw=True)
            base, acc1, acc5 = Fn.cls_loss(z, labels, plan, self.label_smoothing, self.criterion_name)
            base = base.mean()
        else:
            t = Mixup.mix_labels(smooth_labels(self._prep_labels(labels), self.label_smoothing), plan)
            z = self.logits_of_rows(rows, B, rngs, False)
            base = self.criterion(z, t).mean()
            acc1, acc5 = self.accuracy(z, t)
        a = self.kd_alpha
        with torch.set_grad_enabled(a > 0.0):
            kd, agree = Fn.kd_loss(z, u.to(z.dtype), self.kd_temperature, self.kd_mode)
            kd = kd.mean()
        # the end points are taken literally: alpha 0 is the base loss bit for bit (value and backward),
        # alpha 1 trains on the teacher alone
        loss = base if a == 0.0 else (kd if a == 1.0 else (1.0 - a) * base + a * kd)
        return {"loss": loss, "acc1": acc1.float().mean(), "acc5": acc5.float().mean(), "cls_loss": base.detach(),
                "kd_loss": kd.detach(), "kd_agree": agree.float().mean()}

    __call__ = forward

    def _prep_labels(self, labels):
        if labels.dim() == 1:  # one-hot by scatter: F.one_hot validates the range with a host sync
            idx = labels.long().clamp(0, self.cfg.labels - 1).view(-1, 1)
            return torch.zeros(labels.shape[0], self.cfg.labels, device=labels.device).scatter_(1, idx, 1.0)
        return labels.float()

    @staticmethod
    def accuracy(logits, labels):
        lab = labels == labels.max(-1, keepdim=True).values
        k = min(5, logits.shape[-1])
        top = logits.topk(k, -1).indices
        accs = torch.gather(lab, 1, top)
        return accs[:, 0], accs.any(-1)

    @torch.no_grad()
    def attention_stats(self, images_u8) -> dict:
        """``{layer_<i>: float64 [H, 6]}`` (ops/attn_stats.py) of every encoder layer in one ``det=True``
        forward of the unmixed images; the head does not run, so BatchNorm statistics are untouched."""
        rows, _ = self.patches(images_u8, None, None, True, plan=None)
        names = [f"layer_{i}" for i in range(len(self.encoder.layers))]
        return AS.collect_layers(names, lambda: self.features(rows, images_u8.shape[0], None, True),
                                 self.cfg.num_cls_tokens)

    @torch.no_grad()
    def attention_maps(self, images_u8, alpha: float = 0.5, mode: str = "rollout") -> dict:
        """``{"maps": fp32 [B, n_cls, gh, gw], "cls_mass": fp32 [B, n_cls]}`` (ops/attn_maps.py): the CLS
        attention rollout (``mode="last"``: the last layer's head-mean CLS attention) from one ``det=True``
        encoder forward of the unmixed images, as in ``attention_stats``; the head does not run."""
        rows, _ = self.patches(images_u8, None, None, True, plan=None)
        got = AM.collect_layers(lambda: self.features(rows, images_u8.shape[0], None, True), len(self.encoder.layers))
        g = self.cfg.grid
        return AM.maps_and_mass(got, got.heads, self.cfg.num_cls_tokens, g, g, alpha, mode)

    @torch.no_grad()
    def evaluate(self, images_u8, labels, rngs=None, report=None) -> dict:
        """Sums over valid (label != -1) samples, like validation_step (finetuning.py:157-165).  ``report``
        (ops/eval_report.py EvalReport) is fed the logits the loss reads and the labels as given; the sums
        do not depend on it."""
        valid = (labels != -1)
        if self._fused_loss(images_u8, labels):
            logits, _ = self.logits(images_u8, None, rngs, det=True, raw=True)
            if report is not None:
                report.update(logits, labels)
            loss, acc1, acc5 = Fn.cls_loss(logits, torch.where(valid, labels, torch.zeros_like(labels)), None, 0.0,
                                           self.criterion_name)
            v = valid.float()
            return {"loss": (loss * v).sum(), "acc1": (acc1.float() * v).sum(), "acc5": (acc5.float() * v).sum(),
                    "num_samples": v.sum()}
        lab = self._prep_labels(torch.where(valid, labels, torch.zeros_like(labels)))
        logits, _ = self.logits(images_u8, lab, rngs, det=True)
        if report is not None:
            report.update(logits, labels)
        loss = self.criterion(logits, lab)
        acc1, acc5 = self.accuracy(logits, lab)
        v = valid.float()
        return {"loss": (loss * v).sum(), "acc1": (acc1.float() * v).sum(), "acc5": (acc5.float() * v).sum(),
                "num_samples": v.sum()}

    # ---------------------------------------------------------------- params
    def flax_params(self) -> dict:
        return self.store.to_flax_tree()

    def batch_stats(self) -> dict | None:
        if not self.cfg.batch_norm:
            return None
        return {"model": {"head": {"BatchNorm_0": {"mean": self.head.running_mean.cpu().numpy(),
                                                   "var": self.head.running_var.cpu().numpy()}}}}
