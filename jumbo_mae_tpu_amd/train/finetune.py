"""Finetune / linear-probe driver (``main_finetune``).

Parity: /root/reference/src/main_finetune.py:37-94 and create_train_state
(/root/reference/src/finetuning.py:168-278):
  * ``--mode finetune``: end-to-end training with Mixup/CutMix, label smoothing, LLRD, droppath;
  * ``--mode linear``: frozen encoder (stop-gradient) + SyncBatchNorm + Dense head;
  * optimizers adamw | lamb | lars | sgd (momentum 0.9); peak LR = lr * B / 256 for LARS, raw lr
    otherwise; warmup-cosine from 1e-6 to 1e-6;
  * ``--pretrained-ckpt``: Flax msgpack; encoder subtree loaded into the fresh tree (Q6 fix);
  * best checkpoint by maximum ``val/acc1``;
  * ``--ema-decay D`` (extension): a weight average follows every optimizer step (optim/ema.py); every
    evaluation runs a second time with the averaged weights swapped in (``val/ema_*``) and the best of
    them is written to ``{name}-ema-best.msgpack``;
  * ``--log-norms global|layer`` (extension): gradient / weight / update norms of every logged step
    (optim/monitor.py), written before the non-finite check so that an abort names its leaves;
  * ``--attn-stats N`` (extension): at every evaluation rank 0 logs the per-layer attention entropy,
    largest logit, largest probability and CLS mass of the first N validation images (ops/attn_stats.py);
  * ``--attn-maps N`` (extension): at every evaluation rank 0 writes the CLS attention maps of the first N
    validation images as a PNG panel and logs their entropy and CLS mass (ops/attn_maps.py);
  * ``--teacher-ckpt URL`` (extension): distillation against a frozen finetuned teacher (``build_teacher``,
    ``FinetuneModel.attach_teacher``, ops/functional.py ``kd_loss``): train/cls_loss, train/kd_loss and
    train/kd_agree are logged and the first evaluation also runs with the teacher (val/teacher_*);
  * ``--eval-report`` (extension): every evaluation also accumulates per-class accuracy, calibration bins and
    the confusion matrix from its logits (ops/eval_report.py) -- val/mean_class_acc1, val/ece, ... -- and
    rank 0 writes ``{name}-report-{step}.json`` and ``{name}-confusion-{step}.npy``.
"""

from __future__ import annotations

import time

import torch

from ..ckpt.checkpoint import load_params, load_pretrained_params, save_params
from ..config import ViTConfig
from ..data.loader import create_dataloaders
from ..models.classifier import FinetuneModel
from ..ops.eval_report import EvalReport
from ..optim.monitor import log_norms, make_monitor
from ..parallel import dist as pdist
from ..utils import gopen
from ..utils.flops import finetune_fwd_flops_per_image
from ..utils.mixup import Mixup
from ..utils.trace import set_enabled as set_trace_ranges
from ..utils.rng import RngStreams
from . import common as C
from .cli import finetune_parser
from ..runtime.graph import StepRunner
from .engine import Trainer
from .meter import AverageMeter, Logger


def build_model(args, device, dtype, rank: int = 0) -> FinetuneModel:
    linear = args.mode == "linear"
    vc = ViTConfig(layers=args.layers, dim=args.dim, heads=args.heads, labels=args.labels, layerscale=args.layerscale,
                   patch_size=args.patch_size, image_size=args.image_size, posemb=args.posemb, pooling=args.pooling,
                   rope_theta=args.rope_theta, qk_norm=args.qk_norm, ffn=args.ffn,
                   dropout=args.dropout, droppath=args.droppath, grad_ckpt=args.grad_ckpt, image_mask_ratio=None,
                   linear_probing=linear, batch_norm=linear)
    mix = Mixup(args.mixup, args.cutmix, seed=args.mixup_seed * 1009 + rank)
    return FinetuneModel(vc, mix, args.label_smoothing, args.criterion).to(device, dtype, seed=args.init_seed)


def build_teacher(args, device, dtype, log=print) -> FinetuneModel:
    """--teacher-ckpt: the frozen distillation teacher -- the student's patch size, image size, labels and
    position embedding; its own depth / width / heads / layerscale / feed-forward kind; no BatchNorm head, dropout, droppath
    or Mixup -- with EVERY leaf (encoder and head) taken from the checkpoint: a missing leaf or a shape
    mismatch is an error that names the leaf.  Every rank holds the whole teacher (rank 0's copy)."""
    vc = ViTConfig(layers=args.teacher_layers or args.layers, dim=args.teacher_dim or args.dim,
                   heads=args.teacher_heads or args.heads, labels=args.labels, layerscale=args.teacher_layerscale,
                   patch_size=args.patch_size, image_size=args.image_size, posemb=args.posemb, pooling=args.pooling,
                   rope_theta=args.rope_theta, qk_norm=args.qk_norm, ffn=args.teacher_ffn or args.ffn,
                   dropout=0.0, droppath=0.0, grad_ckpt=False, image_mask_ratio=None, linear_probing=False,
                   batch_norm=False)
    teacher = FinetuneModel(vc, None, 0.0, args.criterion).freeze().to(device, dtype, seed=args.init_seed)
    tree = load_params(args.teacher_ckpt)
    if "model" not in tree and isinstance(tree.get("params"), dict):
        tree = tree["params"]
    try:
        teacher.store.load_flax_tree(tree, strict=True)
    except KeyError as e:
        raise KeyError(f"--teacher-ckpt {args.teacher_ckpt}: no leaf {e.args[0]} (a finetune checkpoint with its "
                       "head is needed; check --teacher-layers / --teacher-layerscale)") from None
    except ValueError as e:
        raise ValueError(f"--teacher-ckpt {args.teacher_ckpt}: {e} (check --teacher-dim / --teacher-heads / "
                         "--labels)") from None
    pdist.broadcast_(teacher.store.master)
    teacher.store.sync_shadow()
    log(f"Teacher weights are loaded from {args.teacher_ckpt}.")
    return teacher


def evaluate_teacher(teacher, loader, rngs, device) -> dict:
    """The validation pass with the teacher (val/teacher_loss, val/teacher_acc1, val/teacher_acc5): how a
    user sees that it loaded correctly.  As in ``evaluate_ema``, the default generator is put back."""
    with torch.random.fork_rng(devices=[]):
        res = evaluate(teacher, loader, rngs, device)
    return {k.replace("val/", "val/teacher_"): v for k, v in res.items()}


def make_report(args, model, device):
    """--eval-report: a fresh report for one validation pass, else None."""
    if not args.eval_report:
        return None
    return EvalReport(model.cfg.labels, args.eval_report_bins, args.criterion, device)


def finish_report(report, args, step: int, log, tag: str = "") -> dict:
    """After the pass (COLLECTIVE): one int64 all-reduce, then rank 0 writes
    ``{output_dir}/{name}-{tag}report-{step:07d}.json`` and, while the matrix is kept,
    ``{name}-{tag}confusion-{step:07d}.npy``; returns the ``val/{tag}...`` metrics (``tag``: "" or "ema_")."""
    import os

    import numpy as np

    report.all_reduce()
    prefix = "val/" + tag
    if pdist.info().is_main:
        out = args.output_dir or "."
        if gopen.is_local(out):
            os.makedirs(out, exist_ok=True)
            stem = os.path.join(out, f"{args.name or 'run'}-{tag.replace('_', '-')}")
            with open(f"{stem}report-{step:07d}.json", "w") as f:
                f.write(report.dumps(step, prefix))
            cm = report.confusion()
            if cm is not None:
                np.save(f"{stem}confusion-{step:07d}.npy", cm)
        else:
            log(f"[eval] --eval-report: remote --output-dir {args.output_dir}, report files skipped")
    return report.summary(prefix)


def evaluate(model, loader, rngs, device, report=None) -> dict:
    rngs = rngs.fork()  # validation never advances the training streams
    sums = None
    for images, labels in C.DevicePrefetcher(loader, device):
        m = model.evaluate(images, labels, rngs.as_dict(), **({} if report is None else {"report": report}))
        sums = m if sums is None else {k: sums[k] + m[k] for k in m}
    keys = ["loss", "acc1", "acc5", "num_samples"]
    packed = torch.stack([sums[k].float() for k in keys])
    pdist.all_reduce_sum_(packed)
    vals = dict(zip(keys, packed.tolist()))
    n = max(vals.pop("num_samples"), 1.0)
    return {f"val/{k}": v / n for k, v in vals.items()}


def evaluate_ema(model, ema, loader, rngs, device, report=None) -> dict:
    """The validation pass with the averaged weights swapped into the store (COLLECTIVE under ZeRO-1):
    val/ema_loss, val/ema_acc1, val/ema_acc5.  BatchNorm running statistics are the live ones.  A loader
    iterator seeds its workers from the default generator, which this second pass must not advance."""
    with ema.swapped(), torch.random.fork_rng(devices=[]):
        res = evaluate(model, loader, rngs, device, report)
    return {k.replace("val/", "val/ema_"): v for k, v in res.items()}


def save_ema_best(args, model, ema) -> None:
    """{name}-ema-best.msgpack: the ordinary Flax params tree of the averaged weights, copied to the
    host while they are swapped in (COLLECTIVE under ZeRO-1; rank 0 writes)."""
    with ema.swapped():
        tree = model.flax_params() if pdist.info().is_main else None
    if tree is not None:
        save_params(args.output_dir, args.name or "run", tree, "ema-best")


def main(args) -> dict:
    info = pdist.init_distributed(args.device)
    set_trace_ranges(args.trace_ranges)
    device = info.device
    log = print if info.is_main else (lambda *a, **k: None)
    dtype = C.compute_dtype(args, device)
    model = build_model(args, device, dtype, info.rank)
    if args.pretrained_ckpt:
        tree = load_pretrained_params(args.pretrained_ckpt, model.flax_params(), log)
        model.store.load_flax_tree(tree, strict=False)
        log(f"Pretrained weights are loaded from {args.pretrained_ckpt}.")
    pdist.broadcast_(model.store.master)
    model.store.sync_shadow()
    C.summarize_params(model.store, log)
    teacher = None
    if args.teacher_ckpt:  # rebuilt from the flag on --resume too: checkpoints hold the student only
        teacher = build_teacher(args, device, dtype, log)
        model.attach_teacher(teacher, args.distill_alpha, args.distill_temperature, args.distill_mode)
        log(f"Distillation ({args.distill_mode}, alpha {args.distill_alpha:g}, T {args.distill_temperature:g}): "
            f"student {model.store.num_params():,} parameters, teacher {teacher.store.num_params():,} (frozen)")
    if model.cfg.batch_norm:
        log("BatchNorm statistics are initialized.")
    peak = args.learning_rate * args.train_batch_size / 256 if args.optimizer == "lars" else args.learning_rate
    opt = C.make_optimizer(args, model.store, peak, 1e-6)
    reducer = C.make_reducer(args, model.store)
    rngs = RngStreams({"mixup": args.mixup_seed, "dropout": args.dropout_seed, "noise": args.noise_seed},
                      info.rank, device)
    trainer = Trainer(model, opt, reducer, rngs, args.grad_accum, skip_nonfinite=args.skip_nonfinite)
    run_step = StepRunner(trainer, hip_graph=args.hip_graph and device.type == "cuda" and info.world_size == 1)
    resumed = C.maybe_resume(args, model, opt, rngs, log)
    start = resumed.step
    ema = C.make_ema(args, model.store, opt, resumed, log)
    monitor = make_monitor(args, opt)  # --log-norms

    def extra():
        if not model.cfg.batch_norm:
            return None
        return {"batch_stats": {"mean": model.head.running_mean.cpu(), "var": model.head.running_var.cpu()}}

    # a resumed run continues the data stream after the batches the interrupted run consumed
    train_loader, valid_loader = create_dataloaders(args, info.rank, info.world_size, resumed.batches,
                                                    device_augment=C.use_device_augment(args, device),
                                                    device_valid=C.use_device_valid(args, device))
    result = {}
    step = start

    def evaluate_with_report(model, ema, loader):
        """``evaluate`` / ``evaluate_ema`` at the current step, with the --eval-report values merged in."""
        report = make_report(args, model, device)
        if ema is None:
            res = evaluate(model, loader, rngs, device, report)
        else:
            res = evaluate_ema(model, ema, loader, rngs, device, report)
        if report is not None:
            res.update(finish_report(report, args, step, log, "" if ema is None else "ema_"))
        return res

    logger = Logger(args.output_dir, args.name, args.project, vars(args), enabled=info.is_main,
                    use_wandb=False if args.log_file_only else None)
    if valid_loader is not None:  # SANITATION CHECK (main_finetune.py:53-54)
        result.update(evaluate_with_report(model, None, valid_loader))
        if ema is not None:
            result.update(evaluate_with_report(model, ema, valid_loader))
            result["val/ema_acc1/best"] = resumed.best("val/ema_acc1", 0.0)  # nothing is saved here
        if teacher is not None:  # here and only here
            result.update(evaluate_teacher(teacher, valid_loader, rngs, device))
        if args.attn_stats > 0 and info.is_main:
            result.update(C.evaluate_attn_stats(model, valid_loader, args, device, log))
        if args.attn_maps > 0 and info.is_main:
            result.update(C.evaluate_attn_maps(model, valid_loader, args, device, start, log))
        logger.log(dict(result), start)
        log(f"[eval] step {start} {result}")
    meter = AverageMeter(use_latest=["learning_rate"])
    max_acc1 = resumed.best("val/acc1", 0.0)
    max_ema_acc1 = resumed.best("val/ema_acc1", 0.0)

    def best():
        return {"val/acc1": max_acc1, **({"val/ema_acc1": max_ema_acc1} if ema is not None else {})}

    it = C.DevicePrefetcher(train_loader, device) if train_loader is not None else None
    t0 = time.time()
    perf = C.PerfClock(start, args.train_batch_size, finetune_fwd_flops_per_image(model.cfg), info.world_size)
    step = start
    for step in range(start + 1, args.training_steps + 1):
        micro = [tuple(next(it)) for _ in range(args.grad_accum)]
        log_step = args.log_interval > 0 and step % args.log_interval == 0
        if monitor is not None and log_step:
            monitor.begin()  # the weights this step starts from
        metrics = run_step(micro)
        meter.update(**metrics)
        if log_step:
            summ = meter.summary("train/")
            summ["processed_samples"] = step * args.train_batch_size
            summ.update(perf.summary(step))
            comm = trainer.comm_ms()
            if comm is not None:
                summ["perf/comm_ms"] = comm
            if monitor is not None:  # this step's own values, not a mean over the interval
                log_norms(monitor, summ, log)
            C.check_finite(summ, step)
            if info.is_main:
                logger.log(summ, step)
                log(f"[train] step {step} " + " ".join(f"{k}={v:.5g}" for k, v in summ.items()))
        do_eval = args.eval_interval > 0 and (step % args.eval_interval == 0 or step == args.training_steps)
        stop = C.stop_here(args, step, start)
        do_save = do_eval or stop or (args.save_interval > 0 and step % args.save_interval == 0)
        # every rank's random state (collective), then rank 0 writes; "last" is written after the
        # evaluation so that its sidecar carries the updated best metric
        per_rank = C.rank_states(rngs, model) if do_save else None
        if do_eval and valid_loader is not None:
            res = evaluate_with_report(model, None, valid_loader)
            if res["val/acc1"] > max_acc1:  # identical on every rank (all-reduced)
                max_acc1 = res["val/acc1"]
                C.save_last(args, model, opt, step, rngs, extra(), postfix="best", per_rank=per_rank,
                            best=best(), ema=ema)
            if ema is not None:
                res.update(evaluate_with_report(model, ema, valid_loader))
                if res["val/ema_acc1"] > max_ema_acc1:  # identical on every rank (all-reduced)
                    max_ema_acc1 = res["val/ema_acc1"]
                    save_ema_best(args, model, ema)
            if info.is_main:
                if args.attn_stats > 0:
                    res.update(C.evaluate_attn_stats(model, valid_loader, args, device, log))
                if args.attn_maps > 0:
                    res.update(C.evaluate_attn_maps(model, valid_loader, args, device, step, log))
                res["val/acc1/best"] = max_acc1
                if ema is not None:
                    res["val/ema_acc1/best"] = max_ema_acc1
                res["processed_samples"] = step * args.train_batch_size
                logger.log(res, step)
                log(f"[eval] step {step} {res}")
            result.update(res)
        if do_save:
            C.save_last(args, model, opt, step, rngs, extra(), per_rank=per_rank, best=best(), ema=ema)
        if stop:
            log(f"[train] --stop-after-steps: stopping at step {step}")
            break
    C.flush_checkpoints()
    result["train_time_s"] = time.time() - t0
    result["final_step"] = step
    logger.close()
    return result


def cli(argv=None):
    args = finetune_parser().parse_args(argv)
    out = main(args)
    pdist.cleanup()
    return out


if __name__ == "__main__":
    cli()
