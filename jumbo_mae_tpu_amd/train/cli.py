"""Command-line flags, identical in name, spelling and default to the reference drivers.

Reference: /root/reference/src/main_pretrain.py:97-167 and main_finetune.py:97-160 (note the
underscore spelling of ``--image_mask_ratio`` and the seeds defaulting to ``random.randint`` at
parse time).  Additions (all optional, defaults keep reference behaviour): ``--resume``,
``--save-interval``, ``--mask-mode``, ``--compute-dtype``, ``--bucket-mb``, ``--device``,
``--log-norms``, ``--ffn`` / ``--dec-ffn`` (gelu | swiglu, the feed-forward kind), ``--ema-decay``, the
distillation flags ``--teacher-*`` / ``--distill-*`` and ``--eval-report`` / ``--eval-report-bins`` (``main_finetune`` only).
Flags the reference accepts but ignores (``--pooling``, ``--dec-posemb``, ``--label-mapping``,
``--ipaddr``, ``--hostname``; quirk Q10) are accepted and recorded.
"""

from __future__ import annotations

import argparse
import random


def _common(p: argparse.ArgumentParser, mode: str, batch: int, vbatch: int, posemb: str):
    p.add_argument("--mode", default=mode)
    p.add_argument("--train-dataset-shards")
    p.add_argument("--valid-dataset-shards")
    p.add_argument("--train-batch-size", type=int, default=batch)
    p.add_argument("--valid-batch-size", type=int, default=vbatch)
    p.add_argument("--train-loader-workers", type=int, default=40)
    p.add_argument("--valid-loader-workers", type=int, default=5)

    p.add_argument("--random-crop", default="rrc")
    p.add_argument("--color-jitter", type=float, default=0.0)
    p.add_argument("--auto-augment", default="rand-m9-mstd0.5-inc1")
    p.add_argument("--random-erasing", type=float, default=0.25)
    p.add_argument("--augment-repeats", type=int, default=3)
    p.add_argument("--test-crop-ratio", type=float, default=0.875)

    p.add_argument("--mixup", type=float, default=0.8)
    p.add_argument("--cutmix", type=float, default=1.0)
    return p


def _model(p: argparse.ArgumentParser, posemb: str):
    p.add_argument("--layers", type=int, default=12)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--heads", type=int, default=12)
    p.add_argument("--labels", type=int, default=-1)
    p.add_argument("--layerscale", action="store_true", default=False)
    p.add_argument("--patch-size", type=int, default=16)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--posemb", default=posemb,
                   help="learnable | sincos2d | rope -- encoder position embedding: a learnable or fixed sincos2d "
                        "table added at the patch embedding, or rope = axial 2-D rotary embedding of q and k in every "
                        "attention layer (no table, nothing to resize at another --image-size)")
    p.add_argument("--rope-theta", type=float, default=100.0, help="base of the rotary frequencies (--posemb rope)")
    p.add_argument("--qk-norm", choices=("none", "rms"), default="none",
                   help="rms = the encoder's attention RMS-normalises q and k per head before the softmax, with one "
                        "trainable scale each per layer (the remedy for growing attention logits, val/attn_max_logit); "
                        "fused with --posemb rope into one pass.  A checkpoint loads only into a model of the same "
                        "--qk-norm")
    p.add_argument("--ffn", choices=("gelu", "swiglu"), default="gelu",
                   help="feed-forward kind of the encoder, its shared jumbo MLP included: gelu = Dense(4 dim) -> gelu -> "
                        "Dense, swiglu = W2 (silu(W1 x) * (W3 x)) at the parameter-matched hidden width "
                        "ceil((8 dim / 3) / 128) * 128 (768 -> 2048; no width flag), with the new leaves .../ff/w3.  A "
                        "checkpoint loads only into a model of the same --ffn")
    p.add_argument("--pooling", default="cls")
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--droppath", type=float, default=0.1)
    p.add_argument("--grad-ckpt", action="store_true", default=False)


def _optim(p: argparse.ArgumentParser):
    p.add_argument("--optimizer", default="adamw")
    p.add_argument("--learning-rate", type=float, default=1e-3)
    p.add_argument("--weight-decay", type=float, default=0.05)
    p.add_argument("--adam-b1", type=float, default=0.9)
    p.add_argument("--adam-b2", type=float, default=0.999)
    p.add_argument("--adam-eps", type=float, default=1e-8)
    p.add_argument("--lr-decay", type=float, default=1.0)
    p.add_argument("--clip-grad", type=float, default=0.0)
    p.add_argument("--grad-accum", type=int, default=1)

    p.add_argument("--warmup-steps", type=int, default=10000)
    p.add_argument("--training-steps", type=int, default=200000)
    p.add_argument("--log-interval", type=int, default=50)
    p.add_argument("--eval-interval", type=int, default=0)

    p.add_argument("--project")
    p.add_argument("--name")
    p.add_argument("--ipaddr")
    p.add_argument("--hostname")
    p.add_argument("--output-dir", default=".", type=_output_dir)


def _output_dir(v: str) -> str:
    """Checkpoint names are joined onto the output dir, which a ``pipe:`` command cannot take (its
    read command would run with the checkpoint bytes on stdin and write nothing)."""
    if v.startswith("pipe:"):
        raise argparse.ArgumentTypeError("--output-dir cannot be a pipe: command; use a path or gs:// / s3:// URL")
    return v


def _extensions(p: argparse.ArgumentParser):
    g = p.add_argument_group("MI355X framework extensions")
    g.add_argument("--resume", default=None,
                   help="'auto' or a path prefix {output_dir}/{name}-last: resume params + optimizer + step")
    g.add_argument("--save-interval", type=int, default=0, help="also save 'last' every N steps (0: at eval)")
    g.add_argument("--compute-dtype", default="auto", choices=["auto", "bf16", "fp32"])
    g.add_argument("--bucket-mb", type=float, default=64.0,
                   help="data-parallel all-reduce bucket size (tools/allreduce_bench.py recommends one)")
    g.add_argument("--reduce-dtype", default="fp32", choices=["fp32", "bf16"],
                   help="gradient all-reduce dtype (bf16 halves the bytes on xGMI; master weights, "
                        "optimizer state and the local gradient stay fp32)")
    g.add_argument("--shard-optimizer", action="store_true",
                   help="ZeRO-1: reduce-scatter the gradient buckets, update 1/N of the parameters per rank, "
                        "all-gather the updated weights (parallel/ddp.py)")
    g.add_argument("--zero1-gather", default="bf16", choices=["bf16", "fp32"],
                   help="ZeRO-1 weight all-gather: the bf16 compute shadow (fp32 master stays sharded until a "
                        "checkpoint) or the fp32 master (re-cast after the gather)")
    g.add_argument("--stop-after-steps", type=int, default=0,
                   help="end this invocation after N steps, writing 'last' (time-sliced / preemptible "
                        "jobs: continue with --resume auto); 0 = run to --training-steps")
    g.add_argument("--device", default=None, help="cuda|cpu (default: cuda if available)")
    g.add_argument("--device-augment", default="auto", choices=["auto", "on", "all", "off"],
                   help="train transform on the GPU, bit-exact to PIL: RandomResizedCrop + flip and, with 'on', "
                        "RandAugment (rand-*) / AutoAugment policies / --color-jitter after it (auto: on a GPU when the "
                        "train transform is RandomResizedCrop + flip only -- the pretraining presets; on: an error "
                        "for AugMix, --random-erasing > 0 and --random-crop src|none, which stay on the host; all: "
                        "what 'on' covers plus AugMix (augmix-*) and --random-erasing, i.e. the default finetune "
                        "flags, and an error for --random-crop src|none only).  "
                        "auto, on and all also run the validation transform (Resize + CenterCrop) on the GPU, bit-exact "
                        "to PIL, while int(image_size / test_crop_ratio) >= image_size; off keeps everything in "
                        "the loader workers")
    g.add_argument("--log-file-only", action="store_true", help="never use wandb even if installed")
    g.add_argument("--trace-ranges", action="store_true", help="roctx ranges per step phase (rocprofv3 --marker-trace)")
    g.add_argument("--hip-graph", action="store_true",
                   help="capture the whole train step once in a HIP graph and replay it (single process)")
    g.add_argument("--skip-nonfinite", action="store_true",
                   help="skip the update of a step whose loss is non-finite (one host sync per step); "
                        "default: abort at the next log step")
    g.add_argument("--log-norms", default="off", choices=["off", "global", "layer"],
                   help="at every logged step, for that step itself: gradient / weight / update norms from one fused "
                        "fp64 pass over the optimizer's chunk table (optim/monitor.py).  global: train/grad_norm, "
                        "train/param_norm, train/update_norm, train/update_ratio, train/grad_absmax, "
                        "train/nonfinite_grads, train/nonfinite_params (and train/clip_scale with --clip-grad); "
                        "layer: also norms/grad/<group>, norms/param/<group>, norms/update_ratio/<group> per "
                        "layer group.  Non-finite values are counted per leaf and the leaves named before the abort")
    g.add_argument("--attn-stats", type=int, default=0,
                   help="at every evaluation rank 0 runs the first N validation images through the model once more "
                        "(pretraining: masked by a private generator seeded with --noise-seed) and logs, per layer, "
                        "attn/entropy/<layer> (mean row entropy of the attention softmax in nats, averaged over the "
                        "heads; uniform attention = log S), attn/entropy_min/<layer> (the lowest head), "
                        "attn/max_logit/<layer>, attn/max_prob/<layer>, attn/cls_mass/<layer>, and over the layers "
                        "val/attn_entropy_min and val/attn_max_logit (ops/attn_stats.py); 0 = off")
    g.add_argument("--attn-maps", type=int, default=0,
                   help="at every evaluation rank 0 runs the first N validation images (unmasked) through the "
                        "encoder once more, writes {output_dir}/{name}-attn-{step:07d}.png (one row per image: the "
                        "original, then one heat-map overlay per CLS token) and logs val/attn_map_entropy (nats, of "
                        "the patch map normalised to sum 1) and val/attn_map_cls_mass (ops/attn_maps.py); 0 = off")
    g.add_argument("--attn-maps-mode", default="rollout", choices=["rollout", "last"],
                   help="rollout: CLS attention rollout over the encoder's layers (residual weight 0.5); "
                        "last: the head-mean attention of the CLS rows in the last layer")
    return g


def pretrain_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("main_pretrain")
    _common(p, "pretrain", 4096, 512, "sincos2d")
    # reference places --image_mask_ratio right after --mode (main_pretrain.py:100)
    p.add_argument("--image_mask_ratio", type=float, default=0.75)
    _model(p, "sincos2d")
    p.add_argument("--dec-layers", type=int, default=6)
    p.add_argument("--dec-dim", type=int, default=512)
    p.add_argument("--dec-heads", type=int, default=8)
    p.add_argument("--dec-layerscale", action="store_true", default=False)
    p.add_argument("--dec-posemb", default="sincos2d")
    p.add_argument("--dec-qk-norm", choices=("none", "rms"), default="none",
                   help="--qk-norm for the MAE decoder's attention layers")
    p.add_argument("--dec-ffn", choices=("gelu", "swiglu"), default="gelu",
                   help="--ffn for the MAE decoder's blocks")
    p.add_argument("--dec-dropout", type=float, default=0.0)
    p.add_argument("--dec-droppath", type=float, default=0.1)
    p.add_argument("--norm-pix-loss", action="store_true", default=False)
    for s in ("init", "mixup", "dropout", "noise", "shuffle"):
        p.add_argument(f"--{s}-seed", type=int, default=random.randint(0, 1000000))
    _optim(p)
    ext = _extensions(p)
    ext.add_argument("--recon-images", type=int, default=0,
                     help="at every evaluation rank 0 reconstructs the first N validation images (mask from a private "
                          "generator seeded with --noise-seed), writes {output_dir}/{name}-recon-{step:07d}.png "
                          "(original | masked | reconstruction | pasted) and logs val/psnr_masked; 0 = off")
    ext.add_argument("--knn-k", type=int, default=0,
                     help="at every evaluation: weighted k-NN accuracy of the encoder features, leave-one-out on the "
                          "validation set (val/knn_acc1, val/knn_acc5; needs validation labels); 1..64, 0 = off")
    ext.add_argument("--knn-temperature", type=float, default=0.07,
                     help="temperature T of the k-NN vote: neighbour j weighs exp((sim_j - sim_0) / T)")
    ext.add_argument("--feat-stats", action="store_true", default=False,
                     help="at every evaluation: label-free statistics of the encoder features of the whole validation "
                          "set (ops/feat_stats.py): val/feat_rankme (effective rank of the feature matrix), "
                          "val/feat_pr (participation ratio of the covariance spectrum), val/feat_top1_var, "
                          "val/feat_std, val/feat_rms_norm, val/feat_uniformity (log mean exp(-2 t (1 - cos)) over "
                          "pairs of rows), val/feat_rows, val/feat_nonfinite; needs no validation labels")
    ext.add_argument("--feat-uniformity-t", type=float, default=2.0,
                     help="t of val/feat_uniformity (Wang & Isola use 2); must be positive")
    p.add_argument("--mask-mode", default="shared", choices=["shared", "per-sample"],
                   help="shared: one permutation per rank per step (reference, Q1)")
    return p


def finetune_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("main_finetune")
    p.add_argument("--pretrained-ckpt", default=None)
    _common(p, "finetune", 2048, 256, "learnable")
    p.add_argument("--criterion", default="ce")
    p.add_argument("--label-smoothing", type=float, default=0.1)
    _model(p, "learnable")
    for s in ("init", "mixup", "dropout", "shuffle", "noise"):
        p.add_argument(f"--{s}-seed", type=int, default=random.randint(0, 1000000))
    p.add_argument("--label-mapping")
    _optim(p)
    ext = _extensions(p)
    ext.add_argument("--ema-decay", type=_ema_decay, default=0.0,
                     help="exponential moving average of the weights with decay D (warm-up min(D, (1 + t) / (10 + t))), "
                          "updated after every optimizer step: every evaluation also runs with the averaged weights "
                          "(val/ema_loss, val/ema_acc1, val/ema_acc5) and the best of them is written to "
                          "{name}-ema-best.msgpack; 0 <= D < 1, 0 = off")
    ext.add_argument("--teacher-ckpt", default="",
                     help="distillation: a finetune params checkpoint ({name}-best / -last / -ema-best .msgpack of this "
                          "framework or of the reference) loaded into a frozen teacher; the train loss becomes "
                          "(1 - alpha) * loss + alpha * kd and train/cls_loss, train/kd_loss, train/kd_agree are logged; "
                          "the first evaluation also reports val/teacher_acc1 and val/teacher_loss; empty = off")
    ext.add_argument("--teacher-layers", type=int, default=None, help="teacher depth (default: --layers)")
    ext.add_argument("--teacher-dim", type=int, default=None, help="teacher width (default: --dim)")
    ext.add_argument("--teacher-heads", type=int, default=None, help="teacher heads (default: --heads)")
    ext.add_argument("--teacher-layerscale", action="store_true", default=False)
    ext.add_argument("--teacher-ffn", choices=("gelu", "swiglu"), default=None,
                     help="teacher feed-forward kind (default: --ffn)")
    ext.add_argument("--distill-alpha", type=_distill_alpha, default=0.5,
                     help="weight of the distillation term, 0 <= alpha <= 1 (0: the loss without a teacher, bit for "
                          "bit; 1: the teacher alone)")
    ext.add_argument("--distill-temperature", type=_distill_temperature, default=1.0,
                     help="soft mode: T > 0 of kd = T^2 KL(softmax(teacher / T) || softmax(student / T))")
    ext.add_argument("--distill-mode", default="soft", choices=["soft", "hard"],
                     help="soft: temperature-scaled KL to the teacher's distribution; hard (DeiT): cross-entropy "
                          "against the teacher's arg-max class")
    ext.add_argument("--eval-report", action="store_true", default=False,
                     help="every evaluation also reports val/mean_class_acc1, val/mean_class_acc5, "
                          "val/worst_class_acc1, val/ece, val/mce, val/mean_conf, val/classes_seen and "
                          "val/nonfinite_rows (with --ema-decay also val/ema_*), and rank 0 writes "
                          "{name}-report-{step}.json (bins, per-class rows, most confused pairs) and, up to 4096 "
                          "classes, the confusion matrix {name}-confusion-{step}.npy")
    ext.add_argument("--eval-report-bins", type=_eval_report_bins, default=15,
                     help="confidence bins of the calibration metrics (ECE / MCE), 1 <= N <= 64")
    return p


def _eval_report_bins(v: str) -> int:
    n = int(v)
    if not 1 <= n <= 64:
        raise argparse.ArgumentTypeError(f"--eval-report-bins {v}: expected 1 <= N <= 64")
    return n


def _ema_decay(v: str) -> float:
    d = float(v)
    if not 0.0 <= d < 1.0:
        raise argparse.ArgumentTypeError(f"--ema-decay {v}: expected 0 <= D < 1")
    return d


def _distill_alpha(v: str) -> float:
    a = float(v)
    if not 0.0 <= a <= 1.0:
        raise argparse.ArgumentTypeError(f"--distill-alpha {v}: expected 0 <= alpha <= 1")
    return a


def _distill_temperature(v: str) -> float:
    t = float(v)
    if not 0.0 < t < float("inf"):
        raise argparse.ArgumentTypeError(f"--distill-temperature {v}: expected T > 0")
    return t
