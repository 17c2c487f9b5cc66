"""MAE pretraining driver (``main_pretrain``).

Parity: /root/reference/src/main_pretrain.py:37-94 and create_train_state
(/root/reference/src/pretraining.py:170-270):
  * peak LR = learning_rate * train_batch_size / 256, warmup-cosine from 1e-6 to 1e-5;
  * "SANITATION CHECK" validation before training (skipped when there is no validation set, Q8);
  * metrics averaged over log_interval with the latest learning_rate, keys train/loss,
    train/learning_rate, processed_samples, val/loss, val/loss/best;
  * at eval_interval (and the last step): evaluates, saves ``{name}-best.msgpack`` on a new minimum
    validation loss and ``{name}-last.msgpack`` (the reference writes "last" before the evaluation;
    here it follows it so that its resume sidecar carries the updated best metric);
  * ``--log-norms global|layer`` (extension): gradient / weight / update norms of every logged step
    (optim/monitor.py), written before the non-finite check so that an abort names its leaves;
  * ``--attn-stats N`` (extension): at every evaluation rank 0 logs the per-layer attention entropy,
    largest logit, largest probability and CLS mass of the first N validation images (ops/attn_stats.py);
  * ``--feat-stats`` (extension): at every evaluation the label-free representation monitor -- effective rank,
    participation ratio and uniformity of the encoder features of the whole validation set (ops/feat_stats.py);
  * ``--attn-maps N`` (extension): at every evaluation rank 0 writes the CLS attention maps of the first N
    validation images (unmasked) as a PNG panel and logs their entropy and CLS mass (ops/attn_maps.py).
Launch: ``torchrun --nproc-per-node 8 src/main_pretrain.py <reference flags>``.
"""

from __future__ import annotations

import time

import torch

from ..config import DecoderConfig, ViTConfig
from ..data.loader import create_dataloaders
from ..models.mae import PretrainModel
from ..ops import feat_stats as feat_ops
from ..ops import knn as knn_ops
from ..optim.monitor import log_norms, make_monitor
from ..parallel import dist as pdist
from ..utils.flops import pretrain_fwd_flops_per_image
from ..utils.rng import RngStreams
from ..utils.trace import set_enabled as set_trace_ranges
from . import common as C
from .cli import pretrain_parser
from ..runtime.graph import StepRunner
from .engine import Trainer
from .meter import AverageMeter, Logger


def build_model(args, device, dtype) -> PretrainModel:
    vc = ViTConfig(layers=args.layers, dim=args.dim, heads=args.heads, labels=args.labels, layerscale=args.layerscale,
                   patch_size=args.patch_size, image_size=args.image_size, posemb=args.posemb, pooling=args.pooling,
                   rope_theta=args.rope_theta, qk_norm=args.qk_norm, ffn=args.ffn,
                   dropout=args.dropout, droppath=args.droppath, grad_ckpt=args.grad_ckpt,
                   image_mask_ratio=args.image_mask_ratio, linear_probing=False)
    dc = DecoderConfig(dec_layers=args.dec_layers, dec_dim=args.dec_dim, dec_heads=args.dec_heads,
                       dec_layerscale=args.dec_layerscale, dec_posemb=args.dec_posemb, dec_qk_norm=args.dec_qk_norm,
                       dec_ffn=args.dec_ffn,
                       dec_dropout=args.dec_dropout,
                       dec_droppath=args.dec_droppath, grad_ckpt=args.grad_ckpt, patch_size=args.patch_size,
                       image_size=args.image_size)
    return PretrainModel(vc, dc, norm_pix_loss=args.norm_pix_loss,
                         mask_mode=getattr(args, "mask_mode", "shared")).to(device, dtype, seed=args.init_seed)


def evaluate(model, loader, rngs, device, knn_k: int = 0, knn_T: float = 0.07, log=None, feat_stats: bool = False,
             feat_t: float = 2.0) -> dict:
    """val/loss, with ``knn_k`` > 0 (--knn-k) the k-NN monitor's val/knn_acc1 / val/knn_acc5 and with
    ``feat_stats`` (--feat-stats) the representation monitor's val/feat_* from the same pass over the
    validation shard (``knn_metrics``, ``FeatMonitor``); the features are extracted once for both."""
    rngs = rngs.fork()  # validation never advances the training streams
    sums = None
    feats, labs = [], []
    monitor = FeatMonitor(feat_t) if feat_stats else None
    for batch in C.DevicePrefetcher(loader, device):
        images, labels = batch if isinstance(batch, (list, tuple)) else (batch, None)
        valid = (labels != -1) if labels is not None else None
        m = model.evaluate(images, valid, rngs.as_dict())
        sums = m if sums is None else {k: sums[k] + m[k] for k in m}
        knn = knn_k > 0 and labels is not None
        if knn or monitor is not None:  # deterministic, no random stream: the loss above is unchanged
            f = model.features(images)
            rows = knn_ops.normalize_features(f)
            if knn:
                feats.append(rows)
                labs.append(labels.to(torch.int64))
            if monitor is not None:
                monitor.update(f, rows, valid)
    packed = torch.stack([sums["loss"], sums["num_samples"]]).float()
    pdist.all_reduce_sum_(packed)
    loss, n = packed.tolist()
    out = {"val/loss": loss / max(n, 1.0)}
    if knn_k > 0:
        if feats:
            out.update(knn_metrics(torch.cat(feats), torch.cat(labs), knn_k, knn_T))
        elif log is not None:
            log("[eval] --knn-k: the validation loader yields no labels, k-NN monitor skipped")
    if monitor is not None:
        out.update(monitor.finish())
    return out


def gather_rows(feats: torch.Tensor, tags: torch.Tensor, pad: int):
    """All-gather of this rank's rows ``feats`` [n, D] and their int64 ``tags`` [n], each shard padded
    to the longest one with zero rows tagged ``pad`` (collective).  Returns (bank, bank_tags,
    self_idx): the gathered rows in rank order and the bank index of each of this rank's own rows.
    One process: the inputs themselves."""
    import torch.distributed as dist

    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    n = feats.shape[0]
    self_idx = torch.arange(n, device=feats.device)
    if world == 1:
        return feats, tags, self_idx
    rank = dist.get_rank()
    longest = torch.tensor([n], dtype=torch.int64, device=feats.device)
    dist.all_reduce(longest, op=dist.ReduceOp.MAX)
    L = int(longest.item())
    f = torch.zeros(L, feats.shape[1], dtype=feats.dtype, device=feats.device)
    y = torch.full((L,), pad, dtype=torch.int64, device=feats.device)
    f[:n], y[:n] = feats, tags
    fw = f.view(torch.uint8)  # the bytes: every backend gathers uint8
    gf = torch.empty(world * L, fw.shape[1], dtype=torch.uint8, device=feats.device)
    gy = torch.empty(world * L, dtype=torch.int64, device=feats.device)
    dist.all_gather(list(gf.chunk(world)), fw)  # the chunks are views: gathered in place, in rank order
    dist.all_gather(list(gy.chunk(world)), y)
    return gf.view(feats.dtype), gy, self_idx + rank * L


def knn_metrics(feats: torch.Tensor, labels: torch.Tensor, k: int, T: float) -> dict:
    """Leave-one-out weighted k-NN accuracy over the whole validation set (collective).

    ``feats`` [n, D] bf16 normalised / ``labels`` [n] (-1 = padding) are this rank's shard.  The
    ranks all-gather both, padded to the longest shard with label -1 (``gather_rows``); each rank
    classifies its own rows against the gathered bank, leaving out the row itself by its global index;
    hit sums and the count travel in one packed all-reduce."""
    bank, bank_labels, self_idx = gather_rows(feats, labels, -1)
    hit1, hit5 = knn_ops.knn_classify(feats, labels, k, T, bank, bank_labels, self_idx)
    packed = torch.stack([hit1.sum(), hit5.sum(), (labels != -1).sum()]).double()
    pdist.all_reduce_sum_(packed)
    h1, h5, cnt = packed.tolist()
    return {"val/knn_acc1": h1 / max(cnt, 1.0), "val/knn_acc5": h5 / max(cnt, 1.0)}


class FeatMonitor:
    """The representation monitor of one evaluation pass (--feat-stats): ``update`` per batch, then
    ``finish`` (collective) returns the val/feat_* metrics of ops/feat_stats.py ``summary``.

    A row counts when the loader does not mark it as padding (label -1; without labels every row
    counts) and all of its features are finite; the others are kept out of the Gram state through
    ``valid`` and out of the uniformity through ``bank_valid``, and the non-finite ones are counted."""

    def __init__(self, t: float = 2.0):
        self.t = float(t)
        self.state = None
        self.rows, self.valid = [], []
        self.nonfinite = None

    def update(self, f: torch.Tensor, rows: torch.Tensor | None = None, valid: torch.Tensor | None = None) -> None:
        """``f`` fp32 [B, D] features, ``rows`` their ``normalize_features`` (computed when None),
        ``valid`` bool [B] (None: every row)."""
        if self.state is None:
            self.state = feat_ops.new_state(f.shape[1], f.device)
            self.nonfinite = torch.zeros(1, dtype=torch.float64, device=f.device)
        real = valid.bool() if valid is not None else torch.ones(f.shape[0], dtype=torch.bool, device=f.device)
        finite = feat_ops.finite_rows(f)
        ok = real & finite
        feat_ops.feat_gram(f, ok, self.state)
        self.nonfinite += (real & ~finite).sum()
        self.rows.append(knn_ops.normalize_features(f) if rows is None else rows)
        self.valid.append(ok)

    def finish(self) -> dict:
        """G, s, n and the non-finite count are all-reduced in fp64; the bf16 rows and their validity
        are all-gathered (``gather_rows``) and each rank sums e over its own rows against the gathered
        bank; e_sum and pairs travel in one packed all-reduce.  Rank 0 alone runs ``summary`` (a copy of
        G to the host and two eigvalsh calls) and broadcasts the few scalars: every rank returns the
        same dict.  Every rank must have seen at least one batch."""
        if self.state is None:
            raise RuntimeError("FeatMonitor.finish: no batch was seen")
        st = self.state
        pdist.all_reduce_sum_(st["G"])
        tail = torch.cat([st["s"], st["n"], self.nonfinite])
        pdist.all_reduce_sum_(tail)
        D = st["s"].shape[0]
        st["s"], st["n"], self.nonfinite = tail[:D], tail[D:D + 1], tail[D + 1:]
        rows, ok = torch.cat(self.rows), torch.cat(self.valid)
        bank, bank_ok, self_idx = gather_rows(rows, ok.to(torch.int64), 0)
        bank_ok = bank_ok != 0
        e = feat_ops.feat_uniformity(rows, bank, self_idx, bank_ok, self.t)
        total = bank_ok.sum().double()
        packed = torch.stack([e[ok].sum(), ok.sum().double() * (total - 1.0)])
        pdist.all_reduce_sum_(packed)
        e_sum, pairs = packed.tolist()
        keys = feat_ops.KEYS
        vals = torch.zeros(2 * len(keys), dtype=torch.float64, device=packed.device)  # values, then presence
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0:
            out = feat_ops.summary(st["G"], st["s"], int(st["n"].item()), e_sum, pairs, int(self.nonfinite.item()))
            vals = torch.tensor([out.get(k, 0.0) for k in keys] + [float(k in out) for k in keys],
                                dtype=torch.float64, device=packed.device)
        pdist.broadcast_(vals)
        vals = vals.tolist()
        return {k: v for k, v, have in zip(keys, vals, vals[len(keys):]) if have}


first_images = C.first_images


def recon_panel(images_u8: torch.Tensor, out: dict):
    """PIL image with one row per input image: original | masked | reconstruction | pasted."""
    import numpy as np
    from PIL import Image

    cols = [images_u8, out["masked"], out["recon"], out["paste"]]
    rows = torch.cat([c.permute(0, 2, 3, 1) for c in cols], 2)  # [B, S, 4 S, 3]
    return Image.fromarray(np.ascontiguousarray(rows.reshape(-1, rows.shape[2], 3).cpu().numpy()))


def evaluate_recon(model, loader, args, device, step: int, log) -> dict:
    """--recon-images (rank 0 only, no collectives): reconstructs the first N validation images
    under a mask drawn from a private generator seeded with --noise-seed -- the same patches at
    every evaluation, and nothing taken from the training streams -- writes
    ``{output_dir}/{name}-recon-{step:07d}.png`` and returns ``val/psnr_masked`` (their mean)."""
    from ..utils import gopen

    with torch.random.fork_rng(devices=[]):  # a loader iterator seeds its workers from the default generator
        images = first_images(loader, args.recon_images, device)
    B, n = images.shape[0], model.cfg.seq_patches
    g = torch.Generator().manual_seed(args.noise_seed)
    noise = torch.rand((n,) if model.mask_mode == "shared" else (B, n), generator=g).to(device)
    out = model.reconstruct(images, noise=noise)
    if gopen.is_local(args.output_dir or "."):
        import os

        os.makedirs(args.output_dir or ".", exist_ok=True)
        path = os.path.join(args.output_dir or ".", f"{args.name or 'run'}-recon-{step:07d}.png")
        recon_panel(images, out).save(path)
    else:
        log(f"[eval] --recon-images: remote --output-dir {args.output_dir}, reconstruction PNG skipped")
    return {"val/psnr_masked": float(out["psnr_masked"].mean())}


def main(args) -> dict:
    if args.knn_k:
        knn_ops.check_k(args.knn_k)  # before any work: 1..64
        if not args.knn_temperature > 0:
            raise ValueError(f"--knn-temperature must be positive (got {args.knn_temperature})")
    if args.feat_stats and not args.feat_uniformity_t > 0:  # before any work
        raise ValueError(f"--feat-uniformity-t must be positive (got {args.feat_uniformity_t})")
    info = pdist.init_distributed(args.device)
    set_trace_ranges(args.trace_ranges)
    device = info.device
    log = print if info.is_main else (lambda *a, **k: None)
    dtype = C.compute_dtype(args, device)
    model = build_model(args, device, dtype)
    pdist.broadcast_(model.store.master)  # CC6: identical initial params on every rank
    model.store.sync_shadow()
    C.summarize_params(model.store, log)
    opt = C.make_optimizer(args, model.store, args.learning_rate * args.train_batch_size / 256, 1e-5)
    reducer = C.make_reducer(args, model.store)
    rngs = RngStreams({"mixup": args.mixup_seed, "dropout": args.dropout_seed, "noise": args.noise_seed},
                      info.rank, device)
    trainer = Trainer(model, opt, reducer, rngs, args.grad_accum, skip_nonfinite=args.skip_nonfinite)
    run_step = StepRunner(trainer, hip_graph=args.hip_graph and device.type == "cuda" and info.world_size == 1)
    resumed = C.maybe_resume(args, model, opt, rngs, log)
    start = resumed.step
    monitor = make_monitor(args, opt)  # --log-norms

    # a resumed run continues the data stream after the batches the interrupted run consumed
    train_loader, valid_loader = create_dataloaders(args, info.rank, info.world_size, resumed.batches,
                                                    device_augment=C.use_device_augment(args, device),
                                                    device_valid=C.use_device_valid(args, device))
    result = {}
    logger = Logger(args.output_dir, args.name, args.project, vars(args), enabled=info.is_main,
                    use_wandb=False if args.log_file_only else None)
    if valid_loader is not None:  # SANITATION CHECK (main_pretrain.py:53-54), skipped without a valid set (Q8)
        result.update(evaluate(model, valid_loader, rngs, device, args.knn_k, args.knn_temperature, log,
                               args.feat_stats, args.feat_uniformity_t))
        if args.recon_images > 0 and info.is_main:
            result.update(evaluate_recon(model, valid_loader, args, device, start, log))
        if args.attn_stats > 0 and info.is_main:
            result.update(C.evaluate_attn_stats(model, valid_loader, args, device, log))
        if args.attn_maps > 0 and info.is_main:
            result.update(C.evaluate_attn_maps(model, valid_loader, args, device, start, log))
        logger.log(dict(result), start)
        log(f"[eval] step {start} {result}")
    meter = AverageMeter(use_latest=["learning_rate"])
    min_val_loss = resumed.best("val/loss", 1e9)
    it = C.DevicePrefetcher(train_loader, device) if train_loader is not None else None
    t0 = time.time()
    perf = C.PerfClock(start, args.train_batch_size, pretrain_fwd_flops_per_image(model.cfg, model.dec_cfg),
                       info.world_size)
    step = start
    for step in range(start + 1, args.training_steps + 1):
        micro = []
        for _ in range(args.grad_accum):
            b = next(it)
            micro.append((b[0] if isinstance(b, (list, tuple)) else b,))
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
            res = evaluate(model, valid_loader, rngs, device, args.knn_k, args.knn_temperature, log,
                           args.feat_stats, args.feat_uniformity_t)
            if res["val/loss"] < min_val_loss:  # identical on every rank (all-reduced)
                min_val_loss = res["val/loss"]
                C.save_last(args, model, opt, step, rngs, postfix="best", per_rank=per_rank,
                            best={"val/loss": min_val_loss})
            if info.is_main:
                if args.recon_images > 0:
                    res.update(evaluate_recon(model, valid_loader, args, device, step, log))
                if args.attn_stats > 0:
                    res.update(C.evaluate_attn_stats(model, valid_loader, args, device, log))
                if args.attn_maps > 0:
                    res.update(C.evaluate_attn_maps(model, valid_loader, args, device, step, log))
                res["val/loss/best"] = min_val_loss
                res["processed_samples"] = step * args.train_batch_size
                logger.log(res, step)
                log(f"[eval] step {step} {res}")
            result.update(res)
        if do_save:
            C.save_last(args, model, opt, step, rngs, per_rank=per_rank, best={"val/loss": min_val_loss})
        if stop:
            log(f"[train] --stop-after-steps: stopping at step {step}")
            break
    C.flush_checkpoints()
    result["train_time_s"] = time.time() - t0
    result["final_step"] = step
    logger.close()
    return result


def cli(argv=None):
    args = pretrain_parser().parse_args(argv)
    out = main(args)
    pdist.cleanup()
    return out


if __name__ == "__main__":
    cli()
