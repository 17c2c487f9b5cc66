"""Pieces shared by the pretrain and finetune drivers."""

from __future__ import annotations

import time

import torch

from ..ckpt.checkpoint import ckpt_path, load_params, load_resume_state, save_params, save_resume_state, writer
from ..optim.flat import FlatOptimizer
from ..optim.schedule import warmup_cosine_decay_schedule
from ..parallel import dist as pdist
from ..parallel.ddp import GradReducer
from ..utils import gopen


def pick_device(args) -> torch.device:
    return pdist.info().device


def compute_dtype(args, device) -> torch.dtype:
    if args.compute_dtype == "fp32" or (args.compute_dtype == "auto" and device.type != "cuda"):
        return torch.float32
    return torch.bfloat16


def summarize_params(store, log=print):
    """module.tabulate equivalent (pretraining.py:214): per-subtree parameter counts."""
    groups: dict[str, int] = {}
    for s in store.segments:
        key = "/".join(s.path[:2]) if s.path[0] == "model" else s.path[0]
        groups[key] = groups.get(key, 0) + s.numel
    width = max(len(k) for k in groups) + 2
    lines = [f"{'subtree'.ljust(width)}params"] + [f"{k.ljust(width)}{v:,}" for k, v in groups.items()]
    lines.append(f"{'TOTAL'.ljust(width)}{store.num_params():,} (trainable {store.num_params(True):,})")
    log("\n".join(lines))


def make_optimizer(args, store, peak_lr: float, end_value: float) -> FlatOptimizer:
    log = print if pdist.info().is_main else (lambda *a, **k: None)
    log(f"Peak learning rate: {peak_lr:.1e}")
    sched = warmup_cosine_decay_schedule(1e-6, peak_lr, args.warmup_steps, args.training_steps, end_value)
    return FlatOptimizer(store, args.optimizer, sched, b1=args.adam_b1, b2=args.adam_b2, eps=args.adam_eps,
                         weight_decay=args.weight_decay, lr_decay=args.lr_decay, num_layers=args.layers,
                         clip_grad=args.clip_grad)


def make_reducer(args, store):
    if pdist.info().world_size > 1 or pdist.forced_group():
        dt = torch.bfloat16 if getattr(args, "reduce_dtype", "fp32") == "bf16" else torch.float32
        return GradReducer(store, bucket_mb=args.bucket_mb, reduce_dtype=dt,
                           shard=getattr(args, "shard_optimizer", False),
                           gather_dtype=getattr(args, "zero1_gather", "bf16"))
    return None


def use_device_augment(args, device) -> bool:
    """--device-augment: auto = on a GPU with the extension and the pretraining train transform
    (RandomResizedCrop + flip only); on = additionally RandAugment / AutoAugment / ColorJitter after
    the crop (the finetune presets), and an error for what stays on the host; all = additionally
    AugMix and random erasing (the default finetune flags), and an error for --random-crop src|none."""
    from ..data.loader import device_augment_all_ok, device_augment_ok, device_augment_rrc_only
    mode = getattr(args, "device_augment", "off")
    if mode == "off" or device.type != "cuda" or not getattr(args, "train_dataset_shards", None):
        return False
    if mode == "on" and not device_augment_ok(args):
        raise SystemExit("--device-augment on: AugMix (--auto-augment augmix-*), --random-erasing > 0 and "
                         "--random-crop src|none are not covered by the device augment; they run on the host "
                         "(--device-augment off; --device-augment all covers AugMix and random erasing)")
    if mode == "all" and not device_augment_all_ok(args):
        raise SystemExit("--device-augment all: --random-crop src|none are not covered by the device augment; "
                         "they run on the host (--device-augment off)")
    if mode not in ("on", "all") and not device_augment_rrc_only(args):
        return False
    from ..ops import _ext
    if not _ext.available():  # no built extension (JMAE_ALLOW_TORCH_FALLBACK runs): the PIL path
        if mode in ("on", "all"):
            raise SystemExit(f"--device-augment {mode} needs the built HIP extension "
                             "(python -m jumbo_mae_tpu_amd.csrc.build)")
        return False
    return True


def use_device_valid(args, device) -> bool:
    """--device-augment auto | on | all also runs the validation transform (Resize -> CenterCrop) on the
    GPU -- bit-exact to PIL, so no metric changes: on a GPU with the extension, with validation
    shards, while the centre crop lies inside the resized image (``device_valid_ok``).  Raises for
    nothing: what it does not cover stays on the host."""
    from ..data.loader import device_valid_ok
    mode = getattr(args, "device_augment", "off")
    if mode == "off" or device.type != "cuda" or not getattr(args, "valid_dataset_shards", None):
        return False
    if not device_valid_ok(args):
        return False
    from ..ops import _ext
    return bool(_ext.available())


class DevicePrefetcher:
    """Moves the next host batch to the device on a side stream while the current step runs; a
    device-augment batch (data/loader.py ``PackedImages``) is resized / flipped there too."""

    def __init__(self, it, device):
        self.it = iter(it)
        self.device = device
        self.stream = torch.cuda.Stream(device) if device.type == "cuda" else None
        self.next = None
        self._preload()

    def _to(self, b):
        from ..data.loader import PackedImages, unpack_on_device
        if isinstance(b, PackedImages):
            return unpack_on_device(b, self.device)
        if isinstance(b, (list, tuple)):
            return type(b)(self._to(x) for x in b)
        if isinstance(b, torch.Tensor):
            return b.to(self.device, non_blocking=True)
        return b

    def _preload(self):
        try:
            b = next(self.it)
        except StopIteration:
            self.next = None
            return
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                self.next = self._to(b)
        else:
            self.next = self._to(b)

    def __iter__(self):
        return self

    def __next__(self):
        if self.next is None:
            raise StopIteration
        if self.stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            for t in (self.next if isinstance(self.next, (list, tuple)) else [self.next]):
                if isinstance(t, torch.Tensor):
                    t.record_stream(torch.cuda.current_stream(self.device))
        b = self.next
        self._preload()
        return b


def rank_states(rngs, model) -> list:
    """COLLECTIVE (every rank calls it at the same step): each rank's random state -- its device
    streams (mixup / dropout / noise) and the host Mixup generator -- gathered in rank order.
    Saved in the resume sidecar so that after ``--resume`` every rank continues its OWN streams
    (the reference's per-device ``shard_prng_key`` independence), not rank 0's."""
    mine = {"rngs": rngs.state_dict() if rngs is not None else {}}
    mix = getattr(model, "mixup", None)
    if mix is not None and getattr(mix, "rs", None) is not None:
        mine["mixup_host"] = mix.rs.bit_generator.state
    return pdist.all_gather_object(mine)


def make_ema(args, store, opt, resumed, log=print):
    """--ema-decay D > 0: the weight average (optim/ema.py), created from the weights as they stand --
    after the pretrained load, the broadcast and ``maybe_resume`` -- restored from the resume sidecar
    where that carries one, and attached to the optimizer.  None with the flag off."""
    decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
    if decay <= 0.0:
        return None
    from ..optim.ema import WeightEma
    ema = WeightEma(store, decay)
    if resumed.get("ema") is not None:
        ema.load_state_dict(resumed["ema"])
        log(f"[resume] restored the weight EMA after {ema.updates} updates")
    elif resumed.step > 0:
        log("[resume] no weight EMA in the resume state: the average starts from the restored weights")
    opt.attach_ema(ema)
    return ema


def save_last(args, model, opt, step, rngs, extra_state=None, postfix="last", per_rank=None, best=None, ema=None):
    """Rank 0: params msgpack (Flax tree) + resume sidecar, both written in the background.

    The sidecar holds the optimizer state, every rank's random state (``per_rank`` from
    ``rank_states``), the data position (train batches consumed per rank) and the best
    validation metric so far -- and, with ``ema`` (--ema-decay), the weight average and its update count."""
    if hasattr(opt, "gather_state"):
        opt.gather_state()  # collective: sharded optimizer moments made whole on every rank
    if ema is not None:
        ema.gather()  # collective: and the weight average
    if not pdist.info().is_main:
        return None
    tree = model.flax_params()
    url = save_params(args.output_dir, args.name or "run", tree, postfix)
    state = {"step": step, "optimizer": opt.state_dict(), "rngs": rngs.state_dict() if rngs else {},
             "time": time.time(), "world_size": pdist.info().world_size,
             "data": {"batches_per_rank": step * getattr(args, "grad_accum", 1)}}
    if per_rank is not None:
        state["rngs_per_rank"] = per_rank
    if best is not None:
        state["best"] = dict(best)
    if ema is not None:
        state["ema"] = ema.state_dict()
    if extra_state:
        state.update(extra_state)
    save_resume_state(ckpt_path(args.output_dir, args.name or "run", postfix, "state.pt"), state)
    return url


class Resumed(dict):
    """What ``maybe_resume`` restored: step, data position and best metrics (empty = fresh run)."""

    @property
    def step(self) -> int:
        return int(self.get("step", 0))

    @property
    def batches(self) -> int:
        return int(self.get("data", {}).get("batches_per_rank", 0))

    def best(self, key: str, default: float) -> float:
        return float(self.get("best", {}).get(key, default))


def maybe_resume(args, model, opt, rngs, log=print) -> Resumed:
    """--resume auto|<prefix>: restore params, optimizer moments/count, this rank's RNG streams and
    host Mixup generator; returns the step, data position and best metrics (``Resumed``)."""
    if not args.resume:
        return Resumed()
    prefix = gopen.join(args.output_dir, f"{args.name or 'run'}-last") if args.resume == "auto" else args.resume
    pfile, sfile = prefix + ".msgpack", prefix + ".state.pt"
    if not (gopen.exists(pfile) and gopen.exists(sfile)):
        log(f"[resume] nothing to resume at {prefix}")
        return Resumed()
    model.store.load_flax_tree(load_params(pfile), strict=True)
    st = load_resume_state(sfile)
    opt.load_state_dict(st["optimizer"])
    info = pdist.info()
    per_rank = st.get("rngs_per_rank")
    if per_rank is not None and len(per_rank) == info.world_size:
        mine = per_rank[info.rank]
        if rngs is not None and mine.get("rngs"):
            rngs.load_state_dict(mine["rngs"])
        mix = getattr(model, "mixup", None)
        if mine.get("mixup_host") is not None and mix is not None and getattr(mix, "rs", None) is not None:
            mix.rs.bit_generator.state = mine["mixup_host"]
    elif rngs is not None:
        # saved with another world size (or by an older version): fresh per-rank streams keyed by
        # the step, so ranks stay independent and do not replay the first steps' draws
        rngs.reseed(int(st["step"]))
        log("[resume] world size changed or no per-rank RNG state: streams re-derived from (seed, rank, step)")
    if "batch_stats" in st and hasattr(model, "head") and getattr(model.head, "running_mean", None) is not None:
        model.head.running_mean.copy_(st["batch_stats"]["mean"])
        model.head.running_var.copy_(st["batch_stats"]["var"])
    pdist.broadcast_(model.store.master)
    model.store.sync_shadow()
    log(f"[resume] restored step {st['step']} from {prefix}")
    out = Resumed(step=int(st["step"]), best=st.get("best", {}))
    if st.get("ema") is not None:
        out["ema"] = st["ema"]  # make_ema restores it
    if "data" in st and st.get("world_size", info.world_size) == info.world_size:
        out["data"] = st["data"]
    return out


def stop_here(args, step: int, start: int) -> bool:
    """--stop-after-steps: this invocation has run its share of steps."""
    n = getattr(args, "stop_after_steps", 0)
    return n > 0 and step - start >= n and step < args.training_steps


def flush_checkpoints():
    writer().flush()


def check_finite(metrics: dict, step: int):
    """Non-finite loss detection: abort with a clear message."""
    v = metrics.get("train/loss")
    if v is not None and not (v == v and abs(v) != float("inf")):
        raise FloatingPointError(f"non-finite training loss at step {step}: {v}")


class PerfClock:
    """perf/* log keys: images/sec, step time and MFU over each log window."""

    def __init__(self, start_step: int, global_batch: int, fwd_flops_per_image: float, world_size: int):
        self.t, self.step = time.time(), start_step
        self.batch, self.flops, self.world = global_batch, fwd_flops_per_image, world_size

    def summary(self, step: int) -> dict:
        from ..utils.flops import mfu
        now = time.time()
        dt = max(now - self.t, 1e-9)
        n = max(step - self.step, 1)
        ips = n * self.batch / dt
        self.t, self.step = now, step
        return {"perf/images_per_sec": ips, "perf/step_ms": 1e3 * dt / n,
                "perf/mfu": mfu(ips, self.flops, self.world)}


def first_images(loader, n: int, device) -> torch.Tensor:
    """The first ``n`` real (unpadded) images of a validation loader, uint8 [<= n, 3, S, S]."""
    got, have = [], 0
    for batch in DevicePrefetcher(loader, device):
        images, labels = batch if isinstance(batch, (list, tuple)) else (batch, None)
        if labels is not None:
            images = images[labels != -1]
        got.append(images[:n - have])
        have += got[-1].shape[0]
        if have >= n:
            break
    return torch.cat(got)


def evaluate_attn_stats(model, loader, args, device, log) -> dict:
    """--attn-stats (rank 0 only, no collectives): the attention monitor's probe pass on the first N
    validation images -- for a model that masks (``mask_mode``) under a mask drawn from a private
    generator seeded with --noise-seed, the same patches at every evaluation.  Nothing is taken from
    the training streams.  Returns the ``attn/...`` and ``val/attn_...`` log values
    (ops/attn_stats.py summarize) and prints one line per head with rows of no finite entropy."""
    from ..ops import attn_stats as AS

    with torch.random.fork_rng(devices=[]):  # a loader iterator seeds its workers from the default generator
        images = first_images(loader, args.attn_stats, device)
    if hasattr(model, "mask_mode"):
        B, n = images.shape[0], model.cfg.seq_patches
        g = torch.Generator().manual_seed(args.noise_seed)
        noise = torch.rand((n,) if model.mask_mode == "shared" else (B, n), generator=g).to(device)
        tables = model.attention_stats(images, noise=noise)
    else:
        tables = model.attention_stats(images)
    vals, lines = AS.summarize(tables)
    for line in lines:
        log("[eval] " + line)
    return vals


def attn_map_ramp():
    """The fixed colour ramp of the attention overlays, uint8 [256, 3]: piecewise linear through black,
    purple, red, orange, yellow, white."""
    import numpy as np

    stops = np.array([[0, 0, 0], [84, 15, 109], [187, 55, 84], [249, 142, 8], [252, 230, 60], [255, 255, 255]], float)
    x = np.linspace(0.0, len(stops) - 1.0, 256)
    i = np.minimum(x.astype(int), len(stops) - 2)
    f = (x - i)[:, None]
    return np.round(stops[i] * (1.0 - f) + stops[i + 1] * f).astype(np.uint8)


def attn_map_panel(images_u8: torch.Tensor, maps: torch.Tensor, blend: float = 0.6):
    """PIL image with one row per input image: original | one heat-map overlay per CLS token.  Each map
    ``[gh, gw]`` is divided by its max, nearest-upsampled by the patch size, coloured by ``attn_map_ramp``
    and blended over the image with weight ``blend`` (NumPy and PIL only)."""
    import numpy as np
    from PIL import Image

    img = images_u8.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)  # [B, S, S, 3]
    m = maps.detach().double().cpu().numpy()  # [B, C, gh, gw]
    B, C, gh, gw = m.shape
    ph, pw = img.shape[1] // gh, img.shape[2] // gw
    top = m.reshape(B, C, -1).max(-1)[:, :, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(top > 0, m / top, 0.0)
    idx = np.clip(np.nan_to_num(np.round(u * 255.0), nan=0.0), 0, 255).astype(np.int64)
    heat = attn_map_ramp()[idx].astype(np.float64)  # [B, C, gh, gw, 3]
    heat = heat.repeat(ph, 2).repeat(pw, 3)
    cols = [img]
    for c in range(C):
        over = img.copy()
        over[:, :gh * ph, :gw * pw] = (1.0 - blend) * img[:, :gh * ph, :gw * pw] + blend * heat[:, c]
        cols.append(over)
    rows = np.concatenate(cols, 2)  # [B, S, (1 + C) S, 3]
    return Image.fromarray(np.ascontiguousarray(np.round(rows).astype(np.uint8).reshape(-1, rows.shape[2], 3)))


def attn_map_values(out: dict) -> dict:
    """``val/attn_map_entropy``: the mean over images and CLS tokens of the entropy (nats) of the patch map
    normalised to sum 1; ``val/attn_map_cls_mass``: the mean mass left on the CLS tokens."""
    m = out["maps"].double().flatten(2)
    p = m / m.sum(-1, keepdim=True)
    ent = -torch.where(p > 0, p * torch.log(p), torch.zeros_like(p)).sum(-1)
    return {"val/attn_map_entropy": float(ent.mean()), "val/attn_map_cls_mass": float(out["cls_mass"].double().mean())}


def evaluate_attn_maps(model, loader, args, device, step: int, log) -> dict:
    """--attn-maps (rank 0 only, no collectives): the attention maps (``model.attention_maps``,
    --attn-maps-mode) of the first N validation images, unmasked; writes
    ``{output_dir}/{name}-attn-{step:07d}.png`` and returns ``val/attn_map_entropy`` and
    ``val/attn_map_cls_mass``.  Nothing is taken from the training streams."""
    import os

    with torch.random.fork_rng(devices=[]):  # a loader iterator seeds its workers from the default generator
        images = first_images(loader, args.attn_maps, device)
    out = model.attention_maps(images, mode=args.attn_maps_mode)
    if gopen.is_local(args.output_dir or "."):
        os.makedirs(args.output_dir or ".", exist_ok=True)
        path = os.path.join(args.output_dir or ".", f"{args.name or 'run'}-attn-{step:07d}.png")
        attn_map_panel(images, out["maps"]).save(path)
    else:
        log(f"[eval] --attn-maps: remote --output-dir {args.output_dir}, attention-map PNG skipped")
    return attn_map_values(out)
