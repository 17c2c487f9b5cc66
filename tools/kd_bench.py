"""Distillation loss on the GPU: the two kernels of csrc/distill.hip (ops.functional.kd_loss) against the
torch composition kd_loss_torch, forward + backward at [B, L] bf16, and -- with --step -- the ViT-B
finetune step of bench.py's finetune task with a frozen teacher attached (profiles/distill.txt).

    python tools/kd_bench.py [--batch 128 --labels 1000 --iters 200]
    python tools/kd_bench.py --step [--teacher vit_large_patch16|vit_base_patch16|none] [--batch 128 --steps 30]"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jumbo_mae_tpu_amd.ops import functional as Fn  # noqa: E402
from jumbo_mae_tpu_amd.ops import prims as P  # noqa: E402

SHAPES = {"vit_base_patch16": (12, 768, 12), "vit_large_patch16": (24, 1024, 16)}


def _time(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def kernels(a):
    g = torch.Generator().manual_seed(0)
    z = (4.0 * torch.randn(a.batch, a.labels, generator=g)).bfloat16().cuda().requires_grad_(True)
    u = (4.0 * torch.randn(a.batch, a.labels, generator=g)).bfloat16().cuda()
    w = torch.full((a.batch,), 1.0 / a.batch, device="cuda")
    for mode in ("soft", "hard"):
        row = {"shape": [a.batch, a.labels], "dtype": "bf16", "mode": mode, "T": a.temperature}
        for on in (False, True):
            P._KD_OURS = on

            def fwd_bwd():
                kd, _ = Fn.kd_loss(z, u, a.temperature, mode)
                torch.autograd.grad(kd, z, w)

            row["ours_us" if on else "torch_us"] = round(_time(fwd_bwd, a.iters), 2)
        print(json.dumps(row), flush=True)


def step(a):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.mixup import Mixup
    from jumbo_mae_tpu_amd.utils.rng import RngStreams
    kw = dict(labels=1000, image_size=224, patch_size=16, posemb="learnable")
    L, D, H = SHAPES["vit_base_patch16"]
    s = FinetuneModel(ViTConfig(layers=L, dim=D, heads=H, droppath=0.1, **kw), Mixup(0.8, 1.0, seed=0),
                      label_smoothing=0.1).to("cuda", torch.bfloat16, seed=0)
    if a.teacher != "none":
        L, D, H = SHAPES[a.teacher]
        t = FinetuneModel(ViTConfig(layers=L, dim=D, heads=H, **kw)).freeze().to("cuda", torch.bfloat16, seed=1)
        s.attach_teacher(t, 0.5, a.temperature, "soft")
    opt = FlatOptimizer(s.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 5, 1000, 1e-6), weight_decay=0.05,
                        lr_decay=0.75, num_layers=s.cfg.layers)
    tr = Trainer(s, opt, None, RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, "cuda"))
    g = torch.Generator().manual_seed(0)
    mb = (torch.randint(0, 256, (a.batch, 3, 224, 224), dtype=torch.uint8, generator=g).cuda(),
          torch.randint(0, 1000, (a.batch,), generator=g).cuda())
    ms = _time(lambda: tr.train_step([mb]), a.steps) / 1e3
    print(json.dumps({"teacher": a.teacher, "batch": a.batch, "ms_per_step": round(ms, 3),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--labels", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--teacher", default="vit_large_patch16", choices=["none"] + sorted(SHAPES))
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    (step if a.step else kernels)(a)


if __name__ == "__main__":
    main()
