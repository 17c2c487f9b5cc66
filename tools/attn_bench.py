"""Time the fused attention kernels at the flagship shapes (MAE decoder / Jumbo encoder) and the
tile-streamed kernels at the ViT-H/14 shapes (head dim 80) beside the PyTorch composition.

    python tools/attn_bench.py [--iters N] [--shapes dec,enc]
    python tools/attn_bench.py --shapes vith_enc --torch     # adds the composition column
    python tools/attn_bench.py --shapes vith_ft --dropout 0.1   # attention-probability dropout

Prints one line per (shape, pass) with us/call and achieved TFLOP/s (useful flops only).  With
``--torch`` each line also carries the time of ``ops/prims.py`` attn_fwd / attn_bwd with the HIP
route disabled in-process -- the composition with fp32 [B, H, S, S] score tensors, the path of
head dims without kernels -- and a last line per shape gives forward + backward and the peak
memory (torch.cuda.max_memory_allocated) of one forward + backward each way.  With ``--dropout RATE``
the same calls carry a seed (the mask is regenerated in the kernels; the composition builds it on
the CPU, ops/prims.py _drop_mask) and no fused bias gradient is requested.  Times are medians of
``--reps`` windows of ``--iters`` calls after a warm-up; run one shape per process to compare
shapes."""

import argparse
import os
import statistics
import sys

import torch

# JMAE_ROOT: package tree to import (A/B of two builds, tools/run_attn_ab.sh)
sys.path.insert(0, os.environ.get("JMAE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jumbo_mae_tpu_amd.ops import _ext  # noqa: E402
from jumbo_mae_tpu_amd.ops import prims as P  # noqa: E402

SHAPES = {"dec": (512, 199, 16, 32), "dec2k": (2048, 199, 16, 32), "enc": (512, 52, 16, 64), "enc2k": (2048, 52, 16, 64), "ft": (128, 199, 16, 64), "ft12": (128, 199, 12, 64),
          # ViT-H/14 at 224 px: encoder pretrain (64 kept + 3 CLS), finetune (256 + 3), and one hd-128 shape
          "vith_enc": (64, 67, 16, 80), "vith_ft": (32, 259, 16, 80), "hd128": (32, 199, 8, 128),
          # finetune at 448 px (ViT-B/16): 784 + 3 tokens
          "ft448": (8, 787, 12, 64)}


def _time(fn, iters, reps):
    res = []
    for _ in range(reps):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(res)


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


class _composition:
    """ops/prims.py with the HIP attention route switched off for the duration."""

    def __enter__(self):
        self.saved = P._attn_hip
        P._attn_hip = lambda qkv, heads: False

    def __exit__(self, *exc):
        P._attn_hip = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="dec,enc")
    ap.add_argument("--torch", action="store_true", help="also time the PyTorch composition (ops/prims.py, HIP route off)")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="RATE",
                    help="attention-probability dropout at this rate (0: none)")
    a = ap.parse_args()
    ext = _ext.load()
    for name in a.shapes.split(","):
        B, S, H, hd = SHAPES[name]
        D = H * hd
        qkv = (torch.randn(B, S, 3 * D, device="cuda") * 1.5).bfloat16()
        do = torch.randn(B, S, D, device="cuda").bfloat16()
        db = torch.zeros(3 * D, device="cuda") if ext.attn_fused_bias(S, hd) and not a.dropout else None
        seed = torch.tensor([0x5EED_1234_5678], dtype=torch.int64, device="cuda") if a.dropout else None
        drop = (seed, a.dropout) if a.dropout else None
        o, lse = ext.attn_fwd(qkv, H, seed, a.dropout)
        fl_f = 4.0 * B * H * S * S * hd
        tot = [0.0, 0.0]
        if a.dropout:
            name = f"{name}+drop{a.dropout:g}"
        for label, fn, tfn, fl in (("fwd", lambda: ext.attn_fwd(qkv, H, seed, a.dropout),
                                    lambda: P.attn_fwd(qkv, H, drop=drop), fl_f),
                                   ("bwd", lambda: ext.attn_bwd(do, qkv, o, lse, H, db, seed, a.dropout),
                                    lambda: P.attn_bwd(do, qkv, o, lse, H, drop=drop), 2.5 * fl_f)):
            us = _time(fn, a.iters, a.reps)
            tot[0] += us
            line = f"{name} {label} B={B} S={S} H={H} hd={hd}: {us:8.1f} us  {fl / us / 1e6:7.1f} TF/s"
            if a.torch:
                with _composition():
                    ut = _time(tfn, a.iters, a.reps)
                tot[1] += ut
                line += f"   composition {ut:8.1f} us  ({ut / us:5.2f}x)"
            print(line, flush=True)
        if a.torch:
            def both():
                o2, l2 = P.attn_fwd(qkv, H, drop=drop)
                P.attn_bwd(do, qkv, o2, l2, H, drop=drop)

            m_hip = _peak_mib(both)
            with _composition():
                m_t = _peak_mib(both)
            print(f"{name} fwd+bwd: hip {tot[0]:8.1f} us  composition {tot[1]:8.1f} us  ({tot[1] / tot[0]:5.2f}x)   "
                  f"peak memory above the inputs: hip {m_hip:7.1f} MiB  composition {m_t:7.1f} MiB", flush=True)


if __name__ == "__main__":
    main()
