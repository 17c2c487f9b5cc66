"""Norm monitor pass (csrc/optim.hip seg_stats kernels, optim/monitor.py) on the ViT-L pretrain store.

    python tools/norm_stats_bench.py [--model vit_large_patch16] [--rounds 5] [--iters 10]

Builds the pretrain model's flat store and its optimizer (no step is run: the gradient is filled with
noise), then times, warm, with device events, in one process:

  collect     ``NormMonitor.collect()``: 12 B read per parameter (p, g, snapshot), two kernels
  begin       ``NormMonitor.begin()``: the snapshot copy, 8 B per parameter
  opt_ema     the weight-EMA pass on the same rows: 8 B read + 4 B written per parameter -- the yardstick
              for a memory-bound pass over the same bytes
  torch       the composition a framework would run on the leaf views: three ``torch._foreach_norm`` calls
              (g, p, p - snapshot through ``torch._foreach_sub``), ``isfinite`` counts and ``abs().max()``
              per leaf
Each figure is the median of ``--rounds`` rounds of ``--iters`` event-timed calls, every round after one
warm-up call; all rounds are printed.
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jumbo_mae_tpu_amd.config import decoder_config, vit_config  # noqa: E402
from jumbo_mae_tpu_amd.models.mae import PretrainModel  # noqa: E402
from jumbo_mae_tpu_amd.ops import _ext  # noqa: E402
from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer  # noqa: E402
from jumbo_mae_tpu_amd.optim.monitor import NormMonitor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_large_patch16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    ext = _ext.load(True)
    dev = torch.device("cuda:0")
    vc = vit_config(a.model, labels=0, posemb="sincos2d", image_mask_ratio=0.75, droppath=0.0, dropout=0.0)
    model = PretrainModel(vc, decoder_config(dec_droppath=0.0)).to(dev, torch.bfloat16, seed=0)
    store = model.store
    opt = FlatOptimizer(store, "adamw", lambda c: 1e-3, b2=0.95, weight_decay=0.05, num_layers=vc.layers)
    mon = NormMonitor(opt, "layer")
    store.grad.copy_(torch.randn(store.total, device=dev) * 1e-3)
    mon.begin()
    store.master.add_(torch.randn(store.total, device=dev) * 1e-4)
    n = store.num_params()
    rows = opt.chunks
    print(f"{a.model} pretrain store: {n:,} parameters in {len(store.segments)} leaves, {rows.shape[0]} chunk rows, "
          f"{torch.cuda.get_device_name(dev)}", flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(name, fn, bytes_per_param):
        ts = []
        for _ in range(a.rounds):
            fn()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        t = statistics.median(ts)
        print(f"{name:8s} {t:9.1f} us  (rounds {', '.join(f'{x:.0f}' for x in ts)})  "
              f"{bytes_per_param * n / t / 1e6:5.2f} TB/s at {bytes_per_param:.0f} B/param", flush=True)
        return t

    def collect():
        mon._armed = True  # every call reads the snapshot, as after a begin()
        return mon.collect()

    t_collect = timed("collect", collect, 12.0)
    t_begin = timed("begin", mon.begin, 8.0)
    ema = store.master.clone()
    ema_hyper = torch.tensor([1e-4], device=dev)
    t_ema = timed("opt_ema", lambda: ext.opt_ema(store.master, ema, rows, opt.meta, ema_hyper), 12.0)
    del ema

    pv = [store.seg_view(store.master, s) for s in store.segments]
    gv = [store.seg_view(store.grad, s) for s in store.segments]
    ov = [store.seg_view(mon.snapshot, s) for s in store.segments]

    def composition():
        gn = torch._foreach_norm(gv)
        pn = torch._foreach_norm(pv)
        dn = torch._foreach_norm(torch._foreach_sub(pv, ov))
        bad = [(~torch.isfinite(x)).sum() for x in gv] + [(~torch.isfinite(x)).sum() for x in pv]
        mx = [x.abs().max() for x in gv]
        return torch.stack(list(gn) + list(pn) + list(dn) + mx), torch.stack(bad)

    t_torch = timed("torch", composition, 12.0)
    print(f"collect / opt_ema = {t_collect / t_ema:.3f}   torch / collect = {t_torch / t_collect:.2f}   "
          f"begin + collect = {t_begin + t_collect:.1f} us per logged step", flush=True)
    stats = collect()
    d = mon.summary(stats)
    print(f"grad_norm {d['train/grad_norm']:.6g}  param_norm {d['train/param_norm']:.6g}  "
          f"update_ratio {d['train/update_ratio']:.3e}  nonfinite {d['train/nonfinite_grads']:.0f}", flush=True)


if __name__ == "__main__":
    main()
