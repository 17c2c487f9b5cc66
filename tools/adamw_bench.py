"""AdamW multi-tensor kernel (csrc/optim.hip) alone on ViT-L-sized flat buffers (16 B per lane;
profiles/r3_adamw_streaming.txt: the pass runs at ~5.0 TB/s).

    python tools/adamw_bench.py [--n 400000000] [--rounds 5] [--ema]

--ema also times the weight-EMA pass (``opt_ema``: 12 B per parameter) and the EMA swap (``ema_swap``
with the bf16 shadow: 18 B per parameter) on the same chunk table, in the same process."""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jumbo_mae_tpu_amd.ops import _ext  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=65536, help="elements per chunk-table row")
    ap.add_argument("--ema", action="store_true", help="also time opt_ema and ema_swap on the same buffers")
    a = ap.parse_args()
    ext = _ext.load()
    C = a.chunk
    n = a.n // C * C
    p, g = torch.randn(n, device="cuda") * 0.02, torch.randn(n, device="cuda") * 1e-3
    mu, nu = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    starts = torch.arange(0, n, C, dtype=torch.int32)
    chunks = torch.stack([starts, torch.full_like(starts, C), torch.zeros_like(starts)], 1).contiguous().cuda()
    meta = torch.tensor([1.0, 1.0, 0.0, 1.0], device="cuda")
    hyper = torch.tensor([1e-4, 0.1, 0.05, 1.0, 0.9, 0.95, 1e-8, 0.05], device="cuda")
    gn = torch.tensor([-1.0], device="cuda")
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
        tb = min(ts)
        print(f"{name} n={n} chunk={C}: {tb:8.1f} us (rounds {', '.join(f'{x:.0f}' for x in ts)})  "
              f"{bytes_per_param * n / tb / 1e6:5.2f} TB/s at {bytes_per_param:.0f} B/param", flush=True)
        return tb

    t_adamw = timed("adamw", lambda: ext.opt_adamw(p, g, mu, nu, shadow, chunks, meta, hyper, gn), 30.0)
    if a.ema:
        ema = p.clone()
        ema_hyper = torch.tensor([1e-4], device="cuda")
        meta2 = meta.reshape(1, 4)
        t_ema = timed("ema", lambda: ext.opt_ema(p, ema, chunks, meta2, ema_hyper), 12.0)
        t_swap = timed("ema_swap", lambda: ext.ema_swap(p, ema, shadow, chunks), 18.0)
        print(f"ema / adamw = {t_ema / t_adamw:.3f}   ema_swap / adamw = {t_swap / t_adamw:.3f}", flush=True)


if __name__ == "__main__":
    main()
