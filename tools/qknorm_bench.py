"""Kernel times of QK-norm (csrc/qknorm.hip) at one shape: forward + backward with and without rope,
against rope_apply forward + inverse alone and against the torch composition on the GPU.  Medians
over ``--iters`` launches timed by events, one process per shape (as tools/attn_bench.py):

    python tools/qknorm_bench.py --B 2048 --S 52 --H 16 --hd 64
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--S", type=int, default=52)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--hd", type=int, default=64)
    ap.add_argument("--n-cls", type=int, default=3)
    ap.add_argument("--grid", type=int, default=14)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    a = ap.parse_args()
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.ops.qknorm import qknorm_bwd_torch, qknorm_torch
    from jumbo_mae_tpu_amd.ops.rope import Rope, rope_table
    ext = _ext.load(True)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    B, S, H, hd = a.B, a.S, a.H, a.hd
    x = (torch.randn(B, S, 3 * H * hd, device="cuda") * 2).to(dt)
    dy = torch.randn_like(x)
    gq, gk = 1 + 0.5 * torch.randn(hd, device="cuda"), 1 + 0.5 * torch.randn(hd, device="cuda")
    table = rope_table(a.grid, hd, 100.0, "cuda")
    Sp = S - a.n_cls
    pos = torch.stack([torch.randperm(a.grid * a.grid)[:Sp] for _ in range(B)]).to(torch.int32).cuda()
    rope = Rope(a.n_cls, a.grid, table, pos)
    ra = (a.n_cls, a.grid, table, pos)
    saved = ext.qknorm_fwd(x.clone(), H, gq, gk)
    esz = x.element_size()
    n_qk = B * S * 2 * H * hd
    res = {}
    for name, args in (("qknorm", ()), ("qknorm+rope", ra)):
        res[name + " fwd"] = _median_ms(lambda: ext.qknorm_fwd(x, H, gq, gk, *args), a.iters)
        res[name + " bwd"] = _median_ms(lambda: ext.qknorm_bwd(dy, saved, H, gq, gk, *args), a.iters)
    res["rope fwd"] = _median_ms(lambda: ext.rope_apply(x, H, *ra, False), a.iters)
    res["rope inverse"] = _median_ms(lambda: ext.rope_apply(x, H, *ra, True), a.iters)
    x = (torch.randn(B, S, 3 * H * hd, device="cuda") * 2).to(dt)
    it = max(3, a.iters // 6)
    with torch.no_grad():
        res["composition fwd (+rope)"] = _median_ms(lambda: qknorm_torch(x, H, gq, gk, rope), it, 2)
        res["composition bwd (+rope)"] = _median_ms(lambda: qknorm_bwd_torch(dy, saved, H, gq, gk, rope), it, 2)
    print(f"shape B {B} S {S} H {H} hd {hd} {a.dtype}, n_cls {a.n_cls}, grid {a.grid}; medians of {a.iters} launches")
    for k, v in res.items():
        print(f"  {k:28s} {v:8.4f} ms")
    # bytes moved: fwd reads q|k, writes q|k and saved; bwd reads dq|dk and saved, writes dq|dk
    fb = 3 * n_qk * esz
    for k in ("qknorm fwd", "qknorm bwd", "qknorm+rope fwd", "qknorm+rope bwd"):
        print(f"  {k:28s} {fb / 2 ** 20:8.1f} MiB moved, {fb / res[k] / 1e9:8.3f} TB/s")


if __name__ == "__main__":
    main()
