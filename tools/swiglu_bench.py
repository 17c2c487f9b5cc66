"""Kernel times and achieved bytes/s of the SwiGLU gate (csrc/swiglu.hip) beside the GELU kernels
(csrc/elementwise.hip gelu_fwd / gelu_bwd) at the matching GELU width, in one process.  Medians over ``--iters``
launches timed by events; the operands of a launch rotate through ``--sets`` buffers so that together they
exceed the 256 MiB Infinity Cache:

    python tools/swiglu_bench.py --M 25088 --dims 768 1024
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fns, iters, warmup=4):
    n = len(fns)
    for i in range(warmup):
        fns[i % n]()
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fns[i % n]()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=25088)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sets", type=int, default=4)
    a = ap.parse_args()
    from jumbo_mae_tpu_amd.config import ffn_hidden
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    M = a.M
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    print(f"M {M}, bf16; medians of {a.iters} launches over {a.sets} operand sets")
    for dim in a.dims:
        Hs, Hg = ffn_hidden(dim, "swiglu"), 4 * dim
        pre = [(2 * torch.randn(M, 2 * Hs, device="cuda")).bfloat16() for _ in range(a.sets)]
        da = [torch.randn(M, Hs, device="cuda").bfloat16() for _ in range(a.sets)]
        h = [(2 * torch.randn(M, Hg, device="cuda")).bfloat16() for _ in range(a.sets)]
        dg = [torch.randn(M, Hg, device="cuda").bfloat16() for _ in range(a.sets)]
        b13 = torch.zeros(2 * Hs, device="cuda")
        b1 = torch.zeros(Hg, device="cuda")
        rows = (
            (f"swiglu_fwd  Hs {Hs}", [lambda p=p: ext.swiglu_fwd(p) for p in pre], 6 * M * Hs),
            (f"swiglu_fwd  Hs {Hs} dropout 0.1", [lambda p=p: ext.swiglu_fwd(p, seed, 0.1) for p in pre], 6 * M * Hs),
            (f"swiglu_bwd  Hs {Hs} + bias grad", [lambda p=p, d=d: ext.swiglu_bwd(p, d, b13) for p, d in zip(pre, da)],
             10 * M * Hs),
            (f"swiglu_bwd  Hs {Hs}", [lambda p=p, d=d: ext.swiglu_bwd(p, d) for p, d in zip(pre, da)], 10 * M * Hs),
            (f"gelu_fwd    N {Hg}", [lambda x=x: ext.gelu_fwd(x) for x in h], 4 * M * Hg),
            (f"gelu_bwd    N {Hg} + bias grad", [lambda x=x, d=d: ext.gelu_bwd(x, d, b1, False) for x, d in zip(h, dg)],
             6 * M * Hg),
        )
        for name, fns, nbytes in rows:
            ms = _median_ms(fns, a.iters)
            print(f"  dim {dim:5d}  {name:36s} {ms:8.4f} ms  {nbytes / 2 ** 20:8.1f} MiB  {nbytes / ms / 1e9:6.3f} TB/s")
        del pre, da, h, dg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
