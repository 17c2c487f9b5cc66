"""Representation statistics of a pretraining checkpoint's encoder features (the numbers that
``main_pretrain --feat-stats`` logs; no labels needed).

    python tools/feat_stats.py --ckpt out/run-last.msgpack <model flags of main_pretrain> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' [--feat-uniformity-t 2] [--time 5]

The model flags are the pretrain parser's and must describe the checkpoint; without --ckpt the model
keeps its --init-seed initialization.  Prints one JSON line with the val/feat_* keys.

``--time K``: the median event time over K runs of each kernel (``feat_gram`` over the rows in batches
of --valid-batch-size into one state, ``feat_uniformity`` of the rows against themselves) and of its
torch fp64 composition on the same device, with each one's peak memory above the inputs.
``--random-rows N`` replaces model and data by N random rows of width 3 * --dim, for timing a shape
without a dataset."""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _median_ms(fn, k: int) -> float:
    fn()
    times = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def _peak_mb(fn) -> float:
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main(argv=None):
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.ops import feat_stats as FS
    from jumbo_mae_tpu_amd.ops import knn as knn_ops
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train.cli import pretrain_parser
    from jumbo_mae_tpu_amd.train.pretrain import FeatMonitor, build_model

    ap = pretrain_parser()
    ap.add_argument("--ckpt", default=None, help="{name}-last/-best.msgpack of main_pretrain")
    ap.add_argument("--time", type=int, default=0, help="K > 0: median event time of each kernel over K runs")
    ap.add_argument("--random-rows", type=int, default=0, help="N > 0: N random rows instead of model and data")
    args = ap.parse_args(argv)
    if not args.feat_uniformity_t > 0:
        raise ValueError(f"--feat-uniformity-t must be positive (got {args.feat_uniformity_t})")
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    monitor = FeatMonitor(args.feat_uniformity_t)
    keep = []  # fp32 feature batches, kept only for --time
    if args.random_rows > 0:
        g = torch.Generator().manual_seed(0)
        for r0 in range(0, args.random_rows, args.valid_batch_size):
            n = min(args.valid_batch_size, args.random_rows - r0)
            f = torch.randn(n, 3 * args.dim, generator=g).to(device)
            monitor.update(f)
            if args.time > 0:
                keep.append(f)
    else:
        assert args.valid_dataset_shards, "--valid-dataset-shards is required"
        model = build_model(args, device, C.compute_dtype(args, device))
        if args.ckpt:
            model.load_flax_params(load_params(args.ckpt), strict=True)
        args.train_dataset_shards = None
        _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
        for batch in C.DevicePrefetcher(loader, device):
            images, labels = batch if isinstance(batch, (list, tuple)) else (batch, None)
            f = model.features(images)
            monitor.update(f, None, (labels != -1) if labels is not None else None)
            if args.time > 0:
                keep.append(f)
        del loader
    row = {"D": int(monitor.state["s"].shape[0]) if monitor.state is not None else 0, "t": args.feat_uniformity_t}
    row.update(monitor.finish())
    if args.time > 0:
        assert device.type == "cuda", "--time measures the GPU paths"
        D = row["D"]
        rows = torch.cat(monitor.rows)
        me = torch.arange(rows.shape[0], device=device, dtype=torch.int32)
        t = args.feat_uniformity_t

        def gram(fn, **kw):
            st = FS.new_state(D, device)
            for f in keep:
                fn(f, None, st, **kw)
            return st

        arms = {"gram_kernel": lambda: gram(FS.feat_gram),
                "gram_composition": lambda: gram(FS.feat_gram_torch, dtype=torch.float64),
                "uniformity_kernel": lambda: FS.feat_uniformity(rows, rows, me, None, t),
                "uniformity_composition": lambda: FS.feat_uniformity_torch(rows, rows, me, None, t,
                                                                          dtype=torch.float64)}
        for name, fn in arms.items():
            row[name + "_ms"] = round(_median_ms(fn, args.time), 3)
            row[name + "_peak_mb"] = round(_peak_mb(fn), 1)
        a, b = arms["gram_kernel"](), arms["gram_composition"]()
        row["gram_max_rel_diff"] = float(((a["G"] - b["G"]).abs().max() / b["G"].abs().max()))
        a, b = arms["uniformity_kernel"](), arms["uniformity_composition"]()
        row["uniformity_max_rel_diff"] = float(((a - b).abs() / b).max())
        row["rows"] = int(rows.shape[0])
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
