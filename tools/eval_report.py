"""Evaluation report of a finetuned checkpoint: per-class accuracy, calibration (ECE / MCE) and confusion
(what ``main_finetune --eval-report`` logs and writes at every evaluation; ops/eval_report.py).

    python tools/eval_report.py --ckpt out/run-best.msgpack <model flags of main_finetune> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' --out report.json [--dump-rows rows.npz]

runs the validation set once, prints the metrics and the ten worst classes, and writes the report JSON
(``--dump-rows``: also label, pred, rank and conf of every row).  The model flags are the finetune
parser's and must describe the checkpoint; without --ckpt the model keeps its --init-seed initialization.

    python tools/eval_report.py --random-rows B L --time K [--criterion ce|bce]

times the two kernels of csrc/eval_report.hip (per-row outputs, accumulation) over K runs against the torch
composition on the same device, on ``4 * randn`` bf16 logits; prints one JSON line."""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median_us(fn, k: int) -> float:
    for _ in range(3):
        fn()
    times = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return sorted(times)[len(times) // 2]


def time_rows(B: int, L: int, k: int, mode: str, n_bins: int = 15) -> dict:
    from jumbo_mae_tpu_amd.ops import eval_report as E
    from jumbo_mae_tpu_amd.ops import prims as P

    assert torch.cuda.is_available(), "--time measures the GPU paths"
    g = torch.Generator().manual_seed(0)
    z = (4.0 * torch.randn(B, L, generator=g)).bfloat16().cuda()
    y = torch.randint(0, L, (B,), generator=g).cuda()
    row = {"shape": [B, L], "dtype": "bf16", "mode": mode, "bins": n_bins, "runs": k}
    states = {}
    for on in (True, False):
        P._EVAL_REPORT_OURS = on
        name = "kernel" if on else "composition"
        rep = E.EvalReport(L, n_bins, mode, "cuda")
        out = E.eval_rows(z, y, mode)
        row[name + "_rows_us"] = round(_median_us(lambda: E.eval_rows(z, y, mode), k), 2)
        row[name + "_accumulate_us"] = round(_median_us(
            lambda: E.eval_accumulate(y, *out, L, n_bins, rep.state), k), 2)
        row[name + "_update_us"] = round(_median_us(lambda: rep.update(z, y), k), 2)
        fresh = E.EvalReport(L, n_bins, mode, "cuda")
        fresh.update(z, y)
        states[on] = fresh
    P._EVAL_REPORT_OURS = True
    a, b = states[True].v, states[False].v
    row["integer_state_equal"] = all(bool(torch.equal(a[n], b[n])) for n in a if n != "bins")
    return row


def main(argv=None):
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.ops.eval_report import EvalReport
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train.cli import finetune_parser
    from jumbo_mae_tpu_amd.train.finetune import build_model
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    ap = finetune_parser()
    ap.add_argument("--ckpt", default=None, help="{name}-best / -last / -ema-best .msgpack of main_finetune")
    ap.add_argument("--out", default=None, help="write the report JSON here")
    ap.add_argument("--dump-rows", default=None, help="write label / pred / rank / conf of every row (.npz)")
    ap.add_argument("--random-rows", type=int, nargs=2, metavar=("B", "L"), default=None,
                    help="B random rows of L classes instead of model and data (with --time)")
    ap.add_argument("--time", type=int, default=0, help="K > 0: median event time over K runs")
    args = ap.parse_args(argv)
    if args.random_rows:
        row = time_rows(args.random_rows[0], args.random_rows[1], max(args.time, 1), args.criterion,
                        args.eval_report_bins)
        print(json.dumps(row), flush=True)
        return row
    assert args.valid_dataset_shards, "--valid-dataset-shards is required"
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = build_model(args, device, C.compute_dtype(args, device))
    if args.ckpt:
        tree = load_params(args.ckpt)
        if "model" not in tree and isinstance(tree.get("params"), dict):
            tree = tree["params"]
        model.store.load_flax_tree(tree, strict=True)
        model.store.sync_shadow()
    args.train_dataset_shards = None
    _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
    report = EvalReport(model.cfg.labels, args.eval_report_bins, args.criterion, device)
    rows = {"label": [], "pred": [], "rank": [], "conf": []}
    if args.dump_rows:
        from jumbo_mae_tpu_amd.ops import eval_report as E
        inner = report.update

        def update(logits, labels):  # the same per-row outputs, kept
            pred, rank, conf = E.eval_rows(logits, labels, report.mode)
            for k, v in zip(rows, (labels, pred, rank, conf)):
                rows[k].append(v.cpu().numpy())
            inner(logits, labels)

        report.update = update
    rngs = RngStreams({"mixup": 0, "dropout": 0, "noise": 0}, 0, device).fork()
    sums = None
    for images, labels in C.DevicePrefetcher(loader, device):
        m = model.evaluate(images, labels, rngs.as_dict(), report=report)
        sums = m if sums is None else {k: sums[k] + m[k] for k in m}
    n = max(float(sums["num_samples"]), 1.0)
    j = report.to_json()
    j["metrics"].update({"val/" + k: float(sums[k]) / n for k in ("loss", "acc1", "acc5")})
    for k, v in sorted(j["metrics"].items()):
        print(f"{k:28s} {v:.6g}")
    seen = [c for c in j["per_class"] if c["count"]]
    print("worst classes (id, acc1, count, most frequent wrong prediction):")
    for c in sorted(seen, key=lambda c: (c["acc1"], c["id"]))[:10]:
        t = c["top_confusion"]
        print(f"  {c['id']:6d}  {c['acc1']:.4f}  {c['count']:6d}  " + (f"{t['pred']} x{t['count']}" if t else "-"))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(j, f, indent=1)
    if args.dump_rows:
        np.savez(args.dump_rows, **{k: np.concatenate(v) for k, v in rows.items()})
    return j


if __name__ == "__main__":
    main()
