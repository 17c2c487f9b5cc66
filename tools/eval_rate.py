"""Rate of the finetune driver's ``evaluate()`` -- ViT-B/16 with the config/ft.sh model flags at
224 px, valid batch 512, fed by validation loader workers from JPEG tar shards -- with the
validation transform in the workers (``--device-augment off``: PIL Resize + CenterCrop) against on
the GPU (``auto``: csrc/augment.hip window resize), per worker count, both arms in one process on
one box.

Each arm builds the loader the way ``main_finetune`` does (``use_device_valid``), runs one untimed
evaluation (worker start-up, shard cache, kernel warm-up) and then ``--passes`` timed ones; an
evaluation is one pass over the shards, so its time includes refilling the workers' prefetch queues.
The metrics of the two arms must be identical (the device path is bit-exact); that is asserted.

    python tools/eval_rate.py [--workers 10,4] [--shards 40] [--per-shard 256] [--passes 3] [--eval-report]

``--eval-report`` adds a third arm per worker count: the ``auto`` arm again with a fresh evaluation report
(ops/eval_report.py) filled, all-reduced and summarized in every evaluation, as ``main_finetune
--eval-report`` does (no files are written); its existing metrics must equal the other arms'.

Prints one JSON line per (workers, arm) and a final summary line."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from product_rate import FT, ensure_shards  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards-dir", default="/tmp/jmae_eval_shards")
    ap.add_argument("--shards", type=int, default=40)
    ap.add_argument("--per-shard", type=int, default=256)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--workers", default="10,4")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--eval-report", action="store_true")
    a = ap.parse_args()
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train.cli import finetune_parser
    from jumbo_mae_tpu_amd.ops.eval_report import EvalReport
    from jumbo_mae_tpu_amd.train.finetune import build_model, evaluate
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    ensure_shards(a.shards_dir, a.shards, a.per_shard, a.procs)
    spec = os.path.join(a.shards_dir, f"train-{{000000..{a.shards - 1:06d}}}.tar")
    device = torch.device("cuda:0")
    images = a.shards * a.per_shard
    model, rows = None, []
    for nw in [int(x) for x in a.workers.split(",")]:
        metrics = {}
        for mode, rep in [("off", False), ("auto", False)] + ([("auto", True)] if a.eval_report else []):
            args = finetune_parser().parse_args(FT + ["--valid-dataset-shards", spec, "--valid-batch-size", str(a.batch),
                                                      "--valid-loader-workers", str(nw), "--device-augment", mode])
            if model is None:
                model = build_model(args, device, C.compute_dtype(args, device))
                rngs = RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, device)
            dv = C.use_device_valid(args, device)
            assert dv == (mode == "auto"), (mode, dv)
            _, loader = create_dataloaders(args, device_valid=dv)

            def run():
                if not rep:
                    return evaluate(model, loader, rngs, device)
                report = EvalReport(model.cfg.labels, 15, args.criterion, device)
                m = evaluate(model, loader, rngs, device, report)
                report.all_reduce()
                extra.update(report.summary())
                return m

            extra = {}
            key = mode + ("+report" if rep else "")
            metrics[key] = run()  # untimed: workers start, kernels warm
            times = []
            for _ in range(a.passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = run()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                assert m == metrics[key], (m, metrics[key])
            del loader
            row = {"workers": nw, "device_augment": mode, "device_valid": dv, "eval_report": rep, "images": images,
                   "batch": a.batch, **({"report": extra} if rep else {}),
                   "passes_s": [round(t, 3) for t in times],
                   "images_per_sec": round(images / (sum(times) / len(times)), 1),
                   "best_images_per_sec": round(images / min(times), 1), "val": metrics[key],
                   "cpus": os.cpu_count()}
            rows.append(row)
            print(json.dumps(row), flush=True)
        assert all(m == metrics["off"] for m in metrics.values()), metrics  # bit-identical batches -> identical metrics
    print(json.dumps({"summary": {f"{r['workers']}w_{r['device_augment']}" + ("+report" if r["eval_report"] else ""):
                                  r["images_per_sec"] for r in rows}}), flush=True)


if __name__ == "__main__":
    main()
