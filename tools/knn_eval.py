"""Weighted k-NN accuracy of a pretraining checkpoint's encoder features (the numbers that
``main_pretrain --knn-k`` logs, and the usual train-bank protocol).

    python tools/knn_eval.py --ckpt out/run-last.msgpack <model flags of main_pretrain> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' \\
        [--bank-dataset-shards 'train-{000000..000099}.tar' --bank-images 100000] --k 20 [--time 5]

With ``--bank-dataset-shards`` the bank is the features of (the first ``--bank-images`` of) those
shards under the validation transform and the validation images are the queries, no leave-one-out.
Without it the validation set is classified against itself, leave-one-out: the monitor's protocol.
The model flags are the pretrain parser's and must describe the checkpoint; without --ckpt the model
keeps its --init-seed initialization.  Prints one JSON line with ``acc1`` / ``acc5``.

``--time R``: the median event time over R runs of ``knn_topk`` at the run's own shape and of the
chunked torch composition on the same device (fp32 ``q @ bank.T`` in column blocks, ``topk``,
merge), with each one's peak memory above the inputs.  ``--random-rows N`` replaces model and data by
N random unit rows of width 3 * --dim (leave-one-out), for timing a shape without a dataset."""

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


def topk_chunked_torch(q, bank, k, self_idx=None, rows=8192, cols=8192):
    """The baseline a torch user writes: fp32 score blocks [rows, cols], ``topk`` of each, merged
    into a running [rows, k] list.  (No promise on the order of equal scores.)"""
    Nq, Nb = q.shape[0], bank.shape[0]
    idx = torch.empty(Nq, k, dtype=torch.int64, device=q.device)
    sim = torch.empty(Nq, k, dtype=torch.float32, device=q.device)
    for r0 in range(0, Nq, rows):
        qf = q[r0:r0 + rows].float()
        best_s = torch.full((qf.shape[0], k), float("-inf"), device=q.device)
        best_i = torch.full((qf.shape[0], k), -1, dtype=torch.int64, device=q.device)
        for c0 in range(0, Nb, cols):
            s = qf @ bank[c0:c0 + cols].float().t()
            if self_idx is not None:
                me = self_idx[r0:r0 + rows].long() - c0
                inside = (me >= 0) & (me < s.shape[1])
                s[inside.nonzero().squeeze(1), me[inside]] = float("-inf")
            v, i = s.topk(min(k, s.shape[1]), dim=1)
            cs, ci = torch.cat([best_s, v], 1), torch.cat([best_i, i + c0], 1)
            best_s, j = cs.topk(k, dim=1)
            best_i = ci.gather(1, j)
        idx[r0:r0 + rows], sim[r0:r0 + rows] = best_i, best_s
    return idx, sim


def _features(model, loader, device, limit, knn_ops, C):
    feats, labels, have = [], [], 0
    for batch in C.DevicePrefetcher(loader, device):
        assert isinstance(batch, (list, tuple)), "the shards carry no labels"
        images, y = batch
        feats.append(knn_ops.normalize_features(model.features(images)))
        labels.append(y.to(torch.int64))
        have += int((y != -1).sum())
        if limit and have >= limit:
            break
    return torch.cat(feats), torch.cat(labels)


def main(argv=None):
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.ops import knn as knn_ops
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train.cli import pretrain_parser
    from jumbo_mae_tpu_amd.train.pretrain import build_model

    ap = pretrain_parser()
    ap.add_argument("--ckpt", default=None, help="{name}-last/-best.msgpack of main_pretrain")
    ap.add_argument("--bank-dataset-shards", default=None, help="labelled shards whose features are the bank")
    ap.add_argument("--bank-images", type=int, default=0, help="use the first N bank images (0 = all)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--time", type=int, default=0, help="R > 0: median event time of knn_topk over R runs")
    ap.add_argument("--random-rows", type=int, default=0, help="N > 0: N random unit rows instead of model and data")
    args = ap.parse_args(argv)
    knn_ops.check_k(args.k)
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    bank = bank_labels = self_idx = None
    if args.random_rows > 0:
        g = torch.Generator().manual_seed(0)
        feats = torch.empty(args.random_rows, 3 * args.dim, dtype=torch.bfloat16, device=device)
        for r0 in range(0, args.random_rows, 8192):  # in blocks: no fp32 copy of the whole matrix
            n = min(8192, args.random_rows - r0)
            feats[r0:r0 + n] = knn_ops.normalize_features(torch.randn(n, 3 * args.dim, generator=g)).to(device)
        labels = torch.randint(0, 1000, (args.random_rows,), generator=g).to(device)
    else:
        assert args.valid_dataset_shards, "--valid-dataset-shards is required"
        model = build_model(args, device, C.compute_dtype(args, device))
        if args.ckpt:
            model.load_flax_params(load_params(args.ckpt), strict=True)
        args.train_dataset_shards = None
        _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
        feats, labels = _features(model, loader, device, 0, knn_ops, C)
        if args.bank_dataset_shards:  # the bank goes through the validation transform too
            args.valid_dataset_shards = args.bank_dataset_shards
            _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
            bank, bank_labels = _features(model, loader, device, args.bank_images, knn_ops, C)
            if args.bank_images:
                keep = (bank_labels != -1).nonzero().squeeze(1)[:args.bank_images]
                bank, bank_labels = bank[keep], bank_labels[keep]
        del loader
    hit1, hit5 = knn_ops.knn_classify(feats, labels, args.k, args.temperature, bank, bank_labels)
    n = max(int((labels != -1).sum()), 1)
    rows = int(((labels if bank is None else bank_labels) != -1).sum())  # padding rows never enter the bank
    row = {"queries": n, "bank": rows, "D": int(feats.shape[1]),
           "k": args.k, "temperature": args.temperature, "leave_one_out": bank is None,
           "acc1": round(float(hit1.sum()) / n, 6), "acc5": round(float(hit5.sum()) / n, 6)}
    if args.time > 0:
        assert device.type == "cuda", "--time measures the GPU paths"
        b = feats if bank is None else bank
        self_idx = torch.arange(feats.shape[0], device=device, dtype=torch.int32) if bank is None else None
        ours = lambda: knn_ops.knn_topk(feats, b, args.k, self_idx)  # noqa: E731
        comp = lambda: topk_chunked_torch(feats, b, args.k, self_idx)  # noqa: E731
        row["kernel_ms"] = round(_median_ms(ours, args.time), 3)
        row["kernel_peak_mb"] = round(_peak_mb(ours), 1)
        row["composition_ms"] = round(_median_ms(comp, args.time), 3)
        row["composition_peak_mb"] = round(_peak_mb(comp), 1)
        i1, s1 = ours()
        i2, s2 = comp()
        row["max_abs_sim_diff"] = float((s1 - s2).abs().max())
        row["idx_agreement"] = round(float((i1.long() == i2).float().mean()), 6)
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
