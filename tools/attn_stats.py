"""Per-layer, per-head attention statistics of a checkpoint (what ``--attn-stats`` logs, unreduced).

    python tools/attn_stats.py --ckpt out/run-last.msgpack <model flags of main_pretrain> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' --n 64 [--finetune]

Runs the first ``--n`` validation images through the model once (``PretrainModel.attention_stats``
under the mask of a private generator seeded with --noise-seed, or with ``--finetune`` the
``FinetuneModel`` of the finetune parser's flags) and prints, per layer and head, the mean row
entropy of the attention softmax in nats (uniform attention over S keys = log S), the mean largest
probability, the mean mass on the CLS tokens, the largest logit and the rows without a finite entropy,
then one JSON line.  The model flags must describe the checkpoint; without --ckpt the model keeps its
--init-seed initialization.

``--random-qkv B S H hd --time K``: no model and no data: the median event time over K runs of the
kernel on a random bf16 ``qkv [B, S, 3 H hd]`` and of the torch composition on the same device, with
each one's peak memory above the inputs.
"""

from __future__ import annotations

import json
import math
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


def time_random(shape, k: int, device, n_cls: int = 3) -> dict:
    from jumbo_mae_tpu_amd.ops import attn_stats as AS

    assert device.type == "cuda", "--time measures the GPU paths"
    B, S, H, hd = shape
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * hd, generator=g).to(torch.bfloat16).to(device)
    n_cls = min(n_cls, S)
    ours = lambda: AS.attn_stats(qkv, H, n_cls)  # noqa: E731
    comp = lambda: AS.attn_stats_torch(qkv, H, n_cls, torch.float32)  # noqa: E731
    row = {"B": B, "S": S, "H": H, "hd": hd, "n_cls": n_cls,
           "kernel_ms": round(_median_ms(ours, k), 4), "kernel_peak_mb": round(_peak_mb(ours), 2),
           "composition_ms": round(_median_ms(comp, k), 4), "composition_peak_mb": round(_peak_mb(comp), 2)}
    a, b = ours(), comp()
    good = a[:, 5] - a[:, 4]
    row["max_abs_mean_entropy_diff"] = float((a[:, 0] / good - b[:, 0] / (b[:, 5] - b[:, 4])).abs().max())
    return row


def table_lines(tables: dict) -> list:
    lines = [f"{'layer':<24}{'head':>5}{'entropy':>10}{'max_prob':>10}{'cls_mass':>10}{'max_logit':>11}{'bad':>6}"]
    for name, tab in tables.items():
        t = tab.double().cpu()
        for h in range(t.shape[0]):
            good = float(t[h, 5] - t[h, 4])
            mean = [float(t[h, j]) / good if good else math.nan for j in range(3)]
            lines.append(f"{name:<24}{h:>5}{mean[0]:>10.4f}{mean[1]:>10.4f}{mean[2]:>10.4f}{float(t[h, 3]):>11.3f}"
                         f"{int(t[h, 4]):>6}")
    return lines


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.ops import attn_stats as AS
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train import cli

    finetune = "--finetune" in argv
    ap = cli.finetune_parser() if finetune else cli.pretrain_parser()
    ap.add_argument("--finetune", action="store_true", help="a FinetuneModel checkpoint (the finetune parser's flags)")
    ap.add_argument("--ckpt", default=None, help="{name}-last/-best.msgpack of the driver")
    ap.add_argument("--n", type=int, default=64, help="validation images")
    ap.add_argument("--random-qkv", type=int, nargs=4, default=None, metavar=("B", "S", "H", "HD"))
    ap.add_argument("--time", type=int, default=0, help="K > 0 with --random-qkv: median event time over K runs")
    args = ap.parse_args(argv)
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if args.random_qkv is not None:
        row = time_random(tuple(args.random_qkv), max(args.time, 1), device)
        print(json.dumps(row), flush=True)
        return row
    assert args.valid_dataset_shards, "--valid-dataset-shards is required"
    if finetune:
        from jumbo_mae_tpu_amd.train.finetune import build_model
        model = build_model(args, device, C.compute_dtype(args, device), 0)
    else:
        from jumbo_mae_tpu_amd.train.pretrain import build_model
        model = build_model(args, device, C.compute_dtype(args, device))
    if args.ckpt:
        model.store.load_flax_tree(load_params(args.ckpt), strict=True)
    args.train_dataset_shards = None
    args.attn_stats = args.n
    _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
    images = C.first_images(loader, args.n, device)
    del loader
    if finetune:
        tables = model.attention_stats(images)
    else:
        B, n = images.shape[0], model.cfg.seq_patches
        g = torch.Generator().manual_seed(args.noise_seed)
        noise = torch.rand((n,) if model.mask_mode == "shared" else (B, n), generator=g).to(device)
        tables = model.attention_stats(images, noise=noise)
    for line in table_lines(tables):
        print(line)
    vals, bad = AS.summarize(tables)
    for line in bad:
        print(line)
    row = {"images": int(images.shape[0]), "layers": len(tables),
           "attn_entropy_min": vals["val/attn_entropy_min"], "attn_max_logit": vals["val/attn_max_logit"]}
    print(json.dumps(row), flush=True)
    return {"tables": tables, "values": vals, **row}


if __name__ == "__main__":
    main()
