"""CLS attention maps of a checkpoint (what ``--attn-maps`` draws).

    python tools/attn_maps.py --ckpt out/run-last.msgpack <model flags of main_pretrain> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' --n 8 --out maps.png \\
        [--attn-maps-mode last] [--finetune]

Runs the first ``--n`` validation images, unmasked, through the encoder once (``attention_maps`` of the
``PretrainModel``, or with ``--finetune`` of the ``FinetuneModel`` of the finetune parser's flags), writes
the panel of ``train/common.py attn_map_panel`` -- one row per image: the original, then one heat-map
overlay per CLS token -- to ``--out`` and prints one JSON line with the maps' mean entropy and CLS mass.
The picture is chosen with the drivers' own ``--attn-maps-mode rollout|last`` (``--mode`` belongs to the
parsers: pretrain, finetune, linear).
The model flags must describe the checkpoint; without --ckpt the model keeps its --init-seed
initialization.

``--random-qkv B S H hd L --time K`` (K >= 1): no model and no data: the median event time over K runs of
``rollout`` over L random bf16 layers ``qkv [B, S, 3 H hd]`` on the kernels and, on the same device, with
``prims._ATTN_MAPS_OURS = False`` (the torch composition), with each one's peak memory above the inputs.
"""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _median_ms(fn, k: int, warmup: int = 3) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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


def time_random(shape, k: int, device, n_cls: int = 3, alpha: float = 0.5) -> dict:
    from jumbo_mae_tpu_amd.ops import attn_maps as AM
    from jumbo_mae_tpu_amd.ops import prims as P

    assert device.type == "cuda", "--time measures the GPU paths"
    B, S, H, hd, L = shape
    g = torch.Generator().manual_seed(0)
    qkvs = [torch.randn(B, S, 3 * H * hd, generator=g).to(torch.bfloat16).to(device) for _ in range(L)]
    n_cls = min(n_cls, S)

    def run(ours: bool):
        keep, P._ATTN_MAPS_OURS = P._ATTN_MAPS_OURS, ours
        try:
            return AM.rollout(qkvs, H, n_cls, alpha)
        finally:
            P._ATTN_MAPS_OURS = keep

    ours, comp = (lambda: run(True)), (lambda: run(False))
    row = {"B": B, "S": S, "H": H, "hd": hd, "L": L, "n_cls": n_cls,
           "kernel_ms": round(_median_ms(ours, k), 4), "kernel_peak_mb": round(_peak_mb(ours), 2),
           "composition_ms": round(_median_ms(comp, k), 4), "composition_peak_mb": round(_peak_mb(comp), 2)}
    row["max_abs_diff"] = float((ours() - comp()).abs().max())
    return row


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train import cli

    finetune = "--finetune" in argv
    ap = cli.finetune_parser() if finetune else cli.pretrain_parser()
    ap.add_argument("--finetune", action="store_true", help="a FinetuneModel checkpoint (the finetune parser's flags)")
    ap.add_argument("--ckpt", default=None, help="{name}-last/-best.msgpack of the driver")
    ap.add_argument("--n", type=int, default=8, help="validation images")
    ap.add_argument("--out", default="maps.png", help="the PNG panel")
    ap.add_argument("--random-qkv", type=int, nargs=5, default=None, metavar=("B", "S", "H", "HD", "L"))
    ap.add_argument("--time", type=int, default=0, help="K >= 1, with --random-qkv: median event time over K runs")
    args = ap.parse_args(argv)
    if (args.random_qkv is not None) != (args.time >= 1):
        ap.error("--random-qkv B S H HD L and --time K (K >= 1) go together")
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    if args.random_qkv is not None:
        row = time_random(tuple(args.random_qkv), args.time, device)
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
    _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
    images = C.first_images(loader, args.n, device)
    del loader
    out = model.attention_maps(images, mode=args.attn_maps_mode)
    panel = C.attn_map_panel(images, out["maps"])
    panel.save(args.out)
    vals = C.attn_map_values(out)
    row = {"images": int(images.shape[0]), "cls_tokens": int(out["maps"].shape[1]), "grid": list(out["maps"].shape[2:]),
           "mode": args.attn_maps_mode, "out": args.out, "size": list(panel.size),
           "attn_map_entropy": vals["val/attn_map_entropy"], "attn_map_cls_mass": vals["val/attn_map_cls_mass"]}
    print(json.dumps(row), flush=True)
    return {"maps": out["maps"], "cls_mass": out["cls_mass"], "values": vals, **row}


if __name__ == "__main__":
    main()
