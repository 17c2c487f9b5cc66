"""MAE reconstructions of a pretraining checkpoint: the PNG that ``main_pretrain --recon-images``
writes (one row per image: original | masked | reconstruction | pasted) and the masked-patch PSNR
of each image, from the first ``--n`` images of ``--valid-dataset-shards``.

    python tools/reconstruct.py --ckpt out/run-last.msgpack <model flags of main_pretrain> \\
        --valid-dataset-shards 'valid-{000000..000003}.tar' --n 8 --seed 0 --out recon.png [--time 50]

The model flags (--layers, --dim, --heads, --patch-size, --image-size, --dec-*, --norm-pix-loss,
--mask-mode, ...) are the pretrain parser's and must describe the checkpoint; without --ckpt the
model keeps its --init-seed initialization.  Prints one JSON line: ``psnr_masked`` per image, its
mean and, with ``--time K``, the median event time over K calls of ``reconstruct_panels`` on the
HIP kernel and of the torch composition on the GPU for the batch it loaded."""

from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _median_ms(fn, k: int) -> float:
    for _ in range(3):
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


def main(argv=None):
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.ops import mae as mae_ops
    from jumbo_mae_tpu_amd.train import common as C
    from jumbo_mae_tpu_amd.train.cli import pretrain_parser
    from jumbo_mae_tpu_amd.train.pretrain import build_model, first_images, recon_panel

    ap = pretrain_parser()
    ap.add_argument("--ckpt", default=None, help="{name}-last/-best.msgpack of main_pretrain")
    ap.add_argument("--n", type=int, default=8, help="images (the first of the validation shards)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the mask noise")
    ap.add_argument("--out", default="recon.png")
    ap.add_argument("--time", type=int, default=0, help="K > 0: median event time of reconstruct_panels over K calls")
    args = ap.parse_args(argv)
    assert args.valid_dataset_shards, "--valid-dataset-shards is required"
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = build_model(args, device, C.compute_dtype(args, device))
    if args.ckpt:
        model.load_flax_params(load_params(args.ckpt), strict=True)
    args.train_dataset_shards = None
    _, loader = create_dataloaders(args, device_valid=C.use_device_valid(args, device))
    images = first_images(loader, args.n, device)
    del loader
    B, N = images.shape[0], model.cfg.seq_patches
    g = torch.Generator().manual_seed(args.seed)
    noise = torch.rand((N,) if model.mask_mode == "shared" else (B, N), generator=g).to(device)
    out = model.reconstruct(images, noise=noise)
    recon_panel(images, out).save(args.out)
    psnr = [float(v) for v in out["psnr_masked"].tolist()]
    row = {"images": B, "image_size": images.shape[-1], "patch_size": model.cfg.patch_size,
           "norm_pix_loss": bool(model.norm_pix_loss), "out": args.out, "psnr_masked": [round(v, 4) for v in psnr],
           "psnr_masked_mean": round(sum(psnr) / len(psnr), 4)}
    if args.time > 0:
        assert device.type == "cuda", "--time measures the GPU paths"
        with torch.no_grad():
            pred, mask, _ = model._predict(images, {}, True, True, noise)
        p, npx = model.cfg.patch_size, model.norm_pix_loss
        row["pred_dtype"] = str(pred.dtype)
        row["kernel_ms"] = round(_median_ms(lambda: mae_ops.reconstruct_panels(pred, images, mask, p, npx), args.time), 4)
        row["composition_ms"] = round(_median_ms(lambda: mae_ops.reconstruct_torch(pred, images, mask, p, npx),
                                                 args.time), 4)
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
