"""MAE reconstruction panels on the CPU: un-patchify, the torch composition (ops/mae.py
``reconstruct_torch``, the oracle of csrc/recon.hip), ``PretrainModel.reconstruct`` and the
``--recon-images`` flag of ``main_pretrain``."""

import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import recon_ref as R
from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.ops import mae as mae_ops
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
from jumbo_mae_tpu_amd.utils.mae import extract_patches_nchw, masking_ids


@pytest.mark.parametrize("p,H,W", [(14, 28, 28), (14, 28, 42), (16, 32, 32), (16, 48, 32)])
def test_unpatchify_inverts_extract_patches(p, H, W):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, H, W, generator=g)
    pt = extract_patches_nchw(x, p)
    assert pt.shape == (2, (H // p) * (W // p), 3 * p * p)
    assert torch.equal(mae_ops.unpatchify(pt, p, H, W), x)


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("p,H,W", [(14, 28, 28), (16, 32, 48)])
def test_round_trip_of_the_exact_target(p, H, W, norm_pix):
    """pred = the loss target itself: the fp64 composition gives the images back byte for byte and a
    zero error, the near-constant patch (sqrt(var + 1e-6) dominated by neither term) included."""
    g = torch.Generator().manual_seed(1)
    B = 2
    img = R.images_with_flat_patch(B, H, W, p, g)
    N = (H // p) * (W // p)
    mask = (torch.arange(N) % 2).float()
    out = mae_ops.reconstruct_torch(R.exact_target(img, p, norm_pix), img, mask, p, norm_pix, fp64=True)
    assert out["err"].dtype == torch.float64 and out["err"].shape == (B, N)
    assert torch.equal(out["recon"], img)
    assert out["err"].max().item() < 1e-20
    assert torch.equal(out["paste"], img)


def test_composition_clamps_and_zeroes_nan():
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (1, 3, 16, 16), generator=g, dtype=torch.uint8)
    pred = torch.zeros(1, 1, 768)
    pred[0, 0, 0:3] = 100.0
    pred[0, 0, 3:6] = -100.0
    pred[0, 0, 6:9] = float("nan")
    out = mae_ops.reconstruct_torch(pred, img, torch.ones(1), 16, False)
    assert out["recon"][0, :, 0, 0].tolist() == [255, 255, 255]
    assert out["recon"][0, :, 0, 1].tolist() == [0, 0, 0]
    assert out["recon"][0, :, 0, 2].tolist() == [0, 0, 0]
    assert torch.isfinite(out["err"]).all()
    # fill and paste follow the mask: everything masked here
    assert torch.equal(out["paste"], out["recon"]) and (out["masked"] == 127).all()


def _pixel_mask(mask, p, H, W):
    B = mask.shape[0]
    return mask.bool().reshape(B, 1, H // p, W // p).repeat_interleave(p, 2).repeat_interleave(p, 3).expand(B, 3, H, W)


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("mask_mode", ["shared", "per-sample"])
def test_model_reconstruct(mask_mode, norm_pix):
    model = R.tiny_model(mask_mode=mask_mode, norm_pix=norm_pix)
    g = torch.Generator().manual_seed(3)
    B, N = 3, 4
    img = torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8)
    noise = torch.rand((N,) if mask_mode == "shared" else (B, N), generator=g)
    state = torch.get_rng_state()
    out = model.reconstruct(img, noise=noise, fill=9)
    assert torch.equal(torch.get_rng_state(), state)  # a given noise: nothing drawn anywhere
    assert set(out) == {"recon", "paste", "masked", "mask", "err", "psnr_masked"}
    mask = masking_ids(noise, model.cfg.keep_len)[3]
    mask = mask if mask.dim() == 2 else mask.unsqueeze(0).expand(B, N)
    assert out["mask"].shape == (B, N) and torch.equal(out["mask"], mask)
    assert mask.sum(-1).tolist() == [3.0] * B
    mpix = _pixel_mask(mask, 16, 32, 32)
    assert torch.equal(out["paste"][~mpix], img[~mpix]) and torch.equal(out["paste"][mpix], out["recon"][mpix])
    assert torch.equal(out["masked"][~mpix], img[~mpix]) and (out["masked"][mpix] == 9).all()
    assert out["err"].shape == (B, N) and out["psnr_masked"].shape == (B,)
    want = -10.0 * torch.log10((out["err"] * mask).sum(-1) / 3.0)
    assert torch.allclose(out["psnr_masked"], want, rtol=1e-6, atol=0)
    # the same picture twice
    again = model.reconstruct(img, noise=noise, fill=9)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # forward == _predict + patch_mse + masked_mean_loss (droppath 0: det does not matter)
    with torch.no_grad():
        pred, m2, ids = model._predict(img, {}, False, False, noise)
        assert pred.shape == (B, N, 768) and len(ids) == 3
        per_patch = mae_ops.patch_mse(pred, img, 16, norm_pix)
        loss = mae_ops.masked_mean_loss(per_patch, m2)
        assert torch.equal(loss, model.forward(img, noise=noise)["loss"])


def test_reconstruct_draws_only_from_a_stream_it_is_given():
    model = R.tiny_model()
    img = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8)
    gen = torch.Generator().manual_seed(5)
    noise = torch.rand(4, generator=torch.Generator().manual_seed(5))
    a = model.reconstruct(img, rngs={"noise": gen})
    b = model.reconstruct(img, noise=noise)
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["recon"], b["recon"])


def test_recon_flag_is_pretrain_only_and_off_by_default():
    assert pretrain_parser().parse_args([]).recon_images == 0
    assert pretrain_parser().parse_args(["--recon-images", "4"]).recon_images == 4
    with pytest.raises(SystemExit):
        finetune_parser().parse_args(["--recon-images", "4"])


# ------------------------------------------------------------------ driver
S = 32
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", str(S),
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--auto-augment", "none", "--augment-repeats", "1",
          "--labels", "0", "--dec-layers", "1", "--dec-dim", "64", "--dec-heads", "2", "--learning-rate", "5e-3",
          "--training-steps", "2", "--warmup-steps", "1", "--log-interval", "1", "--eval-interval", "2",
          "--droppath", "0.1", "--dec-droppath", "0.1", "--name", "p"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=1, per_shard=8, classes=4, seed=1, prefix="valid")
    outs = {}
    for name, extra in (("with", ["--recon-images", "4"]), ("without", [])):
        out = str(tmp_path_factory.mktemp(name))
        args = pretrain_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                      "--output-dir", out, *extra])
        outs[name] = (out, PT.main(args))
    return outs


def _rows(out):
    return [json.loads(line) for line in open(os.path.join(out, "p-metrics.jsonl"))]


def test_driver_writes_png_and_psnr(runs):
    out, res = runs["with"]
    for step in (0, 2):  # the sanity evaluation and the evaluation at the last step
        with Image.open(os.path.join(out, f"p-recon-{step:07d}.png")) as im:
            assert im.size == (4 * S, 4 * S) and im.mode == "RGB"
    rows = [r for r in _rows(out) if "val/loss" in r]
    assert len(rows) == 2 and all(np.isfinite(r["val/psnr_masked"]) for r in rows), rows
    assert np.isfinite(res["val/psnr_masked"])
    # the leftmost panel is the validation image itself; "masked" differs from it exactly on the
    # fill patches, which are the same at both evaluations (private generator seeded by --noise-seed)
    fills = []
    for step in (0, 2):
        with Image.open(os.path.join(out, f"p-recon-{step:07d}.png")) as im:
            a = np.asarray(im)
        fills.append((a[:, S:2 * S] == 127).all(-1))
        assert np.array_equal(a[:, :S][~fills[-1]], a[:, S:2 * S][~fills[-1]])
    assert fills[0].any() and np.array_equal(fills[0], fills[1])


def test_driver_without_the_flag_is_untouched(runs):
    out, res = runs["without"]
    assert not [f for f in os.listdir(out) if f.endswith(".png")]
    assert not any("val/psnr_masked" in r for r in _rows(out)) and "val/psnr_masked" not in res
    a = flatten_tree(load_params(os.path.join(out, "p-last.msgpack")))
    b = flatten_tree(load_params(os.path.join(runs["with"][0], "p-last.msgpack")))
    assert set(a) == set(b)
    for k in a:  # the flag takes nothing from the training streams: bit-identical final weights
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "/".join(k)
    la = [r["val/loss"] for r in _rows(out) if "val/loss" in r]
    lb = [r["val/loss"] for r in _rows(runs["with"][0]) if "val/loss" in r]
    assert la == lb
