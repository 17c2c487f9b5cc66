"""Shared inputs of the reconstruction tests (tests/test_recon.py, tests/test_recon_gpu.py).

The oracle of csrc/recon.hip is ops/mae.py ``reconstruct_torch(..., fp64=True)`` on the prediction
as stored; nothing here computes reference values of its own."""

import torch

from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import mae as mae_ops
from jumbo_mae_tpu_amd.utils.mae import extract_patches_nchw

# bytes whose normalized values (u / 255 - mean_c) / std_c are nearly equal (0.005, -0.005, 0.008): a
# patch painted with them has the smallest variance the three channel constants admit (3e-5, next to
# the 1e-6 under the square root); a patch of equal values in every channel does not exist in uint8
FLAT_RGB = (124, 116, 104)


def ulp32(x):
    """Spacing of fp32 at |x| (x fp64), as fp64."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def images_with_flat_patch(B, H, W, p, gen):
    """Random uint8 images; patch (0, 0) of image 0 is painted FLAT_RGB."""
    img = torch.randint(0, 256, (B, 3, H, W), generator=gen, dtype=torch.uint8)
    for c in range(3):
        img[0, c, :p, :p] = FLAT_RGB[c]
    return img


def exact_target(img, p, norm_pix):
    """The loss target in fp64 [B, N, 3p^2]: normalized patches (fp32 constants), or their norm_pix."""
    m, s = mae_ops._mean_std(img.device)
    t = extract_patches_nchw((img.double() / 255.0 - m.double()) / s.double(), p)
    return mae_ops.norm_pix(t) if norm_pix else t


def tiny_model(device="cpu", dtype=torch.float32, mask_mode="shared", norm_pix=False, master=None):
    """dim 64, 2 heads, 2 + 1 layers, 32 px, p = 16 (N = 4, 1 kept), no droppath."""
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=0, image_size=32, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75, droppath=0.0)
    dc = DecoderConfig(dec_layers=1, dec_dim=64, dec_heads=2, image_size=32, patch_size=16, dec_droppath=0.0)
    m = PretrainModel(vc, dc, norm_pix_loss=norm_pix, mask_mode=mask_mode).to(torch.device(device), dtype, seed=0)
    if master is not None:
        with torch.no_grad():
            m.store.master.copy_(master.to(m.store.master.device))
        m.store.sync_shadow()
    return m
