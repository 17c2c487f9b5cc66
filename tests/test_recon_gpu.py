"""csrc/recon.hip (MAE reconstruction panels) against ops/mae.py ``reconstruct_torch`` in fp64 on
the prediction as stored, and ``PretrainModel.reconstruct`` on the GPU against the CPU.

Bounds.  ``masked``, ``paste`` and the saturated / NaN bytes are exact.  A ``recon`` byte may
differ from the oracle's by 1 only where the fp64 pixel value lies within ``delta`` of a rounding
tie k + 0.5; ``delta`` = 2 x the largest |x_fp32 - x_fp64| of the fp32 torch composition over the
case's elements (not less than one fp32 ulp of 255), and at most 1 % of a case may be excused
(asserted on the oracle alone).  ``err`` stays per patch within max(2 x the fp32 composition's
error on that patch, 1 fp32 ulp) of the fp64 value and is bit-identical across runs.  Both margins
come from the composition, never from the kernel."""

import pytest
import torch

import recon_ref as R
from jumbo_mae_tpu_amd.ops import _ext
from jumbo_mae_tpu_amd.ops import mae as mae_ops

pytestmark = pytest.mark.gpu

ULP_255 = 2.0 ** -16  # fp32 spacing in [128, 256)

# the 4-byte path with N = 4; the byte path (p = 14); H != W
SHAPES = [(3, 32, 32, 16), (3, 28, 28, 14), (2, 32, 48, 16)]


def _case(B, H, W, p, dtype, norm_pix, shared, nan, seed):
    """(pred as stored [B*N, 3p^2], images, mask) on the CPU.  pred = the exact target + unit noise:
    about a third of it leaves [0, 255] on either side; image 0's first patch is near-constant."""
    g = torch.Generator().manual_seed(seed)
    N = (H // p) * (W // p)
    img = R.images_with_flat_patch(B, H, W, p, g)
    pred = R.exact_target(img, p, norm_pix) + torch.randn(B, N, 3 * p * p, generator=g, dtype=torch.float64)
    pred = pred.reshape(B * N, -1).to(dtype)
    if nan:
        idx = torch.randperm(pred.numel(), generator=g)[:7]
        pred.view(-1)[idx] = float("nan")
    mask = (torch.rand((N,) if shared else (B, N), generator=g) < 0.6).float()
    mask[..., 0], mask[..., 1] = 1.0, 0.0  # the near-constant patch is masked; both kinds exist
    return pred, img, mask


def _run(ext, pred, img, mask, p, norm_pix, fill):
    """The kernel into buffers pre-filled with 0xAA / NaN: an element it skips shows up."""
    B, N = img.shape[0], mask.shape[-1]
    outs = [torch.full_like(img, 0xAA) for _ in range(3)] + [torch.full((B, N), float("nan"), device=img.device)]
    got = ext.recon(pred, img, mask, p, norm_pix, fill, out=outs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs))
    return [t.cpu() for t in got]


def _check(ext, pred, img, mask, p, norm_pix, fill, img_dev=None):
    B, _, H, W = img.shape
    N = mask.shape[-1]
    o64 = mae_ops.reconstruct_torch(pred, img, mask, p, norm_pix, fill, fp64=True)
    o32 = mae_ops.reconstruct_torch(pred, img, mask, p, norm_pix, fill)
    dev_img = img.cuda() if img_dev is None else img_dev
    rec, paste, masked, err = _run(ext, pred.cuda(), dev_img, mask.cuda(), p, norm_pix, fill)
    rec2, paste2, masked2, err2 = _run(ext, pred.cuda(), dev_img, mask.cuda(), p, norm_pix, fill)

    # exact: masked, paste, saturation, NaN
    mpix = mae_ops._pixel_mask(mask, B, p, H, W).expand(B, 3, H, W)
    assert mpix.any() and not mpix.all()
    assert torch.equal(masked, o64["masked"])
    assert torch.equal(paste[~mpix], img[~mpix]) and torch.equal(paste[mpix], rec[mpix])
    x64 = o64["x"]
    lo, hi = x64 == 0.0, x64 == 255.0
    assert lo.sum() > 0.05 * x64.numel() and hi.sum() > 0.05 * x64.numel(), (int(lo.sum()), int(hi.sum()))
    assert (rec[lo] == 0).all() and (rec[hi] == 255).all()
    nanpix = mae_ops.unpatchify(torch.isnan(pred.float()).reshape(B, N, -1), p, H, W)
    assert (rec[nanpix] == 0).all()

    # recon bytes: the oracle's, except within delta of a rounding tie
    delta = max(2.0 * (o32["x"].double() - x64).abs().max().item(), ULP_255)
    near = ((x64 - torch.floor(x64)) - 0.5).abs() <= delta
    share = near.double().mean().item()
    diff = (rec.int() - o64["recon"].int()).abs()
    print(f"[recon] delta={delta:.3e} near-tie share={share:.2e} differing bytes={int((diff > 0).sum())}")
    assert share <= 0.01, share  # a property of the seeded inputs and the oracle alone
    assert (diff[~near] == 0).all(), int((diff[~near] > 0).sum())
    assert (diff[near] <= 1).all()

    # err: per patch, 2 x the fp32 composition's own error or one ulp
    e64 = o64["err"]
    bound = torch.maximum(2.0 * (o32["err"].double() - e64).abs(), R.ulp32(e64))
    miss = (err.double() - e64).abs()
    print(f"[recon] err: worst miss / bound = {(miss / bound).max().item():.3f}, "
          f"worst miss in ulps = {(miss / R.ulp32(e64)).max().item():.3f}")
    assert torch.isfinite(err).all() and (miss <= bound).all(), (miss / bound).max().item()

    # reruns are bit-identical
    assert torch.equal(err.view(torch.int32), err2.view(torch.int32))
    assert torch.equal(rec, rec2) and torch.equal(paste, paste2) and torch.equal(masked, masked2)
    return rec, paste, masked, err


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-sample"])
@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm-pix"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_recon_kernel(shape, dtype, norm_pix, shared):
    ext = _ext.load(True)
    B, H, W, p = shape
    nan = dtype == torch.float32 and norm_pix and not shared  # one case per shape carries NaNs
    pred, img, mask = _case(B, H, W, p, dtype, norm_pix, shared, nan, seed=H + W + p)
    assert bool(torch.isnan(pred.float()).any()) == nan
    _check(ext, pred, img, mask, p, norm_pix, fill=127 if shared else 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_recon_kernel_p16_byte_path(dtype):
    """p = 16 on an image base that is not 4-byte aligned takes the byte path; same bounds, and the
    same bytes as the word path."""
    ext = _ext.load(True)
    B, H, W, p = 2, 32, 32, 16
    pred, img, mask = _case(B, H, W, p, dtype, True, False, False, seed=11)
    buf = torch.empty(img.numel() + 1, dtype=torch.uint8, device="cuda")
    off = buf[1:].view_as(img)
    off.copy_(img)
    assert off.data_ptr() % 4 != 0 and off.is_contiguous()
    a = _check(ext, pred, img, mask, p, True, 127, img_dev=off)
    b = _check(ext, pred, img, mask, p, True, 127)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_recon_binding_validates():
    ext = _ext.load(True)
    dev = "cuda"

    def call(B=2, H=32, W=32, p=16, width=None, n_mask=None, **kw):
        N = (H // p) * (W // p) if p > 0 else 1
        pred = kw.get("pred", torch.zeros(B * N, 3 * p * p if width is None else width, device=dev))
        img = kw.get("img", torch.zeros(B, 3, H, W, dtype=torch.uint8, device=dev))
        mask = kw.get("mask", torch.ones(N if n_mask is None else n_mask, device=dev))
        return ext.recon(pred, img, mask, p, False, 127)

    assert len(call()) == 4
    with pytest.raises(RuntimeError, match="even"):
        call(H=28, W=28, p=7)  # odd patch size
    with pytest.raises(RuntimeError, match="whole number"):
        call(H=30, W=32)  # H % p != 0
    with pytest.raises(RuntimeError, match="pred must be"):
        call(width=767)
    with pytest.raises(RuntimeError, match="mask must be"):
        call(n_mask=5)
    with pytest.raises(RuntimeError, match="mask must be"):
        call(mask=torch.ones(3, 4, device=dev))  # per-sample mask of the wrong batch
    with pytest.raises(RuntimeError):
        call(pred=torch.zeros(8, 768, device=dev, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        call(img=torch.zeros(2, 3, 32, 32, device=dev))  # float images
    with pytest.raises(RuntimeError):
        call(mask=torch.ones(4))  # host mask
    with pytest.raises(RuntimeError):
        call(pred=torch.zeros(8, 1536, device=dev)[:, ::2])  # strided pred


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm-pix"])
@pytest.mark.parametrize("mask_mode", ["shared", "per-sample"])
def test_model_reconstruct_gpu_matches_cpu(mask_mode, norm_pix):
    cpu = R.tiny_model(mask_mode=mask_mode, norm_pix=norm_pix)
    gpu = R.tiny_model("cuda", torch.bfloat16, mask_mode, norm_pix, master=cpu.store.master)
    g = torch.Generator().manual_seed(4)
    B, N = 3, 4
    img = torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8)
    noise = torch.rand((N,) if mask_mode == "shared" else (B, N), generator=g)
    a = cpu.reconstruct(img, noise=noise)
    b = gpu.reconstruct(img.cuda(), noise=noise.cuda())
    assert torch.equal(a["mask"], b["mask"].cpu())
    assert torch.equal(a["masked"], b["masked"].cpu())
    mpix = mae_ops._pixel_mask(a["mask"], B, 16, 32, 32).expand(B, 3, 32, 32)
    assert torch.equal(b["paste"].cpu()[~mpix], img[~mpix])
    assert torch.equal(b["paste"].cpu()[mpix], b["recon"].cpu()[mpix])
    d = (a["psnr_masked"] - b["psnr_masked"].cpu()).abs()
    print(f"[recon] psnr cpu {a['psnr_masked'].tolist()} gpu {b['psnr_masked'].tolist()}")
    assert d.max().item() < 0.1, d  # bf16 model numerics: a loose sanity bound, not a kernel tolerance
