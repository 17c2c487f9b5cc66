"""fp64 references, inputs and the shared comparison rules of the MAE glue kernel tests
(csrc/mae.hip): tests/test_mae_glue_structured_gpu.py runs the kernels against them,
tests/test_mae_ref.py keeps this module honest without a GPU (the references against the project's
torch compositions, the bf16 helpers, the near-tie share of every seeded case).

Nothing here touches the extension.  Every reference is fp64 on the fp32 normalisation constants
and on the inputs as stored (bf16 predictions, the fp32 mixup ratio).

Comparison rules (those of tests/test_recon_gpu.py)
  fp32 output   |out - ref64| <= max(2 |fp32 torch composition - ref64|, 1 fp32 ulp of ref64) per element.
  bf16 output   out == bf16_rne(ref64) bit for bit, except where ref64 lies within
                delta = max(2 |fp32 composition - ref64|, 1 fp32 ulp) of the midpoint between two bf16
                values: there either neighbour passes.  At most 1 % of an output may be excused that
                way, a property of the seeded inputs that the CPU test asserts on the references alone.
Both margins come from the composition, never from the kernel.
"""

from __future__ import annotations

import functools

import torch

from recon_ref import FLAT_RGB, exact_target, images_with_flat_patch, ulp32  # noqa: F401 (re-exported)
from jumbo_mae_tpu_amd.data.constants import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
from jumbo_mae_tpu_amd.ops import mae as mae_ops
from jumbo_mae_tpu_amd.utils.mae import extract_patches_nchw
from jumbo_mae_tpu_amd.utils.mixup import Mixup

F64 = torch.float64
NEAR_TIE_CAP = 0.01


# ------------------------------------------------------------------ bf16 helpers
def _bf16_spacing(x64):
    """Spacing of bf16 (8 significant bits, exponents of fp32) at |x|, fp64."""
    _, e = torch.frexp(x64.abs())  # |x| = m 2^e, m in [0.5, 1); frexp(0) = (0, 0)
    e = torch.where(x64 == 0, torch.full_like(e, -125), e).clamp(min=-125)
    return torch.ldexp(torch.ones_like(x64), e - 8)


def bf16_rne(x64):
    """The bf16 value nearest to each fp64 value, ties to even, rounded ONCE (torch's
    double -> bfloat16 goes through fp32).  Returns a bfloat16 tensor; finite inputs below the
    bf16 overflow threshold only."""
    assert x64.dtype == F64
    q = _bf16_spacing(x64)
    r = torch.round(x64 / q) * q  # torch.round is half-to-even; x / q and r are exact in fp64
    out = r.to(torch.bfloat16)
    assert torch.equal(out.double(), r)
    return out


def bf16_tie_distance(x64):
    """Distance of each fp64 value to the nearest midpoint between two adjacent bf16 values."""
    q = _bf16_spacing(x64)
    u = x64.abs() / q
    return ((u - torch.floor(u)) - 0.5).abs() * q


def bits16(t):
    return t.contiguous().view(torch.int16)


def near_tie(ref64, comp32):
    """(mask of the elements that may round either way, delta) of a bf16 output."""
    delta = torch.maximum(2.0 * (comp32.double() - ref64).abs(), ulp32(ref64))
    return bf16_tie_distance(ref64) <= delta, delta


def near_tie_share(ref64, comp32):
    return near_tie(ref64, comp32)[0].double().mean().item()


def check_bf16(out, ref64, comp32, label, cap=NEAR_TIE_CAP):
    """The bf16 rule.  ``out`` bf16 on the CPU, shaped like ref64."""
    assert out.dtype == torch.bfloat16 and out.shape == ref64.shape, (out.dtype, out.shape, ref64.shape)
    near, delta = near_tie(ref64, comp32)
    share = near.double().mean().item()
    want = bf16_rne(ref64)
    same = bits16(out) == bits16(want)
    q = _bf16_spacing(ref64)
    step = (out.double() - want.double()).abs()
    print(f"[mae] {label}: delta max={delta.max().item():.3e} near-tie share={share:.2e} "
          f"differing={int((~same).sum())} of {same.numel()}")
    assert share <= cap, (label, share)
    assert same[~near].all(), (label, int((~same[~near]).sum()))
    assert (step[near] <= q[near]).all(), label  # the other neighbour of the tie, nothing further
    return share


def check_f32(out, ref64, comp32, label):
    """The fp32 rule.  ``out`` fp32 on the CPU, shaped like ref64."""
    assert out.dtype == torch.float32 and out.shape == ref64.shape, (out.dtype, out.shape, ref64.shape)
    bound = torch.maximum(2.0 * (comp32.double() - ref64).abs(), ulp32(ref64))
    miss = (out.double() - ref64).abs()
    ratio = (miss / bound).max().item()
    print(f"[mae] {label}: worst miss / bound = {ratio:.3f}, worst miss in ulps = "
          f"{(miss / ulp32(ref64)).max().item():.3f}")
    assert torch.isfinite(out).all() and (miss <= bound).all(), (label, ratio)
    return ratio


# ------------------------------------------------------------------ images
def coded_images(B, H, W):
    """img[b, c, y, x] = (17 b + 85 c + 7 y + 13 x) % 256: any swap of b / c / y / x or H / W moves a value."""
    b = torch.arange(B).view(B, 1, 1, 1)
    c = torch.arange(3).view(1, 3, 1, 1)
    y = torch.arange(H).view(1, 1, H, 1)
    x = torch.arange(W).view(1, 1, 1, W)
    return ((17 * b + 85 * c + 7 * y + 13 * x) % 256).to(torch.uint8)


def random_coded_images(B, H, W, seed):
    """The position code plus seeded random bytes (mod 256)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 256, (B, 3, H, W), generator=g)
    return ((coded_images(B, H, W).long() + r) % 256).to(torch.uint8)


def byte_table_images(B, H, W):
    """Every channel of every image holds each byte value 0..255 (H W >= 256), at places that
    differ between channels and images."""
    assert H * W >= 256
    i = torch.arange(H * W).view(1, 1, H * W)
    b = torch.arange(B).view(B, 1, 1)
    c = torch.arange(3).view(1, 3, 1)
    return ((i + 37 * c + 101 * b) % 256).to(torch.uint8).view(B, 3, H, W)


def paint_special_patches(img, p):
    """In place: patch (0, 0) of image 0 = FLAT_RGB, the last patch of image 0 all 0, patch 1 of
    the last image all 255.  Returns the (image, patch) rows painted."""
    B, _, H, W = img.shape
    gw = W // p
    N = (H // p) * gw
    assert N >= 3
    for c in range(3):
        img[0, c, :p, :p] = FLAT_RGB[c]
    y, x = ((N - 1) // gw) * p, ((N - 1) % gw) * p
    img[0, :, y:y + p, x:x + p] = 0
    y, x = (1 // gw) * p, (1 % gw) * p
    img[B - 1, :, y:y + p, x:x + p] = 255
    return {"flat": 0, "zero": N - 1, "full": (B - 1) * N + 1}


def special_images(B, H, W, p, seed=None):
    img = coded_images(B, H, W) if seed is None else random_coded_images(B, H, W, seed)
    rows = paint_special_patches(img, p)
    return img, rows


# ------------------------------------------------------------------ exactly representable activations
def small_int_bf16(shape, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.bfloat16)


def dyadic_f32(shape, gen):
    """Multiples of 1/16 in [-4, 4]: sums of thousands of them, and of small integers, are exact in fp32."""
    return torch.randint(-64, 65, shape, generator=gen).float() / 16.0


# ------------------------------------------------------------------ references
def _const64():
    m = torch.tensor(IMAGENET_DEFAULT_MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    s = torch.tensor(IMAGENET_DEFAULT_STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    return m, s


def normalized64(img):
    m, s = _const64()
    return (img.double() / 255.0 - m) / s


def patch_index(H, W, p):
    """Offsets into one flattened [3, H, W] image of element o = (ph, pw, c) of patch n: [N, 3p^2]."""
    gw = W // p
    n = torch.arange((H // p) * gw).view(-1, 1)
    o = torch.arange(3 * p * p).view(1, -1)
    ph, pw, c = o // (3 * p), (o // 3) % p, o % 3
    return (c * H + (n // gw) * p + ph) * W + (n % gw) * p + pw


def patches_of(x, p):
    """[B, 3, H, W] -> [B, N, 3p^2] in (ph, pw, c) order, by explicit offsets."""
    B, _, H, W = x.shape
    return x.reshape(B, -1)[:, patch_index(H, W, p)]


def patches64(img, p):
    return patches_of(normalized64(img), p)


def patches32(img, p):
    """The fp32 torch composition of the normalized patches."""
    return extract_patches_nchw(mae_ops.normalize_images(img), p)


def _take(t, ids):
    """t [B, N, ...] rows ids [K] (shared) or [B, K] -> [B, K, ...]."""
    ids = ids.long()
    if ids.dim() == 1:
        return t[:, ids]
    return torch.stack([t[b, ids[b]] for b in range(t.shape[0])])


def gather64(img, ids, p):
    t = _take(exact_target(img, p, False), ids)
    return t.reshape(-1, t.shape[-1])


def gather32(img, ids, p):
    t = _take(patches32(img, p), ids)
    return t.reshape(-1, t.shape[-1])


def box_mask(H, W, box):
    y0, y1, x0, x1 = box
    y = torch.arange(H).view(H, 1)
    x = torch.arange(W).view(1, W)
    return (y >= y0) & (y < y1) & (x >= x0) & (x < x1)


def mix64(img, p, mode, ratio, perm, box):
    """mode 0: x[b]; 1: r x[b] + (1 - r) x[perm[b]] with r the fp32 value of ``ratio``;
    2: x[perm[b]] inside the pixel box (y0, y1, x0, x1), x[b] elsewhere.  [B*N, 3p^2] fp64."""
    x = normalized64(img)
    if mode == 1:
        r = torch.tensor(ratio, dtype=torch.float32).double().item()
        x = r * x + (1.0 - r) * x[perm.long()]
    elif mode == 2:
        x = torch.where(box_mask(img.shape[2], img.shape[3], box), x[perm.long()], x)
    t = patches_of(x, p)
    return t.reshape(-1, t.shape[-1])


def mix_plan(mode, ratio, perm, box):
    """The host side of ``Mixup.plan`` for a chosen decision (None: no mixing)."""
    if mode == 0:
        return None
    return {"mode": "mixup" if mode == 1 else "cutmix", "ratio": float(ratio), "perm": perm.long(),
            "box": tuple(box) if box is not None else None}


def mix32(img, p, mode, ratio, perm, box):
    x = Mixup.mix_images(mae_ops.normalize_images(img), mix_plan(mode, ratio, perm, box))
    t = extract_patches_nchw(x, p)
    return t.reshape(-1, t.shape[-1])


def embed_finish64(e, pos, ids, cls, B):
    """e bf16 [B*K, D], pos fp32 [N, D] or None, ids [K] / [B, K], cls fp32 [C, D] -> [B, C+K, D]."""
    D = e.shape[-1]
    K = ids.shape[-1]
    ev = e.double().view(B, K, D)
    if pos is not None:
        ev = ev + _take(pos.double().unsqueeze(0).expand(B, -1, -1), ids)
    return torch.cat([cls.double().view(1, -1, D).expand(B, -1, -1), ev], 1)


def _restore2(restore, B):
    r = restore.long()
    return r.unsqueeze(0).expand(B, -1) if r.dim() == 1 else r


def unshuffle_fwd64(y, tok, restore, pos, C):
    """y bf16 [B, C+K, d], tok fp32 [d], restore [N] / [B, N], pos fp32 [N, d] -> fp64 [B, C+N, d]."""
    B, CK, d = y.shape
    K = CK - C
    N = pos.shape[0]
    j = _restore2(restore, B)
    out = torch.empty(B, C + N, d, dtype=F64)
    out[:, :C] = y[:, :C].double()
    for b in range(B):
        for n in range(N):
            src = y[b, C + j[b, n]].double() if j[b, n] < K else tok.double()
            out[b, C + n] = src + pos[n].double()
    return out


def unshuffle_bwd64(dout, restore, C, K):
    """dout fp32 [B, C+N, d] -> (dy fp64 [B, C+K, d] = the rows of dout gathered, dtok fp64 [d])."""
    B, CN, d = dout.shape
    N = CN - C
    j = _restore2(restore, B)
    dy = torch.zeros(B, C + K, d, dtype=F64)
    dtok = torch.zeros(d, dtype=F64)
    dy[:, :C] = dout[:, :C].double()
    for b in range(B):
        for n in range(N):
            if j[b, n] < K:
                dy[b, C + j[b, n]] = dout[b, C + n].double()
            else:
                dtok += dout[b, C + n].double()
    return dy, dtok


def patch_mse64(pred, img, p, norm_pix):
    """pred bf16 [B*N, 3p^2] as stored -> fp64 [B*N]."""
    t = exact_target(img, p, norm_pix).reshape(pred.shape)
    return (t - pred.double()).square().mean(-1)


def patch_mse_bwd64(pred, img, dmse, p, norm_pix):
    t = exact_target(img, p, norm_pix).reshape(pred.shape)
    return (dmse.double() * 2.0 / pred.shape[-1]).unsqueeze(-1) * (pred.double() - t)


def target32(img, p, norm_pix):
    t = patches32(img, p)
    return mae_ops.norm_pix(t) if norm_pix else t


def patch_mse32(pred, img, p, norm_pix):
    t = target32(img, p, norm_pix).reshape(pred.shape)
    return (t - pred.float()).square().mean(-1)


def patch_mse_bwd32(pred, img, dmse, p, norm_pix):
    """Autograd of the fp32 composition."""
    pr = pred.float().requires_grad_()
    t = target32(img, p, norm_pix).reshape(pred.shape)
    (t - pr).square().mean(-1).backward(dmse)
    return pr.grad


def mask_ids_ref(noise, keep):
    """Stable ranks of noise [R, N]: (shuffle, restore, keep ids, mask), by counting."""
    x = noise.double()
    R, N = x.shape
    xi, xj = x.unsqueeze(2), x.unsqueeze(1)  # [R, i, 1], [R, 1, j]
    before = (xj < xi) | ((xj == xi) & (torch.arange(N).view(1, 1, N) < torch.arange(N).view(1, N, 1)))
    rank = before.sum(-1)
    shuffle = torch.empty_like(rank)
    shuffle.scatter_(1, rank, torch.arange(N).expand(R, N))
    return shuffle, rank, shuffle[:, :keep], (rank >= keep).float()


# ------------------------------------------------------------------ the patch-MSE cases
# (B, H, W, p): the kernel each one runs is in the table of tests/test_mae_glue_structured_gpu.py
MSE_SHAPES = [(3, 32, 48, 16), (1, 28, 42, 14), (1, 24, 36, 12), (2, 16, 24, 8), (3, 8, 12, 4), (1, 36, 54, 18)]
PATCH_SHAPES = [(2, 32, 48, 16), (1, 28, 42, 14), (2, 16, 24, 8), (3, 8, 12, 4), (1, 4, 6, 2)]


@functools.lru_cache(maxsize=None)
def mse_case(B, H, W, p, norm_pix):
    """Inputs and references of one patch-MSE case, computed once and shared (treat as read-only)."""
    g = torch.Generator().manual_seed(1000 * p + H + W + int(norm_pix))
    img, special = special_images(B, H, W, p)
    N = (H // p) * (W // p)
    rows, P3 = B * N, 3 * p * p
    pred = (exact_target(img, p, norm_pix) + torch.randn(B, N, P3, generator=g, dtype=F64)).reshape(rows, P3)
    pred = pred.to(torch.bfloat16)
    dmse = torch.randn(rows, generator=g)
    dmse[::3] = 0.0
    return {"img": img, "pred": pred, "dmse": dmse, "special": special, "rows": rows, "P3": P3,
            "mse64": patch_mse64(pred, img, p, norm_pix), "mse32": patch_mse32(pred, img, p, norm_pix),
            "dpred64": patch_mse_bwd64(pred, img, dmse, p, norm_pix),
            "dpred32": patch_mse_bwd32(pred, img, dmse, p, norm_pix)}


def patch_images(B, H, W, p):
    """Images of the gather / mix / patchify cases: the byte table where it fits, else the position
    code; one seeded random image where B = 3; the special patches painted where B > 1.  At 32 x 48
    what the painting leaves still holds every (channel, byte) pair (tests/test_mae_ref.py)."""
    img = byte_table_images(B, H, W) if H * W >= 256 else coded_images(B, H, W)
    if B > 2:
        img[1] = random_coded_images(1, H, W, seed=H + W)[0]
    if B > 1:
        paint_special_patches(img, p)
    return img


def gather_ids(B, N, seed):
    """name -> int32 ids, shared [K] and per-sample [B, K]: K = N, K = 1, K = 0, and a K = 3 set that
    holds patch 0 and patch N - 1."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, K in (("all", N), ("one", 1), ("none", 0), ("ends", min(3, N))):
        sh = torch.randperm(N, generator=g)[:K]
        ps = torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(B)])
        if name == "ends":
            sh[0], sh[-1] = N - 1, 0
            ps[:, 0], ps[:, -1] = 0, N - 1
        if name == "one":
            sh[0] = N - 1
            ps[:, 0] = torch.arange(B) % N
        out[name + "-shared"] = sh.to(torch.int32)
        out[name + "-per-sample"] = ps.to(torch.int32)
    return out


MIX_BOXES = {"unaligned": (5, 27, 3, 41), "pixel": (9, 10, 17, 18), "empty": (7, 7, 3, 20), "full": None}
MIX_RATIOS = (0.0, 0.3, 0.5, 1.0)


MIX_SHAPES = [(3, 32, 48, 16), (3, 32, 48, 8)]  # mix_patches16_kernel, mix_patches_kernel


def mix_box(name, H, W):
    return (0, H, 0, W) if name == "full" else MIX_BOXES[name]


def mix_perm(B):
    """One fixed point (the last image) and one cycle over the rest."""
    assert B >= 3
    perm = torch.arange(B)
    perm[:B - 1] = torch.roll(torch.arange(B - 1), 1)
    return perm.to(torch.int32)
