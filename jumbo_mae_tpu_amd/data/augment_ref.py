"""NumPy mirror of the device op chain (csrc/augment_chain.hip): RandAugment / AutoAugment /
ColorJitter ops on a uint8 [3, S, S] image from the records of data/autoaugment.py, bit-exact to the
PIL calls they describe (tests/test_device_randaug.py pins every kind against PIL) and the CPU
oracle of the kernels (tests/test_randaug_gpu.py).

Arithmetic, as Pillow does it:
* ImageEnhance.{Color, Brightness, Contrast, Sharpness} = blend(degenerate, image, f) in float32,
  t = d + f (i - d); truncated for 0 <= f <= 1, else clipped to [0, 255] and truncated.
  Degenerates: the ITU-R 601 luma (19595 R + 38470 G + 7471 B + 0x8000) >> 16; black; the constant
  int(mean(luma) + 0.5); the 3x3 SMOOTH filter (float32 taps (1 1 1 / 1 5 1 / 1 1 1) / 13 summed onto
  0.5 row by row, border copied).
* Image.transform(AFFINE): source coordinates in double at pixel centres, fill outside
  [0, W) x [0, H), bilinear / bicubic (a = -0.5 Catmull-Rom in Pillow's p1..p4 form) in double with
  edge-clamped neighbours.
* ImageOps.equalize / autocontrast: per-band histogram -> lookup table.
* AugMix (``augmix_mix``): ``mixed += w_k * chain_k`` in float32 (multiply and add rounded
  separately), clipped and truncated, then Image.blend(original, mixed, m) -- the blend above; the
  ``blended`` variant is a sequence of those blends.  RandomErasing (``erase_paste``): a byte copy of
  the worker-drawn fill.  Both are pinned to PIL / the host transform in
  tests/test_device_erase_augmix.py and are the oracle of tests/test_erase_augmix_gpu.py.
"""

from __future__ import annotations

import numpy as np

from .autoaugment import (AUG_KINDS, AUG_P, K_AFFINE, K_AUTOCONTRAST, K_BRIGHTNESS, K_COLOR, K_CONTRAST, K_EQUALIZE,
                          K_IDENTITY, K_INVERT, K_POSTERIZE, K_SHARPNESS, K_SOLARIZE, K_SOLARIZE_ADD)

BILINEAR, BICUBIC = 2, 3  # PIL.Image.Resampling values, as shipped in the records


def luma(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.int64)
    return (19595 * a[0] + 38470 * a[1] + 7471 * a[2] + 0x8000) >> 16


def blend(deg: np.ndarray, img: np.ndarray, f: float) -> np.ndarray:
    f = np.float32(f)
    t = deg.astype(np.float32) + f * (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    if not (np.float32(0) <= f <= np.float32(1)):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def smooth(a: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH of a [3, H, W] image."""
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)).reshape(3, 3)
    out = a.copy()
    if a.shape[1] < 3 or a.shape[2] < 3:
        return out
    f = a.astype(np.float32)
    H, W = a.shape[1:]
    ss = np.full((3, H - 2, W - 2), 0.5, np.float32)
    for dy in range(3):
        row = f[:, dy:dy + H - 2]
        ss = ss + ((row[:, :, 0:W - 2] * k[dy, 0] + row[:, :, 1:W - 1] * k[dy, 1]) + row[:, :, 2:W] * k[dy, 2])
    out[:, 1:-1, 1:-1] = np.clip(ss, 0, 255).astype(np.uint8)
    return out


def equalize_lut(h: np.ndarray) -> np.ndarray:
    """ImageOps.equalize's table of one band from its 256-bin histogram."""
    nz = h[h > 0]
    lut = np.arange(256, dtype=np.int64)
    if len(nz) <= 1:
        return lut.astype(np.uint8)
    step = int(nz.sum() - nz[-1]) // 255
    if not step:
        return lut.astype(np.uint8)
    n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(n // step, 255).astype(np.uint8)


def autocontrast_lut(h: np.ndarray) -> np.ndarray:
    nz = np.nonzero(h)[0]
    lut = np.arange(256, dtype=np.int64)
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return lut.astype(np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((np.arange(256) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def affine(a: np.ndarray, m, resample: int, fill) -> np.ndarray:
    _, H, W = a.shape
    ys, xs = np.mgrid[0:H, 0:W]
    xin = (m[0] * (xs + 0.5) + m[1] * (ys + 0.5)) + m[2]
    yin = (m[3] * (xs + 0.5) + m[4] * (ys + 0.5)) + m[5]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - x0, yin - y0
    f = a.astype(np.float64)

    def px(yy, xx):
        return f[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]

    if resample == BILINEAR:
        def row(yy):
            left, right = px(yy, x0), px(yy, x0 + 1)
            return left + (right - left) * dx
        v1, v2 = row(y0), row(y0 + 1)
        v = v1 + (v2 - v1) * dy
    elif resample == BICUBIC:
        def cubic(v1, v2, v3, v4, d):
            p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
            return p1 + d * (p2 + d * (p3 + d * p4))

        def row(yy):
            return cubic(px(yy, x0 - 1), px(yy, x0), px(yy, x0 + 1), px(yy, x0 + 2), dx)
        v = np.clip(cubic(row(y0 - 1), row(y0), row(y0 + 1), row(y0 + 2), dy), 0.0, 255.0)
    else:
        raise ValueError(f"resample {resample}")
    out = np.empty_like(a)
    for c in range(3):
        out[c] = np.where(inside, v[c].astype(np.uint8), np.uint8(int(fill[c])))
    return out


def apply_op(a: np.ndarray, rec) -> np.ndarray:
    """One record (data/autoaugment.py op_record) on a uint8 [3, S, S] image."""
    kind, arg = int(rec[0]), rec[1]
    if kind == K_IDENTITY:
        return a.copy()
    i = np.arange(256, dtype=np.int64)
    if kind == K_INVERT:
        return (255 - i).astype(np.uint8)[a]
    if kind == K_POSTERIZE:
        return (i & ~(2 ** (8 - int(arg)) - 1)).astype(np.uint8)[a]
    if kind == K_SOLARIZE:
        return np.where(i < int(arg), i, 255 - i).astype(np.uint8)[a]
    if kind == K_SOLARIZE_ADD:
        return np.where(i < 128, np.minimum(i + int(arg), 255), i).astype(np.uint8)[a]
    if kind in (K_AUTOCONTRAST, K_EQUALIZE):
        make = autocontrast_lut if kind == K_AUTOCONTRAST else equalize_lut
        return np.stack([make(np.bincount(a[c].reshape(-1), minlength=256))[a[c]] for c in range(3)])
    if kind == K_COLOR:
        return blend(np.broadcast_to(luma(a), a.shape), a, arg)
    if kind == K_BRIGHTNESS:
        return blend(np.zeros_like(a), a, arg)
    if kind == K_CONTRAST:
        L = luma(a)
        mean = int(int(L.sum()) / L.size + 0.5)
        return blend(np.full_like(a, mean), a, arg)
    if kind == K_SHARPNESS:
        return blend(smooth(a), a, arg)
    if kind == K_AFFINE:
        return affine(a, rec[2:8], int(rec[8]), rec[9:12])
    raise ValueError(f"unknown op kind {kind}")


def apply_chain(images: np.ndarray, chain: np.ndarray) -> np.ndarray:
    """uint8 [B, 3, S, S] and records [B, slots, AUG_P] -> the chained result (aug_chain's)."""
    assert chain.shape[0] == images.shape[0] and chain.shape[2] == AUG_P and AUG_KINDS == 12
    out = []
    for a, recs in zip(images, chain):
        for rec in recs:
            a = apply_op(a, rec)
        out.append(a)
    return np.stack(out)


def augmix_mix(orig: np.ndarray, chains: np.ndarray, table: np.ndarray, blended: bool) -> np.ndarray:
    """AugMix's composite (augmix_mix_kernel): orig uint8 [B, 3, S, S], chains uint8 [B * W, 3, S, S]
    (chain k of image b at b * W + k), table float32 [B, W + 1] (AugMix.describe).  Not blended:
    ``mixed += w_k * chain_k`` in float32, clipped and truncated, then Image.blend(orig, mixed, m);
    blended: Image.blend(img, chain_k, a_k) step by step."""
    B, W = table.shape[0], table.shape[1] - 1
    assert table.dtype == np.float32 and W >= 1 and chains.shape == (B * W, *orig.shape[1:]), (table.shape, chains.shape)
    out = np.empty_like(orig)
    for b in range(B):
        if blended:
            img = orig[b]
            for k in range(W):
                img = blend(img, chains[b * W + k], table[b, k])
            out[b] = img
            continue
        mixed = np.zeros(orig.shape[1:], np.float32)
        for k in range(W):
            mixed += table[b, k] * chains[b * W + k].astype(np.float32)
        out[b] = blend(orig[b], np.clip(mixed, 0, 255).astype(np.uint8), table[b, W])
    return out


def erase_paste(images: np.ndarray, table: np.ndarray, fill: np.ndarray) -> np.ndarray:
    """RandomErasing's paste (erase_paste_kernel): images uint8 [B, 3, S, S], table int64 [B, 5] = box
    i, j, eh, ew (eh 0: not erased) and the offset of its [3, eh, ew] bytes in the flat uint8 fill."""
    out = images.copy()
    for a, (i, j, eh, ew, off) in zip(out, table.tolist()):
        if eh:
            a[:, i:i + eh, j:j + ew] = fill[off:off + 3 * eh * ew].reshape(3, eh, ew)
    return out
