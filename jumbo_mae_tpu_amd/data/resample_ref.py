"""NumPy mirror of the device augment kernels (csrc/augment.hip): Pillow's bicubic resample
(Resample.c: precompute_coeffs, 22-bit fixed-point taps, horizontal pass into 8-bit rows, vertical
pass, clip8) evaluated on a crop window in the original image's coordinates, then the flip.  It is
bit-exact to ``PIL.Image.resize(size, BICUBIC, box)`` (tests/test_data.py checks that against PIL)
and is the CPU oracle of the GPU kernels (tests/test_augment_gpu.py).

The validation transform's wider descriptor (``WIN_TAB`` columns: the output is an S x S window at
(oi, oj) of a resize to oh x ow, or a pad row) is evaluated the same way -- ``coeffs`` with the full
output size and an offset, i.e. exactly the coefficients of those pixels of the full resize -- and
is bit-exact to ``Resize -> CenterCrop -> PILToTensor`` (tests/test_device_valid.py)."""

from __future__ import annotations

import math

import numpy as np

PB = 22  # Pillow PRECISION_BITS
RRC_TAB = 13  # csrc/augment.hip descriptor widths: random-resized-crop, window resize
WIN_TAB = 18


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def read_range(in_size: int, in0: float, in1: float, out_size: int, off: int, n: int) -> tuple[int, int]:
    """Input indices [first, last) that output coordinates off .. off + n - 1 of the resize of
    [in0, in1) to ``out_size`` read (the kernels' ``axis_bounds`` at both ends)."""
    in0, in1 = float(np.float32(in0)), float(np.float32(in1))
    scale = float(np.float32(in1 - in0)) / out_size
    support = 2.0 * max(scale, 1.0)
    first = max(int(in0 + (off + 0.5) * scale - support + 0.5), 0)
    last = min(int(in0 + (off + n - 1 + 0.5) * scale + support + 0.5), in_size)
    return first, last


def coeffs(in_size: int, in0: float, in1: float, out_size: int, off: int = 0, n: int | None = None):
    """Per output coordinate off .. off + n - 1 (default: all ``out_size``) of the resize of
    [in0, in1) to ``out_size``: (first input index, fixed-point taps) as Pillow computes them."""
    in0, in1 = float(np.float32(in0)), float(np.float32(in1))
    scale = float(np.float32(in1 - in0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(off, off + (out_size - off if n is None else n)):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << PB)) if v < 0 else int(0.5 + v * (1 << PB)) for v in w]
        out.append((xmin, np.array(k, dtype=np.int64)))
    return out


def _clip8(s: np.ndarray) -> np.ndarray:
    return np.where(s >= (1 << PB << 8), 255, np.where(s <= 0, 0, s >> PB)).astype(np.uint8)


def resize_window(win: np.ndarray, desc, size: int) -> np.ndarray:
    """One descriptor (csrc/augment.hip layout, 13 or 18 columns) -> uint8 [3, size, size]."""
    _, wh, ww, y0, x0, H, W, i, j, ch, cw, flip = (int(v) for v in desc[:12])
    oh, ow, oi, oj, fill = (int(v) for v in desc[13:18]) if len(desc) == WIN_TAB else (size, size, 0, 0, 0)
    if fill:  # pad row: no pixel is read
        return np.full((3, size, size), 255, np.uint8)
    a = win.reshape(wh, ww, 3).astype(np.int64)
    cv = coeffs(H, i, i + ch, oh, oi, size)
    chh = coeffs(W, j, j + cw, ow, oj, size)
    first = cv[0][0]
    last = cv[-1][0] + len(cv[-1][1])
    # the shipped window holds everything the two passes read (the kernels' debug-build checks)
    assert 0 <= oi and oi + size <= oh and 0 <= oj and oj + size <= ow, (oh, ow, oi, oj, size)
    assert y0 <= first and last <= y0 + wh, (y0, wh, first, last)
    assert all(x0 <= xmin and xmin + len(k) <= x0 + ww for xmin, k in chh), (x0, ww)
    tmp = np.zeros((last - first, size, 3), np.int64)
    for xx, (xmin, k) in enumerate(chh):
        s = (1 << (PB - 1)) + (a[first - y0:last - y0, xmin - x0:xmin - x0 + len(k), :] * k[None, :, None]).sum(1)
        tmp[:, xx, :] = _clip8(s)
    out = np.zeros((size, size, 3), np.uint8)
    for yy, (ymin, k) in enumerate(cv):
        s = (1 << (PB - 1)) + (tmp[ymin - first:ymin - first + len(k)] * k[:, None, None]).sum(0)
        out[yy] = _clip8(s)
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def unpack_packed(p) -> np.ndarray:
    """A ``data.loader.PackedImages`` batch -> uint8 [B, 3, S, S] (the kernels' result)."""
    src, tab = p.src.numpy(), p.tab.numpy()
    outs = []
    for d in tab:
        n = int(d[1]) * int(d[2]) * 3
        outs.append(resize_window(src[int(d[0]):int(d[0]) + n], d, p.size))
    out = np.stack(outs)
    chain = p.chain.numpy() if getattr(p, "chain", None) is not None else None
    if getattr(p, "mix", None) is not None:  # AugMix: W chains of D records on replicas, composited; then the rest
        from .augment_ref import apply_chain, augmix_mix
        W, D, blended = p.mix_wdb
        recs = np.ascontiguousarray(chain[:, :W * D]).reshape(len(out) * W, D, chain.shape[2])
        out = augmix_mix(out, apply_chain(np.repeat(out, W, axis=0), recs), p.mix.numpy(), bool(blended))
        out = apply_chain(out, chain[:, W * D:])
    elif chain is not None:  # RandAugment / AutoAugment / ColorJitter records
        from .augment_ref import apply_chain
        out = apply_chain(out, chain)
    if getattr(p, "erase", None) is not None:  # RandomErasing boxes
        from .augment_ref import erase_paste
        out = erase_paste(out, p.erase.numpy(), p.fill.numpy())
    return out


def taps(c: int, out: int) -> int:
    return math.ceil(2.0 * max(c / out, 1.0)) * 2 + 1
