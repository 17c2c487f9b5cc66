"""Independent reference of the axial 2-D rotary embedding (ops/rope.py) for the tests: complex
numbers, exact fp64 angles (no table), one explicit loop over the q / k slots."""

import numpy as np


def rope_complex(qkv: np.ndarray, heads: int, n_cls: int, gw: int, theta: float, pos=None, inverse=False,
                 table=None) -> np.ndarray:
    """qkv fp64 [B, S, 3 * heads * hd] -> rotated copy.  Channel pair (2i, 2i + 1) of a head is the complex
    number x0 + i x1; pairs [0, hd/4) are multiplied by exp(i y w_i), pairs [hd/4, hd/2) by exp(i x w_i),
    w_i = theta^(-i / (hd/4)).  ``table`` ([G, hd/4, 2] of (cos, sin)): take the unit numbers from it instead
    (the kernel tests feed every implementation the same rounded table)."""
    B, S, W = qkv.shape
    hd = W // (3 * heads)
    n = hd // 4
    out = np.array(qkv, dtype=np.float64, copy=True).reshape(B, S, 3, heads, hd)
    w = np.float64(theta) ** (-np.arange(n, dtype=np.float64) / n)
    for b in range(B):
        for t in range(n_cls, S):
            if pos is None:
                p = t - n_cls
            else:
                pp = np.asarray(pos)
                p = int(pp[t - n_cls] if pp.ndim == 1 else pp[b, t - n_cls])
            y, x = divmod(p, gw)
            if table is None:
                u = np.concatenate([np.exp(1j * y * w), np.exp(1j * x * w)])
            else:
                tb = np.asarray(table, dtype=np.float64)
                u = np.concatenate([tb[y, :, 0] + 1j * tb[y, :, 1], tb[x, :, 0] + 1j * tb[x, :, 1]])
            if inverse:
                u = np.conj(u)
            for which in (0, 1):
                z = out[b, t, which, :, 0::2] + 1j * out[b, t, which, :, 1::2]  # [heads, hd/2]
                z = z * u[None, :]
                out[b, t, which, :, 0::2] = z.real
                out[b, t, which, :, 1::2] = z.imag
    return out.reshape(B, S, W)
