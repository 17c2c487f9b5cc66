"""NumPy fp64 mirror of QK-norm, written from the definition in ops/qknorm.py (loops over the rows,
the rotation through complex numbers as in tests/rope_ref.py) -- not from ``qknorm_torch``."""

import numpy as np

from rope_ref import rope_complex

EPS = 1e-6


def qknorm_np(qkv, heads, g_q, g_k, rope=None):
    """``qkv`` [B, S, 3 * heads * hd] -> (out, pre): ``out`` the normalised tensor, rotated when
    ``rope`` = (n_cls, gw, theta, pos | None, table | None) as tests/rope_ref.py takes them; ``pre`` [B, S, 3, heads, hd] the normalised tensor
    before the rotation (what the GPU tests' error bound is stated over).  v is copied."""
    x = np.asarray(qkv, np.float64)
    B, S, W = x.shape
    hd = W // (3 * heads)
    x5 = x.reshape(B, S, 3, heads, hd)
    pre = x5.copy()
    for s, g in ((0, g_q), (1, g_k)):
        g = np.asarray(g, np.float64)
        for b in range(B):
            for t in range(S):
                for h in range(heads):
                    row = x5[b, t, s, h]
                    r = 1.0 / np.sqrt(np.dot(row, row) / hd + EPS)
                    pre[b, t, s, h] = row * r * g
    out = pre.reshape(B, S, W)
    if rope is not None:
        n_cls, gw, theta, pos, table = rope
        out = rope_complex(out, heads, n_cls, gw, theta, pos, False, table)
    return out, pre


def qknorm_bwd_np(dy, qkv, heads, g_q, g_k, rope=None):
    """(dx [B, S, 3 * heads * hd] with the v third of ``dy`` passed through, dg_q, dg_k) by the
    definition's backward formulas."""
    x = np.asarray(qkv, np.float64)
    d = np.asarray(dy, np.float64)
    B, S, W = x.shape
    hd = W // (3 * heads)
    if rope is not None:
        n_cls, gw, theta, pos, table = rope
        d = rope_complex(d, heads, n_cls, gw, theta, pos, True, table)
    x5, u5 = x.reshape(B, S, 3, heads, hd), d.reshape(B, S, 3, heads, hd)
    dx = np.asarray(dy, np.float64).reshape(B, S, 3, heads, hd).copy()
    dg = [np.zeros(hd), np.zeros(hd)]
    for s, g in ((0, g_q), (1, g_k)):
        g = np.asarray(g, np.float64)
        for b in range(B):
            for t in range(S):
                for h in range(heads):
                    row, u = x5[b, t, s, h], u5[b, t, s, h]
                    r = 1.0 / np.sqrt(np.dot(row, row) / hd + EPS)
                    xh, tt = row * r, u * g
                    dx[b, t, s, h] = r * (tt - xh * np.mean(tt * xh))
                    dg[s] += u * xh
    return dx.reshape(B, S, W), dg[0], dg[1]
