"""Exact reference and input builders of the attention monitor's tests (ops/attn_stats.py).

``ref_rows``: (ENT, PMAX, CLS, ZMAX) of every attention row in fp64 from the bf16 values -- the logits
by an fp64 contraction (products of bf16 values are exact in fp64), the sums over the keys by
``math.fsum``.  ``ref_table``: the ``[H, 6]`` reduction of given fp32 row values, again by ``math.fsum``,
with ``S*`` (the sums of magnitudes) for the bound ``n 2^-53 S*``.  Rules for non-finite logits: the
module docstring of ops/attn_stats.py.
"""

import math

import numpy as np
import torch

COLS = ("ENT_SUM", "PMAX_SUM", "CLS_SUM", "ZMAX", "BAD", "N")
U53 = 2.0 ** -53


def logits(qkv: torch.Tensor, heads: int) -> np.ndarray:
    """fp64 [B, H, S, S]: (q . k) / sqrt(hd)."""
    B, S, D3 = qkv.shape
    hd = D3 // 3 // heads
    x = qkv.detach().cpu().double().numpy().reshape(B, S, 3, heads, hd)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / math.sqrt(hd)


def ref_rows(qkv: torch.Tensor, heads: int, n_cls: int):
    """(rows fp64 [B, H, S, 4], zabs fp64 [B, H, S]): the exact row values and max_k |z| of each row."""
    z = logits(qkv, heads)
    B, H, S, _ = z.shape
    rows = np.empty((B, H, S, 4))
    zabs = np.zeros((B, H, S))
    for b in range(B):
        for h in range(H):
            for q in range(S):
                zr = z[b, h, q]
                ok = zr[~np.isnan(zr)]
                m = ok.max() if ok.size else -math.inf
                zabs[b, h, q] = np.abs(zr[np.isfinite(zr)]).max() if np.isfinite(zr).any() else 0.0
                if np.isnan(zr).any() or not math.isfinite(m):
                    rows[b, h, q] = (math.nan, math.nan, math.nan, m)
                    continue
                d = zr - m  # -inf stays -inf: e = 0
                e = np.exp(d)
                l = math.fsum(e.tolist())
                t = math.fsum((e[e > 0] * d[e > 0]).tolist())
                c = math.fsum(e[:n_cls].tolist())
                rows[b, h, q] = (math.log(l) - t / l, 1.0 / l, c / l, m)
    return rows, zabs


def ref_table(rows: torch.Tensor):
    """(table fp64 [H, 6], mags fp64 [H, 3]) of fp32 row values [B, H, S, 4]: the definition's reduction
    with ``math.fsum`` and the sums of magnitudes of columns 0-2."""
    r = rows.detach().cpu().double().numpy()
    B, H, S, _ = r.shape
    tab, mags = np.empty((H, 6)), np.empty((H, 3))
    for h in range(H):
        x = r[:, h].reshape(-1, 4)
        good = np.isfinite(x[:, 0])
        for j in range(3):
            tab[h, j] = math.fsum(x[good, j].tolist())
            mags[h, j] = math.fsum(np.abs(x[good, j]).tolist())
        tab[h, 3] = x[good, 3].max() if good.any() else -math.inf
        tab[h, 4] = float((~good).sum())
        tab[h, 5] = float(B * S)
    return torch.from_numpy(tab), torch.from_numpy(mags)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """fp64: the spacing of fp32 at |x| (that of the smallest normal below it)."""
    a = x.abs().double().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ------------------------------------------------------------------------------ inputs
def random_qkv(B, S, H, hd, seed=0, gain=1.0, dtype=torch.bfloat16):
    """Standard normal q and k (logits ~ N(0, gain^2)); per head h the keys are scaled by 1 + h / 2, so the
    heads of one tensor range from diffuse to peaked attention."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, H, hd, generator=g)
    x[:, :, 1] *= gain * (1.0 + 0.5 * torch.arange(H, dtype=torch.float32)).view(1, 1, H, 1)
    return x.reshape(B, S, 3 * H * hd).to(dtype)


def exact_qkv(B, S, H, hd=64, seed=0, amp=4):
    """Integers in [-amp, amp]: every product and partial sum is an exact fp32 integer (hd amp^2 < 2^24) and
    with hd = 64 every logit a multiple of 1/8."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-amp, amp + 1, (B, S, 3, H, hd), generator=g).float()
    return x.reshape(B, S, 3 * H * hd).to(torch.bfloat16)


def equal_keys_qkv(B, S, H, hd=64, seed=0):
    """All keys of a (b, h) equal: uniform attention, ENT = log S, PMAX = 1 / S, CLS = n_cls / S."""
    x = exact_qkv(B, S, H, hd, seed).view(B, S, 3, H, hd).clone()
    x[:, :, 1] = x[:, :1, 1]
    return x.reshape(B, S, 3 * H * hd)


def one_ahead_qkv(B, S, H, hd=64, key=None):
    """Logit 256 at one key (the last unless ``key`` is given) and 0 elsewhere: ENT = 0, PMAX = 1."""
    x = torch.zeros(B, S, 3, H, hd)
    x[:, :, 0, :, 0] = 16.0
    x[:, S - 1 if key is None else key, 1, :, 0] = 128.0
    return x.reshape(B, S, 3 * H * hd).to(torch.bfloat16)


def big_logits_qkv(B, S, H, hd=64):
    """Entries of +-16: logits 2048 - 64 f with f sign flips in the key.  f falls by one per 64-key tile, so the
    running maximum moves in every tile, and differs by one between odd and even keys."""
    sign = torch.where(torch.arange(hd) % 3 == 0, -1.0, 1.0)
    x = torch.zeros(B, S, 3, H, hd)
    x[:, :, 0] = 16.0 * sign
    for k in range(S):
        f = (S - 1 - k) // 64 + (k & 1)
        kk = 16.0 * sign.clone()
        kk[:f] = -kk[:f]
        x[:, k, 1] = kk
    return x.reshape(B, S, 3 * H * hd).to(torch.bfloat16)
