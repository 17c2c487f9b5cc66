"""Exact reference of the norm monitor's per-segment statistics (optim/monitor.py, csrc/optim.hip
``seg_stats_kernel``) on the hand-built chunk tables of tests/optim_ref.py.

For every segment, over the elements the table covers (``Table.seg_of``):

  G2*, P2*, D2*   ``math.fsum`` -- the correctly rounded sum -- of the float64 terms g^2, p^2 and
                  (p - p_old)^2, each fp32 value widened first; g^2 and p^2 are exact in float64 (24-bit
                  significands), the difference rounds once and its square once;
  GMAX            the exact maximum of |g|;  GBAD, PBAD, N   integer counts.

A non-finite value is counted and contributes to no sum (D2 needs p and p_old finite); a frozen segment
(``meta[seg][3] == 0``) reports P2, PBAD and N only.  ``terms`` holds the number of terms of each sum, the
``n`` of the bounds:

  |G2 - G2*| <= n 2^-53 G2*  (same for P2): non-negative exact terms summed in ANY order, one rounding
  per addition (n - 1 of them, each relative to a partial sum <= the total) plus the reference's own;
  |D2 - D2*| <= (n + 4) 2^-53 D2*: the difference is the same float64 number on both sides, its square
  is rounded here and may not be in a contracted FMA.
"""

from __future__ import annotations

import math

import torch

import optim_ref as R

COLS = ("G2", "P2", "D2", "GMAX", "GBAD", "PBAD", "N")
U53 = 2.0 ** -53


def tables(chunk: int) -> dict:
    full = R.runs64()
    return {"runs64": full, "partial": R.partial(full), "prod": R.prod(chunk)}


def ref_stats(tab: R.Table, meta, p, g, p_old=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(stats float64 [nseg, 7], terms int64 [nseg, 3]) from fp32 CPU inputs."""
    out = torch.zeros(tab.nseg, 7, dtype=torch.float64)
    terms = torch.zeros(tab.nseg, 3, dtype=torch.int64)
    P, G = p.detach().cpu().to(torch.float64), g.detach().cpu().to(torch.float64)
    O = p_old.detach().cpu().to(torch.float64) if p_old is not None else None
    for k in range(tab.nseg):
        idx = torch.nonzero(tab.seg_of == k).flatten()
        if idx.numel() == 0:
            continue
        live = float(meta[k, 3]) != 0.0
        pv = P[idx].tolist()
        pfin = [math.isfinite(x) for x in pv]
        p2 = [x * x for x, f in zip(pv, pfin) if f]
        out[k, 1], terms[k, 1] = math.fsum(p2), len(p2)
        out[k, 5] = len(pv) - len(p2)
        out[k, 6] = len(pv)
        if not live:
            continue
        gv = G[idx].tolist()
        g2 = [x * x for x in gv if math.isfinite(x)]
        out[k, 0], terms[k, 0] = math.fsum(g2), len(g2)
        out[k, 3] = max((abs(x) for x in gv if math.isfinite(x)), default=0.0)
        out[k, 4] = len(gv) - len(g2)
        if O is not None:
            d2 = [(x - y) * (x - y) for x, y, f in zip(pv, O[idx].tolist(), pfin) if f and math.isfinite(y)]
            out[k, 2], terms[k, 2] = math.fsum(d2), len(d2)
    return out, terms


def assert_stats(got, ref, terms, tag: str = "", exact_sums: bool = False) -> None:
    """``got`` against ``ref_stats``: columns 3..6 equal, the sums within the derived bounds (or, with
    ``exact_sums``, bit for bit).  Every figure of a failing row is in the message."""
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    for k in range(ref.shape[0]):
        row, want = got[k].tolist(), ref[k].tolist()
        assert row[3:] == want[3:], f"{tag} seg {k}: {dict(zip(COLS[3:], row[3:]))} != {dict(zip(COLS[3:], want[3:]))}"
        for c in range(3):
            n = int(terms[k, c])
            bound = 0.0 if exact_sums else (n + (4 if c == 2 else 0)) * U53 * want[c]
            err = abs(row[c] - want[c])
            assert err <= bound, (f"{tag} seg {k} {COLS[c]}: got {row[c]!r}, reference {want[c]!r}, "
                                  f"|err| {err:.3e} > bound {bound:.3e} (n = {n})")
