"""Plain-loop reference of the evaluation report (ops/eval_report.py, csrc/eval_report.hip): the row
definition and the accumulation written with Python floats and ints, row by row and word by word, sharing
no code with the torch composition.  Used by tests/test_eval_report.py and tests/test_eval_report_gpu.py.

State layout (written out here on its own): rows, nonfinite, padded, bins [n_bins][count, hit1, sum q],
count [L], hit1 [L], hit5 [L], predicted [L], confusion [L][L] while L <= 4096."""

import math

import numpy as np
import torch

MATRIX_MAX_L = 4096


def rows_ref(logits, labels, mode):
    """(pred, rank, conf64, conf32) lists; ``logits`` [B, L] any float dtype (widened exactly), labels ints.
    Padded and non-finite rows: -1, -1, 0.0."""
    z = logits.double().numpy()
    B, L = z.shape
    pred, rank, c64, c32 = [], [], [], []
    for r in range(B):
        y = int(labels[r])
        row = [float(x) for x in z[r]]
        bad = y == -1 or any(math.isnan(x) for x in row)
        if not bad:
            m = max(row)
            bad = math.isinf(m)
        if bad:
            pred.append(-1), rank.append(-1), c64.append(0.0), c32.append(np.float32(0.0))
            continue
        a = min(max(y, 0), L - 1)
        p = 0
        for c in range(1, L):
            if row[c] > row[p]:
                p = c
        rk = 0
        for c in range(L):
            if row[c] > row[a] or (row[c] == row[a] and c < a):
                rk += 1
        if mode == "ce":
            conf = 1.0 / math.fsum(math.exp(x - m) for x in row)
        else:
            x = row[p]
            conf = 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))
        pred.append(p), rank.append(rk), c64.append(conf), c32.append(np.float32(conf))
    return pred, rank, c64, c32


def q_and_bin(conf32, n_bins):
    c = float(conf32)  # exact widening
    if not 0.0 <= c <= 1.0:
        c = 0.0
    return int(round(c * 4294967296.0)), min(n_bins - 1, int(math.floor(c * n_bins)))  # round: half to even


def words(L, n_bins):
    return 3 + 3 * n_bins + 4 * L + (L * L if L <= MATRIX_MAX_L else 0)


def accumulate_ref(state, labels, pred, rank, conf32, L, n_bins):
    """``state`` (a list of Python ints, or a numpy int64 array for large L) += the batch."""
    o_bins, o_cnt = 3, 3 + 3 * n_bins
    o_h1, o_h5, o_pr, o_cm = o_cnt + L, o_cnt + 2 * L, o_cnt + 3 * L, o_cnt + 4 * L
    for y, p, rk, c in zip(labels, pred, rank, conf32):
        y, p, rk = int(y), int(p), int(rk)
        if y == -1:
            state[2] += 1
            continue
        if not 0 <= p < L:
            state[1] += 1
            continue
        a = min(max(y, 0), L - 1)
        q, b = q_and_bin(c, n_bins)
        h1, h5 = int(rk == 0), int(0 <= rk < min(5, L))
        state[0] += 1
        state[o_bins + 3 * b] += 1
        state[o_bins + 3 * b + 1] += h1
        state[o_bins + 3 * b + 2] += q
        state[o_cnt + a] += 1
        state[o_h1 + a] += h1
        state[o_h5 + a] += h5
        state[o_pr + p] += 1
        if L <= MATRIX_MAX_L:
            state[o_cm + a * L + p] += 1
    return state


def zero_state(L, n_bins):
    return np.zeros(words(L, n_bins), dtype=np.int64)


def structured_rows(L, dtype):
    """(logits [R, L] rounded to ``dtype``, labels int64 [R], names): +-60 logits, all-equal rows, the
    maximum tied between class 2 and the last class, the label's logit tied with four others below and
    above its index with and without one larger class (rank 0, 4, 1, 5), a -inf element, an all -inf row,
    a NaN row, a +inf row, label -1 and label L."""
    g = torch.Generator().manual_seed(77 + L)
    rows, labels, names = [], [], []

    def add(z, y, name):
        rows.append(z.clone()), labels.append(int(y)), names.append(name)

    def rnd():
        return (4.0 * torch.randn(L, generator=g)).clamp(max=8.0)

    a = int(torch.randint(0, L, (1,), generator=g))
    z = torch.full((L,), -60.0)
    z[a] = 60.0
    add(z, a, "+60 on the label")
    add(-z, a, "-60 on the label")
    add(z, (a + 1) % L, "+60 on another class")
    add(torch.full((L,), 1.5), a, "all equal")
    add(torch.full((L,), -2.25), L - 1, "all equal, last label")
    if L > 3:
        z = rnd()
        z[2] = z[L - 1] = 9.0
        add(z, L - 1, "max tied 2 / last, label last")
        add(z, 2, "max tied 2 / last, label 2")
    if L >= 8:
        pos = sorted(torch.randperm(L, generator=g)[:6].tolist())
        big, tied = pos[3], pos[:3] + pos[4:]
        for larger in (False, True):
            z = rnd()
            z[tied] = 9.0
            z[big] = 10.0 if larger else -1.0
            add(z, tied[0], f"label lowest of five tied, larger={larger}")
            add(z, tied[-1], f"label highest of five tied, larger={larger}")
            add(z, tied[2], f"label middle of five tied, larger={larger}")
    z = rnd()
    z[L // 2] = float("-inf")
    add(z, a, "-inf element")
    if L > 1:
        add(z, L // 2, "-inf element on the label")
    add(torch.full((L,), float("-inf")), a, "all -inf")
    z = rnd()
    z[L - 1] = float("nan")
    add(z, a, "NaN row")
    z = rnd()
    z[0] = float("inf")
    add(z, a, "+inf row")
    add(rnd(), -1, "padded")
    add(rnd(), L, "label L")
    add(rnd(), -7, "label -7")
    for _ in range(3):
        add(rnd(), int(torch.randint(0, L, (1,), generator=g)), "random")
    return torch.stack(rows).to(dtype), torch.tensor(labels, dtype=torch.int64), names
