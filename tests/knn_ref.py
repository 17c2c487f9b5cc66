"""Inputs and brute-force references shared by tests/test_knn.py and tests/test_knn_gpu.py."""

import math

import numpy as np
import torch


def exact_inputs(Nq, Nb, D, seed, q_from_bank=True):
    """bf16 q [Nq, D], bank [Nb, D] with entries from {-1, -0.5, 0, 0.5, 1} * 2^-3: every product is a
    multiple of 2^-8 of magnitude <= 2^-6, so a dot product over D <= 2^16 terms is exact in fp32 in
    any summation order.  Several bank rows are duplicates of others (ties between different
    indices) and some queries equal bank rows."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
    bank = vals[torch.randint(0, 5, (Nb, D), generator=g)]
    q = vals[torch.randint(0, 5, (Nq, D), generator=g)]
    for i in range(0, Nb // 3):  # row 3 i + 1 copies row i (never itself: 3 i + 1 > i)
        if 3 * i + 1 < Nb:
            bank[3 * i + 1] = bank[i]
    if Nb > 7:
        bank[Nb - 1] = bank[Nb - 7]  # a duplicate pair in the last tile / slice
    if q_from_bank:
        for i in range(0, Nq, 4):
            q[i] = bank[(5 * i) % Nb]
    return q.to(torch.bfloat16), bank.to(torch.bfloat16)


def brute_topk(q, bank, k, self_idx=None):
    """Python loop: (idx int32 [Nq, k], sim fp64 [Nq, k]) ordered by (sim descending, index ascending)."""
    qd, bd = q.double().numpy(), bank.double().numpy()
    Nq, Nb = qd.shape[0], bd.shape[0]
    idx = np.full((Nq, k), -1, dtype=np.int32)
    sim = np.full((Nq, k), -np.inf)
    for r in range(Nq):
        s = bd @ qd[r]
        skip = -1 if self_idx is None else int(self_idx[r])
        order = sorted((j for j in range(Nb) if j != skip), key=lambda j: (-s[j], j))[:k]
        idx[r, :len(order)] = order
        sim[r, :len(order)] = s[order]
    return torch.from_numpy(idx), torch.from_numpy(sim)


def brute_vote(idx, sim, bank_labels, labels, T):
    """Python loop of the weighted vote: (pred int32 [Nq, 5], hit1, hit5 bool [Nq])."""
    Nq, k = idx.shape
    pred = torch.full((Nq, 5), -1, dtype=torch.int32)
    hit1 = torch.zeros(Nq, dtype=torch.bool)
    hit5 = torch.zeros(Nq, dtype=torch.bool)
    for r in range(Nq):
        score = {}
        s0 = float(sim[r, 0])
        for j in range(k):
            i = int(idx[r, j])
            if i < 0:
                continue
            c = int(bank_labels[i])
            score[c] = score.get(c, 0.0) + math.exp((float(sim[r, j]) - s0) / T)
        ranked = sorted(score, key=lambda c: (-score[c], c))[:5]
        for n, c in enumerate(ranked):
            pred[r, n] = c
        y = int(labels[r])
        hit1[r] = y >= 0 and len(ranked) > 0 and ranked[0] == y
        hit5[r] = y >= 0 and y in ranked
    return pred, hit1, hit5


def vote_inputs(Nq, k, classes, Nb=400, seed=0):
    """Hand-built lists for the vote: sims from a coarse grid (so that equal class scores come from
    identical terms), -1 slots in the tail of some rows and in the middle of others, fewer than five
    distinct classes in some rows, rows whose two leading classes tie by construction, labels of -1."""
    g = torch.Generator().manual_seed(seed)
    bank_labels = torch.randint(0, classes, (Nb,), generator=g, dtype=torch.int32)
    bank_labels[:4] = torch.tensor([3, 1, 3, 1], dtype=torch.int32)[:4] % classes  # rows 0..3: classes 3, 1, 3, 1
    idx = torch.randint(0, Nb, (Nq, k), generator=g, dtype=torch.int32)
    sim = (torch.randint(0, 9, (Nq, k), generator=g).float() / 16).sort(1, descending=True).values
    labels = torch.randint(0, classes, (Nq,), generator=g, dtype=torch.int32)
    for r in range(Nq):
        if r % 5 == 1 and k >= 4:  # classes 3 and 1 tie exactly: sims (a, a, b, b) on bank rows 0, 1, 2, 3
            idx[r] = -1
            idx[r, :4] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
            sim[r, :4] = torch.tensor([0.5, 0.5, 0.25, 0.25])
            labels[r] = 3 if r % 2 else 1
        elif r % 5 == 2:  # a tail of empty slots
            idx[r, max(1, k // 2):] = -1
            sim[r, max(1, k // 2):] = float("-inf")
        elif r % 5 == 3 and k >= 3:  # an empty slot in the middle
            idx[r, 1] = -1
        elif r % 5 == 4:  # at most two distinct classes
            idx[r] = idx[r] % 2
        if r % 7 == 0:
            labels[r] = -1
    if k >= 1:
        idx[Nq - 1] = -1  # no neighbour at all
        sim[Nq - 1] = float("-inf")
    return idx, sim, bank_labels, labels
