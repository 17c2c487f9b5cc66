"""Plain-loop references shared by tests/test_feat_stats.py and tests/test_feat_stats_gpu.py."""

import math

import torch


def gram_loops(x, valid=None):
    """(G fp64 [D, D], s fp64 [D], n, S fp64 [D, D]) over the valid rows of ``x``: every element the
    ``math.fsum`` (correctly rounded) of the fp64 products; S the same of their absolute values."""
    xd = x.double()
    rows = [r for r in range(x.shape[0]) if valid is None or bool(valid[r])]
    D = x.shape[1]
    cols = [[float(xd[r, d]) for r in rows] for d in range(D)]
    G = torch.zeros(D, D, dtype=torch.float64)
    S = torch.zeros(D, D, dtype=torch.float64)
    s = torch.zeros(D, dtype=torch.float64)
    for i in range(D):
        s[i] = math.fsum(cols[i])
        for j in range(i, D):
            prods = [a * b for a, b in zip(cols[i], cols[j])]  # exact in fp64 for fp32 inputs
            G[i, j] = G[j, i] = math.fsum(prods)
            S[i, j] = S[j, i] = math.fsum(abs(p) for p in prods)
    return G, s, len(rows), S


def uniformity_loops(q, bank, self_idx=None, bank_valid=None, t=2.0):
    """fp64 [Nq]: per query ``math.fsum`` of ``math.exp(-2 t (1 - s))`` over the eligible bank rows, s
    the fp64 dot product."""
    qd, bd = q.double(), bank.double()
    sc = (qd @ bd.t()).tolist()
    out = []
    for i in range(q.shape[0]):
        skip = -1 if self_idx is None else int(self_idx[i])
        out.append(math.fsum(math.exp(-2.0 * t * (1.0 - sc[i][j])) for j in range(bank.shape[0])
                             if j != skip and (bank_valid is None or bool(bank_valid[j]))))
    return torch.tensor(out, dtype=torch.float64)


def exact_rows(n, D, seed):
    """fp32 [n, D] with entries from {-1, -0.5, 0, 0.5, 1} * 2^-3 (tests/knn_ref.py exact_inputs): every
    product is a multiple of 2^-8, so sums of up to 2^40 of them are exact in fp64 in any order."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
    return vals[torch.randint(0, 5, (n, D), generator=g)]
