"""References for the fused distillation loss (csrc/distill.hip, ops/functional.py kd_loss).

Used by tests/test_distill_gpu.py and kept honest without a GPU by tests/test_distill.py.

The oracle is the definition written out with ``log_softmax`` in fp64 on the already rounded logits:
  soft  kd = T^2 sum_c q_c (log q_c - log p_c), q = softmax(u / T), p = softmax(z / T), d kd / d z = T (p - q);
  hard  kd = -log softmax(z)_t, t = the teacher's arg-max, d kd / d z = softmax(z) - onehot(t);
every arg-max is the lowest index among ties (taken from a stable descending sort here, not from
``argmax``).  ``soft_split64`` is the same soft value in a second algebraic form, sum_c q_c (u_c - z_c) / T
- (lse(u / T) - lse(z / T)): tests/test_distill.py compares the two on the structured rows to show that
the oracle does not cancel there.
"""

import torch

from cls_loss_ref import bf16_steps, structured_rows, ulp32  # noqa: F401  (re-exported)

from jumbo_mae_tpu_amd.ops import functional as Fn


def argmax_first(x):
    """Lowest index of the row maximum, by a stable descending sort."""
    return torch.sort(x, dim=-1, descending=True, stable=True).indices[..., 0]


def closed_form(z, u, T, mode, dtype=torch.float64):
    """(kd [B], d kd / d z [B, L], t [B], agree [B]) of the definition evaluated in ``dtype``."""
    z, u = z.to(dtype), u.to(dtype)
    t = argmax_first(u)
    agree = argmax_first(z) == t
    if mode == "soft":
        lq, lp = torch.log_softmax(u / T, -1), torch.log_softmax(z / T, -1)
        return (T * T) * (lq.exp() * (lq - lp)).sum(-1), T * (lp.exp() - lq.exp()), t, agree
    lp = torch.log_softmax(z, -1)
    onehot = torch.zeros_like(lp).scatter_(1, t.view(-1, 1), 1.0)
    return -lp.gather(1, t.view(-1, 1)).squeeze(1), lp.exp() - onehot, t, agree


def oracle(z, u, T, mode, dloss):
    """fp64: (kd, dloss-weighted dz, t, agree)."""
    kd, dz, t, agree = closed_form(z, u, T, mode)
    return kd, dz * dloss.double().unsqueeze(-1), t, agree


def composition32(z, u, T, mode, dloss):
    """(kd, dz) of the fp32 torch composition ``kd_loss_torch`` on the same input: the path the kernels
    replace, whose error against the oracle sets their bound."""
    z32 = z.float().detach().requires_grad_(True)
    kd, _ = Fn.kd_loss_torch(z32, u.float(), T, mode)
    (dz,) = torch.autograd.grad(kd, z32, dloss.float())
    return kd.detach(), dz


def soft_split64(z, u, T):
    """The soft kd in fp64 as sum_c q_c (u_c - z_c) / T - (lse(u / T) - lse(z / T))."""
    a, b = z.double() / T, u.double() / T
    q = torch.softmax(b, -1)
    return (T * T) * ((q * (b - a)).sum(-1) - (torch.logsumexp(b, -1) - torch.logsumexp(a, -1)))


def bound(v32, v64):
    """max(2 x the fp32 composition's error, 1 fp32 ulp of the fp64 value)."""
    return torch.maximum(2.0 * (v32.double() - v64).abs(), ulp32(v64))


def pair_rows(L, dtype):
    """(z [R, L], u [R, L], names) already rounded to ``dtype``: ``structured_rows`` for both operands,
    then u == z on a random row, an all-equal teacher row, the teacher's maximum tied between class 2
    and the last class (L > 3), and a +-60 row against itself.

    The teacher gets the student's rows some places further on: by one for L < 8 (the +-60 and all-equal
    rows meet each other), by five for L >= 8, so that the five ranked / tied rows meet the five +-60 /
    all-equal rows both ways round, and the ranked rows meet each other with the teacher's halved.  What
    is avoided is a ranked row against an unscaled ranked row: at L = 8 those are permutations of one
    set of values, so wherever the two hold the same value at the same class the gradient T (p - q) is
    exactly 0 by symmetry and EVERY floating-point evaluation, the fp64 oracle included, returns the
    rounding noise of its own summation order there -- a comparison in bf16 steps has no meaning on such
    an element (random rows against each other are tests/test_distill_gpu.py::test_random_logits)."""
    gen = torch.Generator().manual_seed(L)
    rows, _, names = structured_rows(L, dtype, torch.Generator().manual_seed(L))
    k = 5 if len(names) == 10 else 1
    assert len(names) == 10 or L < 8
    z, u = rows.float(), torch.roll(rows.float(), k, 0)
    names = [f"{a} | {b}" for a, b in zip(names, names[-k:] + names[:-k])]
    extra_z, extra_u = [], []

    def add(a, b, name):
        extra_z.append(a)
        extra_u.append(b)
        names.append(name)

    r = (4.0 * torch.randn(L, generator=gen)).to(dtype).float()
    add(r, r.clone(), "u == z")
    add((4.0 * torch.randn(L, generator=gen)), torch.full((L,), 0.5), "all-equal teacher")
    if L > 3:
        t = (4.0 * torch.randn(L, generator=gen)).clamp(max=5.0)
        t[2] = t[L - 1] = 9.0
        add(4.0 * torch.randn(L, generator=gen), t, "teacher tie 2 / last")
    add(z[0].clone(), z[0].clone(), "u == z, +60 on the label")
    if k == 5:
        for i in range(5, 10):
            add(z[i].clone(), 0.5 * z[5 + (i - 4) % 5], "ranked | ranked, halved")
    z = torch.cat([z, torch.stack(extra_z)]).to(dtype)
    u = torch.cat([u, torch.stack(extra_u)]).to(dtype)
    return z, u, names
