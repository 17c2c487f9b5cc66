"""References for the fused BatchNorm kernels (csrc/batchnorm.hip, parallel/syncbn.py).

Used by tests/test_batchnorm_gpu.py and kept honest without a GPU by tests/test_batchnorm.py.

``composition`` is the torch composition of parallel/syncbn.py at world size 1, operation by
operation and in its order, evaluated in fp64 (the oracle) or in fp32 (the path the kernels replace,
whose error against the oracle sets the kernels' bound).
"""

import torch


def composition(x, gamma, beta, dy, dtype, eps=1e-5, **given):
    """(y, mean, var, dgamma, dbeta, dx) of training-mode BatchNorm and its backward, evaluated in ``dtype``
    (``passes`` with its first six results)."""
    return passes(x, gamma, beta, dy, dtype, eps, **given)[:6]


def passes(x, gamma, beta, dy, dtype, eps=1e-5, packed=None, stats=None, packed_g=None):
    """(y, mean, var, dgamma, dbeta, dx, packed, rstd, packed_g) of training-mode BatchNorm over the rows of ``x`` [B, J] and
    its backward for the upstream gradient ``dy``, evaluated in ``dtype``.

    ``packed`` ([2 J]: mean, mean of squares), ``stats`` ([2, J]: mean, rstd) and ``packed_g`` ([2 J]) are
    the fp32 tensors that travel between the passes (and through the all-reduces).  Given one of them,
    the composition goes on from it instead of from its own value: the pass that reads it -- the
    normalisation, the backward reductions, dx -- is then evaluated on exactly the inputs a kernel
    of csrc/batchnorm.hip reads."""
    x, gamma, beta, dy = (t.to(dtype) for t in (x, gamma, beta, dy))
    n = x.shape[0]
    own = torch.cat([x.sum(0), (x * x).sum(0)]) / n
    mean, mean2 = (own if packed is None else packed.to(dtype)).chunk(2)
    var = torch.clamp(mean2 - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat * gamma + beta
    if stats is not None:
        mean, rstd = stats.to(dtype)
        xhat = (x - mean) * rstd
    dgamma = (dy * xhat).sum(0)
    dbeta = dy.sum(0)
    g = dy * gamma
    own_g = torch.cat([g.sum(0), (g * xhat).sum(0)])
    sg, sgx = (own_g if packed_g is None else packed_g.to(dtype)).chunk(2)
    dx = rstd * (g - sg / n - xhat * sgx / n)
    return y, mean, var, dgamma, dbeta, dx, own, rstd, own_g


def running(ra, stat, momentum=0.99):
    """One step of the running-statistics recurrence of ``_update_running``, in the dtype of ``ra``."""
    return ra * momentum + (1 - momentum) * stat.to(ra.dtype)


def eval_formula(x, gamma, beta, running_mean, running_var, dtype, eps=1e-5):
    """The inference branch of ``sync_batch_norm`` evaluated in ``dtype``."""
    x, gamma, beta, rm, rv = (t.to(dtype) for t in (x, gamma, beta, running_mean, running_var))
    return (x - rm) * torch.rsqrt(rv + eps) * gamma + beta


def ulp32(x):
    """Spacing of fp32 at |x| (x fp64), as fp64."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def bf16_steps(a, b):
    """|a - b| in bf16 steps (a, b bf16 tensors; +0 and -0 coincide)."""
    def key(v):
        bits = v.view(torch.int16).int()
        mag = bits & 0x7FFF
        return torch.where(bits < 0, -mag, mag)
    return (key(a) - key(b)).abs()


def bound(v32, v64):
    """The kernels' per-element bound: max(2 x the fp32 composition's own error, 1 fp32 ulp of the value)."""
    return torch.maximum(2.0 * (v32.double() - v64).abs(), ulp32(v64))


def inputs(B, J, gen):
    """Unit-scale inputs: x = randn * U(0.5, 1.5) + randn per column, gamma = 1 + 0.5 randn, beta = randn,
    dy = randn / B rounded to bf16 (so that the same values serve a bf16 and an fp32 upstream gradient)."""
    std = 0.5 + torch.rand(J, generator=gen)
    x = torch.randn(B, J, generator=gen) * std + torch.randn(J, generator=gen)
    gamma = 1.0 + 0.5 * torch.randn(J, generator=gen)
    beta = torch.randn(J, generator=gen)
    dy = (torch.randn(B, J, generator=gen) / B).to(torch.bfloat16).float()
    return x, gamma, beta, dy
