"""References for the fused classification loss (csrc/loss.hip, ops/functional.py cls_loss).

Used by tests/test_cls_loss_gpu.py and kept honest without a GPU by tests/test_cls_loss.py.

The semantics are the torch composition of models/classifier.py / utils/mixup.py.  The dense targets
are part of the model's definition in fp32 (a scattered one-hot, ``smooth_labels``, ``Mixup.mix_labels``
-- the kernel reproduces those fp32 values operation by operation, because which classes tie for the
row maximum decides the label set), so they are built by that fp32 code and are an *input* of the
oracle like the already rounded logits.  Everything downstream of them -- criterion, its gradient,
the label set and the ranking -- is the same composition evaluated in fp64.
"""

import torch
import torch.nn.functional as F

from jumbo_mae_tpu_amd.models.classifier import CRITERION_COLLECTION, FinetuneModel
from jumbo_mae_tpu_amd.utils.mixup import Mixup, smooth_labels


def targets32(labels, L, smoothing=0.0, plan=None):
    """fp32 dense targets [B, L] exactly as FinetuneModel builds them (``_prep_labels`` -> smooth -> mix)."""
    idx = labels.long().clamp(0, L - 1).view(-1, 1)
    t = torch.zeros(labels.shape[0], L, device=labels.device).scatter_(1, idx, 1.0)
    return Mixup.mix_labels(smooth_labels(t, smoothing), plan)


def rank(z, c):
    """The kernel's rank of class ``c`` in the 1-D logits ``z``: strictly larger values, plus equal
    values at a lower index (the lower index wins a tie)."""
    return int((z > z[c]).sum() + (z[:c] == z[c]).sum())


def hits_stable(logits, t):
    """(top-1, top-5) membership of the arg-max label set under a stable descending sort."""
    lab = t == t.max(-1, keepdim=True).values
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices
    k = min(5, logits.shape[-1])
    got = torch.gather(lab, 1, order[:, :k])
    return got[:, 0], got.any(-1)


def composition(logits, t, criterion, dloss, dtype):
    """(loss [B], dlogits [B, L]) of the torch composition evaluated in ``dtype`` (fp64: the oracle;
    fp32: the parent's path, whose error against the oracle sets the kernels' bound)."""
    z = logits.to(dtype).detach().requires_grad_(True)
    loss = CRITERION_COLLECTION[criterion](z, t.to(dtype))
    (dz,) = torch.autograd.grad(loss, z, dloss.to(dtype))
    return loss.detach(), dz


def bce_stable64(logits, t):
    """sigmoid_bce in fp64 without its cancellation: softplus(z) - t z is softplus(-z) for a target
    and softplus(z) otherwise.  binary_cross_entropy_with_logits forms (1 - t) z - log_sigmoid(z),
    which at z = -60 leaves 0 or 7e-15 where the value is 8.7e-27 -- in fp64 too."""
    z = logits.double()
    return F.softplus(torch.where(t > 0, -z, z)).mean(-1)


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


def cpu_plan(B, w, perm):
    """A Mixup plan as ``Mixup.plan`` returns it on the CPU, from an explicit weight and permutation."""
    return {"mode": "mixup", "ratio": w, "box": None, "label_w": w, "perm": torch.as_tensor(perm, dtype=torch.long),
            "label_w_t": w}


def device_plan(B, w, perm, device):
    """The same with the static device buffers of a GPU plan (``dev``: params [mode, ratio, label_w],
    perm int32): the label weight is an fp32 device scalar there, as in the train step."""
    params = torch.tensor([1.0, w, w], dtype=torch.float32, device=device)
    p32 = torch.as_tensor(perm, dtype=torch.int32).to(device)
    return {"mode": "mixup", "ratio": w, "box": None, "label_w": w, "perm": p32, "label_w_t": params[2],
            "dev": {"params": params, "perm": p32}}


def plan_to_cpu(plan):
    """A device plan for the CPU composition: the SAME fp32 weight, as a 0-dim fp32 tensor (a Python
    float would make ``1 - w`` a double subtraction, which the device path never does)."""
    if plan is None:
        return None
    q = dict(plan)
    q.pop("dev", None)
    q["perm"] = plan["perm"].cpu().long()
    q["label_w_t"] = plan["label_w_t"].detach().cpu()
    return q


def structured_rows(L, dtype, gen):
    """Rows that probe the edges: (logits [R, L] already rounded to ``dtype``, labels [R], names).
    +-60 logits (overflow), all-equal logits and -- for L >= 8 -- the label class at rank 0, 4 and 5
    among distinct values and tied with the rank-4 value at a lower / a higher index.  The names of
    the +-60 rows start with "+60" / "-60"."""
    rows, labels, names = [], [], []

    def add(z, a, name):
        rows.append(z)
        labels.append(a)
        names.append(name)

    a = int(torch.randint(0, L, (1,), generator=gen))
    z = torch.full((L,), -60.0)
    z[a] = 60.0
    add(z, a, "+60 on the label")
    z = torch.full((L,), 60.0)
    z[a] = -60.0
    add(z, a, "-60 on the label")
    if L > 1:
        z = torch.full((L,), -60.0)
        z[(a + 1) % L] = 60.0
        add(z, a, "+60 on another class")
    add(torch.full((L,), 1.5), a, "all equal")
    add(torch.full((L,), 1.5), L - 1, "all equal, last class")
    if L >= 8:
        tops = torch.tensor([10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0])
        for r in (0, 4, 5):
            pos = torch.randperm(L, generator=gen)[:8]
            z = -3.0 * torch.rand(L, generator=gen)
            z[pos] = tops
            add(z, int(pos[r]), f"rank {r}")
        for lower in (True, False):
            pos = torch.randperm(L, generator=gen)[:8]
            z = -3.0 * torch.rand(L, generator=gen)
            z[pos] = tops
            z[pos[5]] = tops[4]  # two classes hold the rank-4 value
            i, j = sorted((int(pos[4]), int(pos[5])))
            add(z, i if lower else j, "tie at rank 4, " + ("lower" if lower else "higher") + " index")
    return torch.stack(rows).to(dtype), torch.tensor(labels), names


def distinct_top6_rows(B, L, dtype, gen):
    """4 randn rows (rounded to ``dtype``) whose six largest values are distinct: six random classes are
    raised to 20 .. 15, everything else stays below 15.  The caller verifies it."""
    z = (4.0 * torch.randn(B, L, generator=gen)).clamp(max=14.0)
    k = min(6, L)
    for b in range(B):
        pos = torch.randperm(L, generator=gen)[:k]
        z[b, pos] = torch.arange(20.0, 20.0 - k, -1.0)
    return z.to(dtype)
