"""ops/functional.py cls_loss on the CPU (the torch composition, which is also the mirror the GPU
tests use) and the references of tests/cls_loss_ref.py, without a GPU."""

import pytest
import torch

import cls_loss_ref as R
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel, sigmoid_bce, softmax_cross_entropy
from jumbo_mae_tpu_amd.ops import functional as Fn
from jumbo_mae_tpu_amd.utils.mixup import Mixup


@pytest.mark.parametrize("criterion, smoothing", [("ce", 0.0), ("ce", 0.1), ("bce", 0.0)])
@pytest.mark.parametrize("w", [None, 0.3, 0.5, 1.0])
def test_cpu_equals_explicit_targets(criterion, smoothing, w):
    """cls_loss on integer labels == the criterion on targets written out by hand: one-hot,
    (1 - a) t + a / L, w t + (1 - w) t[perm]."""
    g = torch.Generator().manual_seed(5)
    B, L = 7, 13
    logits = 4.0 * torch.randn(B, L, generator=g)
    labels = torch.randint(0, L, (B,), generator=g)
    perm = torch.tensor([3, 1, 0, 6, 5, 4, 2])  # fixed point at 1
    plan = None if w is None else R.cpu_plan(B, w, perm)
    t = torch.zeros(B, L)
    t[torch.arange(B), labels] = 1.0
    if smoothing:
        t = (1.0 - smoothing) * t + smoothing / L
    if w is not None:
        t = w * t + (1 - w) * t[perm]
    want = (softmax_cross_entropy if criterion == "ce" else sigmoid_bce)(logits, t)
    a1, a5 = FinetuneModel.accuracy(logits, t)
    loss, acc1, acc5 = Fn.cls_loss(logits, labels, plan, smoothing, criterion)
    assert torch.equal(loss, want)
    assert torch.equal(acc1, a1) and torch.equal(acc5, a5)
    assert torch.equal(R.targets32(labels, L, smoothing, plan), t)
    if w == 0.5:  # both classes of a mixed row are in the label set
        lab = t == t.max(-1, keepdim=True).values
        mixed = labels != labels[perm]
        assert mixed.any() and (lab.sum(-1)[mixed] == 2).all() and (lab.sum(-1)[~mixed] == 1).all()


def test_cpu_path_has_a_gradient_and_clamps_labels():
    logits = torch.randn(3, 5, requires_grad=True)
    loss, acc1, acc5 = Fn.cls_loss(logits, torch.tensor([-2, 9, 1]), None, 0.1, "ce")
    want, _, _ = Fn.cls_loss(logits, torch.tensor([0, 4, 1]), None, 0.1, "ce")
    assert torch.equal(loss, want)
    loss.sum().backward()
    assert logits.grad is not None and logits.grad.abs().sum() > 0
    assert acc1.dtype == torch.bool and acc5.dtype == torch.bool and not acc1.requires_grad


def test_rank_rule_is_the_stable_sort():
    """rank(c) = #{z_j > z_c} + #{j < c: z_j == z_c} is c's position under
    torch.sort(stable=True, descending=True), ties included."""
    g = torch.Generator().manual_seed(0)
    for L in (1, 3, 8, 40):
        for _ in range(20):
            z = torch.randint(-2, 3, (L,), generator=g).float()  # few distinct values: many ties
            order = torch.sort(z, descending=True, stable=True).indices.tolist()
            for c in range(L):
                assert R.rank(z, c) == order.index(c)


def test_hits_stable_matches_topk_on_distinct_values():
    g = torch.Generator().manual_seed(1)
    for L in (1, 3, 8, 1000):
        z = R.distinct_top6_rows(6, L, torch.bfloat16, g).float()
        top = z.sort(-1, descending=True).values[:, :6]
        assert (top[:, :-1] > top[:, 1:]).all()
        labels = torch.randint(0, L, (6,), generator=g)
        t = R.targets32(labels, L, 0.1, R.cpu_plan(6, 0.5, torch.tensor([1, 2, 3, 4, 5, 0])))
        a1, a5 = FinetuneModel.accuracy(z, t)
        h1, h5 = R.hits_stable(z, t)
        assert torch.equal(a1, h1) and torch.equal(a5, h5)


def test_structured_rows_are_what_they_say():
    g = torch.Generator().manual_seed(2)
    for dtype in (torch.bfloat16, torch.float32):
        z, labels, names = R.structured_rows(1003, dtype, g)
        z = z.float()
        for row, a, name in zip(z, labels.tolist(), names):
            if name.startswith("rank"):
                assert R.rank(row, a) == int(name.split()[1]), name
            if name.startswith("tie"):
                assert R.rank(row, a) == (4 if "lower" in name else 5), name
                assert (row == row[a]).sum() == 2
            if name.startswith("all equal"):
                assert R.rank(row, a) == a


@pytest.mark.parametrize("criterion", ["ce", "bce"])
def test_finetune_forward_cpu_is_the_composition(criterion):
    """FinetuneModel.forward on the CPU: bit for bit the composition it has always been -- one-hot,
    smoothing, the head's fp32 logits with the plan's mixed labels, criterion mean, accuracies."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.utils.mixup import smooth_labels

    vc = ViTConfig(layers=2, dim=64, heads=2, labels=10, image_size=32, patch_size=16, posemb="learnable")
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (6, 3, 32, 32), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (6,), generator=g)
    m = FinetuneModel(vc, Mixup(0.8, 1.0, seed=3), label_smoothing=0.1, criterion=criterion).to("cpu", torch.float32, seed=0)
    out = m(imgs, labels)
    # the same model and Mixup stream again, the loss written out
    m2 = FinetuneModel(vc, Mixup(0.8, 1.0, seed=3), label_smoothing=0.1, criterion=criterion).to("cpu", torch.float32, seed=0)
    t = torch.zeros(6, 10).scatter_(1, labels.view(-1, 1), 1.0)
    t = smooth_labels(t, 0.1 if criterion == "ce" else 0.0)
    logits, t = m2.logits(imgs, t, None, False)
    assert logits.dtype == torch.float32
    want = (softmax_cross_entropy if criterion == "ce" else sigmoid_bce)(logits, t).mean()
    a1, a5 = FinetuneModel.accuracy(logits, t)
    assert torch.equal(out["loss"], want)
    assert torch.equal(out["acc1"], a1.float().mean()) and torch.equal(out["acc5"], a5.float().mean())
    # evaluate(): -1 labels masked out, no smoothing, no mixing, sums over the valid samples
    ev_labels = torch.where(torch.arange(6) % 3 == 0, torch.full_like(labels, -1), labels)
    ev = m.evaluate(imgs, ev_labels)
    valid = ev_labels != -1
    t = torch.zeros(6, 10).scatter_(1, torch.where(valid, ev_labels, torch.zeros_like(ev_labels)).view(-1, 1), 1.0)
    with torch.no_grad():
        logits, _ = m2.logits(imgs, t, None, True)
        want = (softmax_cross_entropy if criterion == "ce" else sigmoid_bce)(logits, t)
    a1, a5 = FinetuneModel.accuracy(logits, t)
    v = valid.float()
    assert ev["num_samples"].item() == 4
    assert torch.equal(ev["loss"], (want * v).sum())
    assert torch.equal(ev["acc1"], (a1.float() * v).sum()) and torch.equal(ev["acc5"], (a5.float() * v).sum())
