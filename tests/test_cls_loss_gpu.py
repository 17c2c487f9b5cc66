"""The fused classification loss kernels (csrc/loss.hip) against the torch composition in fp64 on the
CPU (tests/cls_loss_ref.py), fed the same already rounded logits and the model's fp32 targets.

Bounds: ``hit`` equals the oracle exactly; a row's loss (and, on fp32 logits, a gradient element) may
miss the fp64 value by max(2 x the error of the fp32 torch composition on the same input, 1 fp32 ulp
of the value) -- the bound comes from the parent's path, computed here, never from the kernel; on
bf16 logits the gradient is within 1 bf16 step of the fp64 gradient rounded to bf16.

One exception, on the oracle's side and on the +-60 structured rows under BCE only: there
binary_cross_entropy_with_logits cancels in fp64 as well (8.7e-27 comes out as 0 or 7e-15), so those
rows' loss is compared with the same criterion in its non-cancelling fp64 form
(cls_loss_ref.bce_stable64), under the same bound."""

import itertools

import pytest
import torch

import cls_loss_ref as R

pytestmark = pytest.mark.gpu

MODES = [("ce", 0.0), ("ce", 0.1), ("bce", 0.0)]
DTYPES = [torch.bfloat16, torch.float32]


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _plans(B, gen):
    """(name, weight, permutation): none; three weights under a permutation without fixed points (a
    rotation; B == 1 has only the identity); one with fixed points."""
    rot = torch.roll(torch.arange(B), 1)
    fixed = torch.arange(B)
    if B >= 3:
        fixed[[0, B - 1]] = fixed[[B - 1, 0]]  # everything in between stays
    out = [("none", None, None)]
    out += [(f"w={w}", w, rot) for w in (0.3, 0.5, 1.0)]
    out.append(("fixed points", 0.3, fixed))
    return out


def _check(logits, labels, criterion, smoothing, plan, gen, what, pm60=None):
    """One forward + backward of the kernels on ``logits`` (a GPU tensor, maybe a view) against the
    oracle.  ``pm60``: mask of the +-60 rows (see the module docstring)."""
    ext = _ext()
    B, L = logits.shape
    mode = 0 if criterion == "ce" else 1
    perm, w = (None, None) if plan is None else (plan["dev"]["perm"], plan["dev"]["params"][2:3])
    dloss = (0.25 + torch.rand(B, generator=gen)) / B  # non-uniform
    lab_d, dl_d = labels.cuda(), dloss.cuda()
    loss, hit, lse = ext.cls_loss_fwd(logits, lab_d, perm, w, smoothing, mode)
    dz = ext.cls_loss_bwd(dl_d, logits, lab_d, perm, w, smoothing, mode, lse)
    loss2, hit2, lse2 = ext.cls_loss_fwd(logits, lab_d, perm, w, smoothing, mode)
    dz2 = ext.cls_loss_bwd(dl_d, logits, lab_d, perm, w, smoothing, mode, lse2)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(hit, hit2) and torch.equal(lse, lse2), what
    assert torch.equal(dz.view(torch.int16 if dz.dtype == torch.bfloat16 else torch.int32),
                       dz2.view(torch.int16 if dz.dtype == torch.bfloat16 else torch.int32)), what
    assert dz.dtype == logits.dtype and dz.shape == logits.shape and hit.dtype == torch.bool

    z = logits.cpu()
    t = R.targets32(labels, L, smoothing, R.plan_to_cpu(plan))
    l64, d64 = R.composition(z, t, criterion, dloss, torch.float64)
    l32, d32 = R.composition(z, t, criterion, dloss, torch.float32)
    h1, h5 = R.hits_stable(z.double(), t)
    assert torch.equal(hit[:, 0].cpu(), h1) and torch.equal(hit[:, 1].cpu(), h5), what

    if pm60 is not None and criterion == "bce":
        l64 = torch.where(pm60, R.bce_stable64(z, t), l64)
    err = (loss.cpu().double() - l64).abs()
    bound = torch.maximum(2.0 * (l32.double() - l64).abs(), R.ulp32(l64))
    worst = (err / bound).max().item()
    print(f"{what}: loss err / bound {worst:.3f}")
    assert worst <= 1.0, (what, "loss", worst, int((err / bound).argmax()))
    if logits.dtype == torch.bfloat16:
        steps = R.bf16_steps(dz.cpu(), d64.to(torch.bfloat16))
        assert steps.max().item() <= 1, (what, "dlogits bf16 steps", steps.max().item())
    else:
        err = (dz.cpu().double() - d64).abs()
        bound = torch.maximum(2.0 * (d32.double() - d64).abs(), R.ulp32(d64))
        worst = (err / bound).max().item()
        print(f"{what}: dlogits err / bound {worst:.3f}")
        assert worst <= 1.0, (what, "dlogits", worst)
    return loss, hit, dz


def _sweep(make_logits, labels, B, gen, what, pm60=None):
    for (criterion, smoothing), dtype, (pname, w, perm) in itertools.product(MODES, DTYPES, _plans(B, gen)):
        plan = None if w is None else R.device_plan(B, w, perm, "cuda")
        _check(make_logits(dtype), labels, criterion, smoothing, plan, gen,
               f"{what} {criterion} a={smoothing} {str(dtype)[6:]} {pname}", pm60)


# L = 1, 3: k = L < 5; 8; 1000: the presets; 1003: odd row bases; 1024 / 1025: the last wave-per-row
# length and the first workgroup-per-row one; 21841: many passes per thread
SHAPES = [(B, L) for B in (1, 3, 130) for L in (1, 3, 8, 1000, 1003)] + [(3, 1024), (3, 1025), (2, 21841)]


@pytest.mark.parametrize("B, L", SHAPES)
def test_random_logits(B, L):
    gen = torch.Generator().manual_seed(1000 * B + L)
    z = 4.0 * torch.randn(B, L, generator=gen)
    labels = torch.randint(0, L, (B,), generator=gen)
    _sweep(lambda dt: z.to(dt).cuda(), labels, B, gen, f"B={B} L={L}")


@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1003, 1025])
def test_structured_rows(L):
    """+-60 logits, all-equal rows, the label at rank 0 / 4 / 5 and tied with the rank-4 value."""
    gen = torch.Generator().manual_seed(L)
    rows = {dt: R.structured_rows(L, dt, torch.Generator().manual_seed(L)) for dt in DTYPES}
    labels, names = rows[torch.float32][1:]
    pm60 = torch.tensor([n[:3] in ("+60", "-60") for n in names])
    assert 2 <= pm60.sum() <= 3
    _sweep(lambda dt: rows[dt][0].cuda(), labels, labels.shape[0], gen, f"structured L={L}", pm60)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hits_equal_topk_on_distinct_top_six(dtype):
    """Against the composition's own torch.topk accuracy, on rows whose six largest values are distinct
    (verified here, no row skipped)."""
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    gen = torch.Generator().manual_seed(9)
    for L in (1, 3, 8, 1000):
        B = 64
        z = R.distinct_top6_rows(B, L, dtype, gen)
        top = z.float().sort(-1, descending=True).values[:, :6]
        assert (top[:, :-1] > top[:, 1:]).all()
        labels = torch.randint(0, L, (B,), generator=gen)
        # half the labels among the raised classes, so that both outcomes occur
        raised = z.float().topk(min(6, L), -1).indices
        pick = torch.randint(0, raised.shape[1], (B,), generator=gen)
        labels[::2] = raised[torch.arange(B), pick][::2]
        plan = R.device_plan(B, 0.5, torch.roll(torch.arange(B), 1), "cuda")
        for p in (None, plan):
            t = R.targets32(labels, L, 0.1, R.plan_to_cpu(p))
            a1, a5 = FinetuneModel.accuracy(z.float(), t)
            perm, w = (None, None) if p is None else (p["dev"]["perm"], p["dev"]["params"][2:3])
            _, hit, _ = _ext().cls_loss_fwd(z.cuda(), labels.cuda(), perm, w, 0.1, 0)
            assert torch.equal(hit[:, 0].cpu(), a1) and torch.equal(hit[:, 1].cpu(), a5)
            if L >= 8:
                assert 0 < a5.sum() < B


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_view_reads_nothing_past_L(dtype):
    """logits as the [:, :1000] view of a [B, 1024] buffer whose pad columns are NaN."""
    gen = torch.Generator().manual_seed(3)
    B, L = 5, 1000
    z = (4.0 * torch.randn(B, L, generator=gen)).to(dtype)
    buf = torch.full((B, 1024), float("nan"), dtype=dtype, device="cuda")
    buf[:, :L] = z.cuda()
    view = buf[:, :L]
    assert view.stride(0) == 1024 and not view.is_contiguous()
    labels = torch.randint(0, L, (B,), generator=gen)
    plan = R.device_plan(B, 0.3, torch.roll(torch.arange(B), 2), "cuda")
    for criterion, smoothing in MODES:
        g1, g2 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
        a = _check(view, labels, criterion, smoothing, plan, g1, f"view {criterion} {smoothing}")
        b = _check(z.cuda(), labels, criterion, smoothing, plan, g2, f"dense {criterion} {smoothing}")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[2].float()).all() and torch.equal(a[2].float(), b[2].float())


def test_bad_arguments_raise():
    ext = _ext()
    B, L = 4, 10
    z = torch.randn(B, L, device="cuda")
    lab = torch.zeros(B, dtype=torch.int64, device="cuda")
    perm = torch.arange(B, dtype=torch.int32, device="cuda")
    w = torch.ones(1, device="cuda")
    loss, hit, lse = ext.cls_loss_fwd(z, lab, perm, w, 0.0, 0)
    dl = torch.ones(B, device="cuda")
    ext.cls_loss_bwd(dl, z, lab, perm, w, 0.0, 0, lse)
    bad_fwd = [
        (z.half(), lab, perm, w),                                   # dtype of the logits
        (z, lab.int(), perm, w),                                    # dtype of the labels
        (z, lab, perm.long(), w),                                   # dtype of perm
        (z, lab, perm, w.double()),                                 # dtype of w
        (z.cpu(), lab, perm, w),                                    # device
        (z, lab[:-1], perm, w),                                     # shape of the labels
        (z, lab, perm[:-1], w),                                     # shape of perm
        (z, lab, perm, None),                                       # perm without w
        (z[0], lab, perm, w),                                       # logits not 2-D
        (torch.randn(L, B, device="cuda").t(), lab, perm, w),       # column stride != 1
        (torch.randn(B, 2 * L, device="cuda")[:, ::2], lab, perm, w),
    ]
    for args in bad_fwd:
        with pytest.raises((RuntimeError, TypeError)):
            ext.cls_loss_fwd(*args, 0.0, 0)
        with pytest.raises((RuntimeError, TypeError)):
            ext.cls_loss_bwd(dl, *args, 0.0, 0, lse)
    for bad_dl, bad_lse in [(dl[:-1], lse), (dl.double(), lse), (dl, lse[:-1]), (dl, lse[:, 0]), (dl, lse.double())]:
        with pytest.raises(RuntimeError):
            ext.cls_loss_bwd(bad_dl, z, lab, perm, w, 0.0, 0, bad_lse)
    with pytest.raises(RuntimeError):
        ext.cls_loss_fwd(z, lab, perm, w, 0.0, 2)
    with pytest.raises(RuntimeError):
        ext.cls_loss_fwd(z, lab, perm, w, 1.0, 0)
    torch.cuda.synchronize()


def test_op_copies_overlapping_rows_and_takes_any_single_row():
    """ops.functional.cls_loss: an expanded (row stride 0) batch is copied, a single row may have any
    row stride; both give the contiguous tensor's results."""
    from jumbo_mae_tpu_amd.ops import functional as Fn
    g = torch.Generator().manual_seed(11)
    row = (4.0 * torch.randn(1, 40, generator=g)).cuda()
    labels = torch.tensor([3, 7, 3], device="cuda")
    want = Fn.cls_loss(row.repeat(3, 1), labels, None, 0.1, "ce")
    got = Fn.cls_loss(row.expand(3, 40), labels, None, 0.1, "ce")
    one = torch.as_strided(row, (1, 40), (7, 1))
    assert one.stride(0) == 7
    got1 = Fn.cls_loss(one, labels[:1], None, 0.1, "ce")
    want1 = Fn.cls_loss(row.clone(), labels[:1], None, 0.1, "ce")
    a = _ext().cls_loss_fwd(one, labels[:1], None, None, 0.1, 0)
    torch.cuda.synchronize()
    for x, y in zip(got + got1 + (a[0],), want + want1 + (want1[0],)):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError):
        _ext().cls_loss_fwd(row.expand(3, 40), labels, None, None, 0.1, 0)


# ------------------------------------------------------------------------------------ model level
def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _tiny(criterion):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.utils.mixup import Mixup
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=1000, image_size=32, patch_size=16, posemb="learnable")
    return FinetuneModel(vc, Mixup(0.8, 1.0, seed=3), label_smoothing=0.1, criterion=criterion).to(
        "cuda", torch.bfloat16, seed=0)


@pytest.mark.parametrize("criterion", ["ce", "bce"])
def test_model_kernel_on_matches_kernel_off(criterion, monkeypatch):
    """A tiny FinetuneModel (mixup + cutmix, smoothing 0.1): the fused loss against the torch
    composition on the GPU, within the bf16-step tolerances of tests/test_model_gpu.py (loss 2 %,
    flat gradient cosine 0.99, 2-D leaves 0.99, the others 0.95); the accuracies are equal (same logits,
    exact hits); a spy sees the kernel path taken with the head's bf16 logits."""
    from jumbo_mae_tpu_amd.ops import functional as Fn
    from jumbo_mae_tpu_amd.ops import prims as P
    calls = []
    real = Fn.cls_loss

    def spy(logits, labels, plan, smoothing, crit):
        calls.append((logits.dtype, logits.is_cuda, plan is not None, smoothing, crit))
        return real(logits, labels, plan, smoothing, crit)

    monkeypatch.setattr(Fn, "cls_loss", spy)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (16, 3, 32, 32), dtype=torch.uint8, generator=g).cuda()
    labels = torch.randint(0, 1000, (16,), generator=g).cuda()
    ev_labels = torch.where(torch.arange(16, device="cuda") % 4 == 1, torch.full_like(labels, -1), labels)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(P, "_CLS_LOSS_OURS", on)
        m = _tiny(criterion)
        out = m(imgs, labels)
        out["loss"].backward()
        ev = m.evaluate(imgs, ev_labels)
        torch.cuda.synchronize()
        res[on] = (out, m.store.grad.clone(), ev, m)
    assert len(calls) == 2, calls  # forward and evaluate of the kernel-on model only
    assert calls[0] == (torch.bfloat16, True, True, 0.1 if criterion == "ce" else 0.0, criterion)
    assert calls[1] == (torch.bfloat16, True, False, 0.0, criterion)
    (o1, g1, e1, m1), (o0, g0, e0, _) = res[True], res[False]
    assert abs(o1["loss"].item() - o0["loss"].item()) / abs(o0["loss"].item()) < 2e-2
    assert o1["acc1"].item() == o0["acc1"].item() and o1["acc5"].item() == o0["acc5"].item()
    assert _cos(g1, g0) > 0.99
    for s in m1.store.segments:
        a, b = g0[s.offset:s.offset + s.numel], g1[s.offset:s.offset + s.numel]
        if a.norm() <= 1e-3 * g0.norm() / len(m1.store.segments) ** 0.5:
            continue
        assert _cos(a, b) > (0.99 if len(s.shape) == 2 else 0.95), s.key
    assert e1["num_samples"].item() == e0["num_samples"].item() == 12
    assert abs(e1["loss"].item() - e0["loss"].item()) / abs(e0["loss"].item()) < 2e-2
    assert e1["acc1"].item() == e0["acc1"].item() and e1["acc5"].item() == e0["acc5"].item()


def test_out_of_range_labels_are_clamped():
    """Labels / perm entries out of range never trap: they are clamped (as the composition clamps the
    labels) and give the clamped classes' results."""
    ext = _ext()
    z = torch.randn(3, 7, device="cuda")
    bad = torch.tensor([-5, 99, 2], device="cuda")
    good = torch.tensor([0, 6, 2], device="cuda")
    perm_bad = torch.tensor([7, -1, 1], dtype=torch.int32, device="cuda")
    perm_good = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    w = torch.full((1,), 0.3, device="cuda")
    a = ext.cls_loss_fwd(z, bad, perm_bad, w, 0.1, 0)
    b = ext.cls_loss_fwd(z, good, perm_good, w, 0.1, 0)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ext.debug_lines()  # release build: empty; debug build: the loss TU's line, cleared by the read
    assert ext.debug_lines() == {}
