"""The fused distillation loss kernels (csrc/distill.hip) against the definition in fp64 on the CPU
(tests/distill_ref.py), fed the same already rounded logits, and the model / train-step level of
``--teacher-ckpt``.

Bounds (the rule of tests/test_cls_loss_gpu.py): ``agree`` and the teacher arg-max ``t`` equal the oracle
exactly; a row's kd (and, on fp32 logits, a gradient element) may miss the fp64 value by max(2 x the
error of the fp32 torch composition ``kd_loss_torch`` on the same input, 1 fp32 ulp of the value) -- the
bound comes from the path the kernels replace, computed here, never from the kernel; on bf16 logits
the gradient is within 1 bf16 step of the fp64 gradient rounded to bf16.  Every case runs twice and must
be bit-identical.

The +-60 structured rows need no second oracle: tests/test_distill.py
(test_oracle_does_not_cancel_on_the_structured_rows) shows two algebraic forms of the fp64 value
agreeing to 1e-3 fp32 ulp on every row of ``distill_ref.pair_rows``.

Model level: metrics with the kernels on equal the fp64 oracle of the (captured) logits within the mean
of the per-row bounds plus the fp32 mean's own rounding, (B / 2 + 1) ulp: B - 1 additions of
non-negative terms and one division, half an ulp of at most the result each."""

import pytest
import torch

import distill_ref as D

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
MODES = [("soft", 1.0), ("soft", 2.0), ("soft", 4.0), ("hard", 1.0)]


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _check(z, u, T, mode, gen, what):
    """One forward + backward of the kernels on GPU tensors ``z``, ``u`` (maybe views), twice, against
    the oracle.  Returns (kd, agree, t, dz)."""
    ext = _ext()
    B, L = z.shape
    m = 0 if mode == "soft" else 1
    dloss = (0.25 + torch.rand(B, generator=gen)) / B  # non-uniform
    dl = dloss.cuda()
    outs = []
    for _ in range(2):
        kd, agree, lse, t = ext.kd_loss_fwd(z, u, T, m)
        dz = ext.kd_loss_bwd(dl, z, u if m == 0 else None, T, m, lse, t if m == 1 else None)
        outs.append((kd, agree, lse, t, dz))
    torch.cuda.synchronize()
    (kd, agree, lse, t, dz), again = outs
    for a, b in zip(outs[0][:4], again[:4]):
        assert torch.equal(a, b), what
    assert torch.equal(_bits(dz), _bits(again[4])), what
    assert dz.dtype == z.dtype and dz.shape == z.shape and dz.is_contiguous()
    assert kd.dtype == torch.float32 and agree.dtype == torch.bool and t.dtype == torch.int32

    zc, uc = z.cpu(), u.cpu()
    k64, d64, t64, a64 = D.oracle(zc, uc, T, mode, dloss)
    k32, d32 = D.composition32(zc, uc, T, mode, dloss)
    assert torch.equal(t.cpu().long(), t64) and torch.equal(agree.cpu(), a64), what
    err, bound = (kd.cpu().double() - k64).abs(), D.bound(k32, k64)
    worst = (err / bound).max().item()
    print(f"{what}: kd err / bound {worst:.3f}")
    assert worst <= 1.0, (what, "kd", worst, int((err / bound).argmax()))
    if z.dtype == torch.bfloat16:
        steps = D.bf16_steps(dz.cpu(), d64.to(torch.bfloat16))
        print(f"{what}: dz bf16 steps {steps.max().item()}")
        assert steps.max().item() <= 1, (what, "dz bf16 steps", steps.max().item())
    else:
        err, bound = (dz.cpu().double() - d64).abs(), D.bound(d32, d64)
        worst = (err / bound).max().item()
        print(f"{what}: dz err / bound {worst:.3f}")
        assert worst <= 1.0, (what, "dz", worst)
    return kd, agree, t, dz


# L = 1, 3, 8; 1000: the presets; 1003: odd row bases; 1024 / 1025: the last wave-per-row length and the
# first workgroup-per-row one; 21841: many passes per thread
SHAPES = [(B, L) for B in (1, 3, 130) for L in (1, 3, 8, 1000, 1003)] + [(3, 1024), (3, 1025), (2, 21841)]


@pytest.mark.parametrize("B, L", SHAPES)
def test_random_logits(B, L):
    gen = torch.Generator().manual_seed(1000 * B + L)
    z = 4.0 * torch.randn(B, L, generator=gen)
    u = 4.0 * torch.randn(B, L, generator=gen)
    for dtype in DTYPES:
        for mode, T in MODES:
            _check(z.to(dtype).cuda(), u.to(dtype).cuda(), T, mode, gen, f"B={B} L={L} {str(dtype)[6:]} {mode} T={T}")


@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1025])
def test_structured_rows(L):
    """+-60 logits, all-equal rows, ranked and tied rows for both operands; u == z; an all-equal teacher;
    the teacher's maximum tied between class 2 and the last class."""
    gen = torch.Generator().manual_seed(L)
    for dtype in DTYPES:
        z, u, names = D.pair_rows(L, dtype)
        for mode, T in MODES:
            kd, agree, t, dz = _check(z.cuda(), u.cuda(), T, mode, gen, f"structured L={L} {str(dtype)[6:]} {mode} T={T}")
            for r, name in enumerate(names):
                if name.startswith("u == z"):
                    assert agree[r].item()
                    if mode == "soft":
                        assert kd[r].item() == 0.0 and not dz[r].float().any().item(), (name, mode, T)
                if name == "all-equal teacher":
                    assert t[r].item() == 0
                if name == "teacher tie 2 / last":
                    assert t[r].item() == 2
        assert sum(n.startswith("u == z") for n in names) == 2 and "all-equal teacher" in names
        assert ("teacher tie 2 / last" in names) == (L > 3)
        assert sum("60" in n for n in names) >= 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_views_equal_the_contiguous_copy(dtype):
    """z and u as column slices of wider [B, L + 24] buffers at odd element offsets (NaN around them)."""
    gen = torch.Generator().manual_seed(5)
    for B, L in ((5, 1000), (3, 1025), (6, 8)):
        z = (4.0 * torch.randn(B, L, generator=gen)).to(dtype)
        u = (4.0 * torch.randn(B, L, generator=gen)).to(dtype)
        bz = torch.full((B, L + 24), float("nan"), dtype=dtype, device="cuda")
        bu = torch.full((B, L + 24), float("nan"), dtype=dtype, device="cuda")
        bz[:, 3:3 + L] = z.cuda()
        bu[:, 7:7 + L] = u.cuda()
        vz, vu = bz[:, 3:3 + L], bu[:, 7:7 + L]
        assert vz.stride(0) == L + 24 and not vz.is_contiguous() and vz.storage_offset() % 2 == 1
        for mode, T in (("soft", 2.0), ("hard", 1.0)):
            g1, g2 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
            a = _check(vz, vu, T, mode, g1, f"view {B}x{L} {mode}")
            b = _check(z.cuda(), u.cuda(), T, mode, g2, f"dense {B}x{L} {mode}")
            for x, y in zip(a[:3], b[:3]):
                assert torch.equal(x, y)
            assert torch.isfinite(a[3].float()).all() and torch.equal(_bits(a[3]), _bits(b[3]))


def test_bad_arguments_raise_and_the_op_takes_awkward_views():
    from jumbo_mae_tpu_amd.ops import functional as Fn
    ext = _ext()
    B, L = 4, 10
    z, u = torch.randn(B, L, device="cuda"), torch.randn(B, L, device="cuda")
    kd, agree, lse, t = ext.kd_loss_fwd(z, u, 1.0, 0)
    dl = torch.ones(B, device="cuda")
    for bad in [(z.half(), u.half()), (z, u.bfloat16()), (z.cpu(), u.cpu()), (z, u[:-1]), (z[0], u[0]),
                (torch.randn(L, B, device="cuda").t(), u.t().contiguous().t())]:
        with pytest.raises((RuntimeError, TypeError)):
            ext.kd_loss_fwd(*bad, 1.0, 0)
    for T, mode in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (1.0, 2)):
        with pytest.raises(RuntimeError):
            ext.kd_loss_fwd(z, u, T, mode)
    for args in [(dl[:-1], z, u, 1.0, 0, lse, None), (dl, z, None, 1.0, 0, lse, None), (dl, z, None, 1.0, 1, lse, None),
                 (dl, z, u, 1.0, 0, lse[:, :2].contiguous(), None), (dl, z, None, 1.0, 1, lse, t.long())]:
        with pytest.raises((RuntimeError, TypeError)):
            ext.kd_loss_bwd(*args)
    # the op copies overlapping rows (an expanded batch) and casts nothing
    row = (4.0 * torch.randn(1, 40, device="cuda"))
    want = Fn.kd_loss(row.repeat(3, 1), u[:3].repeat(1, 4), 2.0, "soft")
    got = Fn.kd_loss(row.expand(3, 40), u[:3].repeat(1, 4), 2.0, "soft")
    torch.cuda.synchronize()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    with pytest.raises(ValueError):
        Fn.kd_loss(z, u.bfloat16(), 1.0, "soft")
    assert ext.debug_lines() == {}


# ------------------------------------------------------------------------------------ model level
B_MODEL = 8


@pytest.fixture(autouse=True)
def own_step_feeder(monkeypatch):
    """The step feeder's static buffers are per process and sized by their first use (a run has one batch
    size); other test files feed other batch sizes through the same names, so every test here gets the
    feeder a fresh process would have and leaves the process's own untouched."""
    from jumbo_mae_tpu_amd.runtime import feeder
    monkeypatch.setattr(feeder, "_FEEDERS", {})


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def _models(alpha, T, mode, mixup=0.8, droppath=0.0, teacher=True):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.utils.mixup import Mixup
    kw = dict(labels=8, image_size=32, patch_size=16, posemb="learnable")
    s = FinetuneModel(ViTConfig(layers=2, dim=64, heads=2, droppath=droppath, **kw), Mixup(mixup, mixup and 1.0, seed=3),
                      label_smoothing=0.1).to("cuda", torch.bfloat16, seed=0)
    if not teacher:
        return s, None
    t = FinetuneModel(ViTConfig(layers=3, dim=96, heads=3, **kw)).freeze().to("cuda", torch.bfloat16, seed=1)
    s.attach_teacher(t, alpha, T, mode)
    return s, t


def _data(n=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (B_MODEL, 3, 32, 32), dtype=torch.uint8, generator=g).cuda(),
             torch.randint(0, 8, (B_MODEL,), generator=g).cuda()) for _ in range(n)]


@pytest.mark.parametrize("mode, T", [("soft", 2.0), ("hard", 1.0)])
def test_model_kernels_on_match_kernels_off(mode, T, monkeypatch):
    """One forward + backward of a tiny student (mixup + cutmix, smoothing 0.1) under a 3-layer teacher
    with prims._KD_OURS on and off, same seeds."""
    from jumbo_mae_tpu_amd.ops import functional as Fn
    from jumbo_mae_tpu_amd.ops import prims as P
    seen = []
    real = Fn.kd_loss

    def spy(z, u, T_, mode_):
        seen.append((z.detach().clone(), u.detach().clone(), T_, mode_))
        return real(z, u, T_, mode_)

    monkeypatch.setattr(Fn, "kd_loss", spy)
    (imgs, labels), = _data()
    res = {}
    for on in (True, False):
        monkeypatch.setattr(P, "_KD_OURS", on)
        s, t = _models(0.5, T, mode)
        before = t.store.master.clone()
        out = s(imgs, labels)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert t.store.grad is None and torch.equal(_bits(t.store.master), _bits(before))
        res[on] = ({k: v.item() for k, v in out.items()}, s.store.grad.clone())
    (z1, u1, T1, m1), (z0, u0, _, _) = seen
    assert z1.dtype == u1.dtype == torch.bfloat16 and z1.shape == (B_MODEL, 8) and (T1, m1) == (T, mode)
    assert torch.equal(_bits(z1), _bits(z0)) and torch.equal(_bits(u1), _bits(u0))  # the same logits both times
    (o1, g1), (o0, g0) = res[True], res[False]
    ones = torch.ones(B_MODEL)
    k64, _, _, a64 = D.oracle(z1.cpu(), u1.cpu(), T, mode, ones)
    k32, _ = D.composition32(z1.cpu(), u1.cpu(), T, mode, ones)
    tol = D.bound(k32, k64).mean().item() + (B_MODEL / 2 + 1) * D.ulp32(k64.mean()).item()
    print(f"{mode}: kd on {o1['kd_loss']!r} off {o0['kd_loss']!r} oracle {k64.mean().item()!r} tol {tol:.3g}")
    assert abs(o1["kd_loss"] - k64.mean().item()) <= tol
    assert abs(o1["kd_loss"] - o0["kd_loss"]) <= 2 * tol
    assert o1["kd_agree"] == o0["kd_agree"] == a64.float().mean().item()
    for k in ("cls_loss", "acc1", "acc5"):  # the base loss is the same kernel on the same logits
        assert o1[k] == o0[k], k
    want = 0.5 * o1["cls_loss"] + 0.5 * o1["kd_loss"]
    assert abs(o1["loss"] - want) <= 4 * D.ulp32(torch.tensor(want, dtype=torch.float64)).item()
    assert abs(o1["loss"] - o0["loss"]) <= tol + 4 * D.ulp32(torch.tensor(want, dtype=torch.float64)).item()
    assert _cos(g1, g0) > 0.999


def _trainer(model):
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams
    opt = FlatOptimizer(model.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 2, 20, 1e-6), weight_decay=0.05,
                        lr_decay=0.75, num_layers=model.cfg.layers)
    return Trainer(model, opt, None, RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, "cuda"))


def test_hip_graph_replays_match_eager_steps():
    """Three replayed steps through StepRunner (teacher forward captured with the rest) against three
    eager steps, on a deterministic configuration as in tests/test_graph_gpu.py (its tolerances: loss
    1e-4 relative, master atol 1e-6 / rtol 1e-5)."""
    from jumbo_mae_tpu_amd.runtime.graph import StepRunner
    data = _data(3, seed=2)
    (s1, t1), (s2, t2) = _models(0.5, 2.0, "soft", mixup=0.0), _models(0.5, 2.0, "soft", mixup=0.0)
    before = t2.store.master.clone()
    eager, graphed = StepRunner(_trainer(s1)), StepRunner(_trainer(s2), hip_graph=True)
    for mb in data:
        a, b = eager([mb]), graphed([mb])
        for k in ("loss", "kd_loss", "cls_loss"):
            assert abs(a[k].item() - b[k].item()) <= 1e-4 * max(1.0, abs(a[k].item())), k
        assert a["kd_agree"].item() == b["kd_agree"].item()
    torch.cuda.synchronize()
    assert graphed.graphed is not None and graphed.graphed.replays == 3
    assert torch.allclose(s1.store.master, s2.store.master, atol=1e-6, rtol=1e-5)
    assert torch.equal(_bits(t2.store.master), _bits(before)) and t2.store.grad is None


def test_alpha_zero_trains_exactly_as_without_a_teacher():
    """Mixup / CutMix and droppath on: the teacher takes nothing from the random streams, and alpha 0 adds
    nothing to the backward -- three steps end on the same master bits."""
    data = _data(3, seed=3)
    s1, _ = _models(0.0, 1.0, "soft", droppath=0.1)
    s0, _ = _models(0.0, 1.0, "soft", droppath=0.1, teacher=False)
    t1, t0 = _trainer(s1), _trainer(s0)
    for mb in data:
        a, b = t1.train_step([mb]), t0.train_step([mb])
        assert a["loss"].item() == b["loss"].item() == a["cls_loss"].item() and a["kd_loss"].item() > 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1.store.master), _bits(s0.store.master))
