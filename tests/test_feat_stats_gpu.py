"""Representation monitor on the GPU: ``jm_feat_gram`` and ``jm_feat_uniformity`` (csrc/feat_stats.hip)
against the plain loops of tests/feat_stats_ref.py and the fp64 torch compositions, and the monitor
through ``PretrainModel`` / ``evaluate`` with the kernels on and off.

Bounds.  Gram: on exactly summable inputs every partial sum is exact, so G and s equal the oracle bit
for bit; on random inputs an element is a chain of n fp64 additions of exact products, each rounding
at most 2^-53 of a partial sum that is at most S = sum |products|: |G - ref| <= n 2^-53 S.
Uniformity: the score of a pair comes from v_mfma_f32_16x16x32_bf16 and is within eps = 2 D 2^-24 of the
fp64 dot product (tests/test_knn_gpu.py), so every term exp(-2 t (1 - s)) is within a factor
exp(2 t eps) of the oracle's and |e - ref| <= ref expm1(2 t eps); exp and the sums are fp64, whose own
error is covered by the floor max(2 x the fp32 composition's error, 1 fp32 ulp of ref).  On exactly
summable inputs the scores are exact: eps = 0."""

import math
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import feat_stats_ref as FR
import knn_ref as KR
from jumbo_mae_tpu_amd.ops import _ext
from jumbo_mae_tpu_amd.ops import feat_stats as FS
from jumbo_mae_tpu_amd.ops import knn as K
from jumbo_mae_tpu_amd.ops import prims as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAM_N = [1, 3, 4, 5, 63, 64, 65, 203]
GRAM_D = [1, 3, 64, 65, 96, 200]


def _gram(x, valid=None, state=None):
    st = FS.new_state(x.shape[1], "cuda") if state is None else state
    FS.feat_gram(x.cuda(), None if valid is None else valid.cuda(), st)
    torch.cuda.synchronize()
    return st


def _oracle_gram(x, valid=None):
    return FS.feat_gram_torch(x, valid, FS.new_state(x.shape[1], "cpu"), dtype=torch.float64)


# ------------------------------------------------------------------ Gram
@pytest.mark.parametrize("D", GRAM_D)
def test_gram_exact_inputs_bit_equal(D):
    for n in GRAM_N:
        x = FR.exact_rows(n, D, seed=n * 1000 + D)
        want = _oracle_gram(x)
        st = _gram(x)
        assert torch.equal(st["G"].cpu(), want["G"]) and torch.equal(st["s"].cpu(), want["s"]), (n, D)
        assert float(st["n"]) == n
        assert torch.equal(st["G"], st["G"].t())
        # two batches into one state equal the concatenated batch, at every split
        for cut in sorted({0, 1, n // 2, n - 1, n}):
            two = _gram(x[:cut]) if cut else FS.new_state(D, "cuda")
            two = _gram(x[cut:], state=two) if cut < n else two
            assert torch.equal(two["G"], st["G"]) and torch.equal(two["s"], st["s"]), (n, D, cut)
    if D <= 65:  # the loops themselves, at the sizes they can afford
        x = FR.exact_rows(65, D, seed=D)
        G, s, _, _ = FR.gram_loops(x)
        st = _gram(x)
        assert torch.equal(st["G"].cpu(), G) and torch.equal(st["s"].cpu(), s)


@pytest.mark.parametrize("D", GRAM_D)
def test_gram_random_inputs_within_the_chain_bound(D):
    g = torch.Generator().manual_seed(D)
    for n in GRAM_N:
        x = torch.randn(n, D, generator=g) * torch.exp(2 * torch.randn(n, 1, generator=g))
        xd = x.double()
        want = _oracle_gram(x)
        S = xd.abs().t() @ xd.abs()
        st = _gram(x)
        err = (st["G"].cpu() - want["G"]).abs()
        bound = n * 2.0 ** -53 * S
        print(f"feat_gram random ({n}, {D}): max err / (n 2^-53 S) = {(err / (n * 2.0 ** -53 * S)).max():.3f}")
        assert (err <= bound).all(), (n, D)
        es = (st["s"].cpu() - want["s"]).abs()
        assert (es <= n * 2.0 ** -53 * xd.abs().sum(0)).all()
        assert torch.equal(st["G"], st["G"].t())
        if n >= 8:  # a cut at a multiple of the 4-row MFMA step runs the very same instructions
            cut = (n // 2) & ~3
            two = _gram(x[cut:], state=_gram(x[:cut]))
            assert torch.equal(two["G"], st["G"]) and torch.equal(two["s"], st["s"])
    x = torch.randn(65, D, generator=g)
    if D <= 65:  # against the correctly rounded loops: one chain's bound
        G, s, n, S = FR.gram_loops(x)
        st = _gram(x)
        assert ((st["G"].cpu() - G).abs() <= n * 2.0 ** -53 * S).all()
        assert ((st["s"].cpu() - s).abs() <= n * 2.0 ** -53 * x.double().abs().sum(0)).all()


@pytest.mark.parametrize("n,D", [(5, 3), (65, 65), (203, 96), (64, 200)])
def test_gram_mask_stride_poison_and_reruns(n, D):
    g = torch.Generator().manual_seed(n + D)
    x = FR.exact_rows(n, D, seed=n + D)
    valid = torch.rand(n, generator=g) < 0.6
    valid[0] = False
    bad = x.clone()
    bad[~valid] = float("nan")  # NaN and inf rows behind the mask
    if n > 2:
        bad[0] = float("inf")
    want = _oracle_gram(x, valid)
    # rows ld > D apart inside a NaN-filled allocation; the state inside NaN-filled allocations too
    ld = D + 5
    buf = torch.full((n + 2, ld), float("nan"), device="cuda")
    view = buf[1:n + 1, 2:2 + D]
    view.copy_(bad.cuda())
    before = buf.clone()
    gbuf = torch.full((D * D + 16,), float("nan"), dtype=torch.float64, device="cuda")
    sbuf = torch.full((D + 16,), float("nan"), dtype=torch.float64, device="cuda")
    st = {"G": gbuf[8:8 + D * D].view(D, D).zero_(), "s": sbuf[8:8 + D].zero_(),
          "n": torch.zeros(1, dtype=torch.float64, device="cuda")}
    FS.feat_gram(view, valid.cuda(), st)
    torch.cuda.synchronize()
    assert torch.equal(st["G"].cpu(), want["G"]) and torch.equal(st["s"].cpu(), want["s"])
    assert float(st["n"]) == int(valid.sum())
    assert torch.isnan(gbuf[:8]).all() and torch.isnan(gbuf[8 + D * D:]).all()
    assert torch.isnan(sbuf[:8]).all() and torch.isnan(sbuf[8 + D:]).all()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))  # the inputs keep their bits
    # reruns are bit-identical (random values: the order of the additions shows)
    xr = torch.randn(n, D, generator=g).cuda()
    a, b = FS.new_state(D, "cuda"), FS.new_state(D, "cuda")
    FS.feat_gram(xr, valid.cuda(), a)
    FS.feat_gram(xr, valid.cuda(), b)
    assert torch.equal(a["G"], b["G"]) and torch.equal(a["s"], b["s"])
    # an all-masked batch and an empty one leave the state as it is
    FS.feat_gram(bad.cuda(), torch.zeros(n, dtype=torch.bool, device="cuda"), a)
    FS.feat_gram(xr[:0], None, a)
    assert torch.equal(a["G"], b["G"]) and torch.equal(a["s"], b["s"]) and float(a["n"]) == float(b["n"])


def test_gram_bad_arguments():
    ext = _ext.load(True)
    x = torch.zeros(8, 16, device="cuda")
    G = torch.zeros(16, 16, dtype=torch.float64, device="cuda")
    s = torch.zeros(16, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="fp32"):
        ext.feat_gram(x.double(), None, G, s)
    with pytest.raises(RuntimeError, match="G must be"):
        ext.feat_gram(x, None, G.float(), s)
    with pytest.raises(RuntimeError, match="G must be"):
        ext.feat_gram(x, None, G[:, :8], s[:8])
    with pytest.raises(RuntimeError, match="s must be"):
        ext.feat_gram(x, None, G, s[:8])
    with pytest.raises(RuntimeError, match="valid must be"):
        ext.feat_gram(x, torch.ones(7, dtype=torch.bool, device="cuda"), G, s)
    with pytest.raises(RuntimeError, match="unit column stride"):
        ext.feat_gram(torch.zeros(16, 8, device="cuda").t(), None, G, s)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.feat_gram(x.cpu(), None, G.cpu(), s.cpu())
    with pytest.raises(ValueError, match="x must be"):
        FS.feat_gram(x[:, :8], None, {"G": G, "s": s, "n": s[:1]})
    torch.cuda.synchronize()
    assert not G.any() and not s.any()


# ------------------------------------------------------------------ uniformity
UNIF_SHAPES = [(1, 1, 32), (3, 5, 32), (37, 203, 96), (130, 130, 64)]


def _ulp32(v):
    """One fp32 ulp of the fp64 values ``v``."""
    f = v.float().abs()
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()


def _check_unif(q, bank, self_idx, bank_valid, t, eps, splits=0):
    ref = FR.uniformity_loops(q, bank, self_idx, bank_valid, t)
    comp = FS.feat_uniformity_torch(q, bank, self_idx, bank_valid, t, dtype=torch.float32)
    floor = torch.maximum(2 * (comp - ref).abs(), _ulp32(ref))
    bound = ref * math.expm1(2 * t * eps) + floor
    dev = [None if a is None else a.cuda() for a in (self_idx, bank_valid)]
    e = FS.feat_uniformity(q.cuda(), bank.cuda(), dev[0], dev[1], t, splits=splits).cpu()
    assert e.dtype == torch.float64 and e.shape == ref.shape
    err = (e - ref).abs()
    print(f"feat_uniformity {tuple(q.shape)} x {tuple(bank.shape)} eps={eps:.2e}: max err {err.max():.3e}, "
          f"max err / bound {(err / bound.clamp(min=1e-300)).max():.3e}")
    assert (err <= bound).all()
    return e


@pytest.mark.parametrize("Nq,Nb,D", UNIF_SHAPES)
@pytest.mark.parametrize("masks", ["none", "self", "valid", "both"])
def test_uniformity_exact_and_random(Nq, Nb, D, masks):
    g = torch.Generator().manual_seed(Nq + Nb)
    self_idx = torch.randint(-1, Nb, (Nq,), generator=g).to(torch.int32) if masks in ("self", "both") else None
    bank_valid = (torch.rand(Nb, generator=g) < 0.7) if masks in ("valid", "both") else None
    q, bank = KR.exact_inputs(Nq, Nb, D, seed=Nq + D)
    _check_unif(q, bank, self_idx, bank_valid, 2.0, 0.0)
    q = K.normalize_features(torch.randn(Nq, D, generator=g))
    bank = K.normalize_features(torch.randn(Nb, D, generator=g))
    if bank_valid is not None and Nb > 2:  # NaN rows behind the mask
        bank = bank.clone()
        bank[~bank_valid] = float("nan")
    for t in (2.0, 0.5):
        _check_unif(q, bank, self_idx, bank_valid, t, 2 * D * 2.0 ** -24)


def test_uniformity_segments_and_splits():
    """More than one bank segment (1024 rows each), a last one that is not full; the way the segments
    are dealt to workgroups never shows."""
    ext = _ext.load(True)
    Nq, Nb, D = 130, 2 * 1024 + 70, 32
    assert ext.feat_uniformity_segments(Nb) == 3 and ext.feat_uniformity_segments(1024) == 1
    g = torch.Generator().manual_seed(3)
    q = K.normalize_features(torch.randn(Nq, D, generator=g))
    bank = K.normalize_features(torch.randn(Nb, D, generator=g))
    self_idx = torch.randint(-1, Nb, (Nq,), generator=g).to(torch.int32)
    bank_valid = torch.rand(Nb, generator=g) < 0.9
    ref = FS.feat_uniformity_torch(q, bank, self_idx, bank_valid, 2.0, dtype=torch.float64)
    comp = FS.feat_uniformity_torch(q, bank, self_idx, bank_valid, 2.0, dtype=torch.float32)
    outs = [FS.feat_uniformity(q.cuda(), bank.cuda(), self_idx.cuda(), bank_valid.cuda(), 2.0, splits=s).cpu()
            for s in (0, 1, 2, 3, 7)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    eps = 2 * D * 2.0 ** -24
    bound = ref * math.expm1(4 * eps) + torch.maximum(2 * (comp - ref).abs(), _ulp32(ref))
    assert ((outs[0] - ref).abs() <= bound).all()
    qe, be = KR.exact_inputs(40, Nb, D, seed=9)
    _check_unif(qe, be, None, None, 2.0, 0.0, splits=2)


def test_uniformity_all_masked_leave_one_out_poison_and_reruns():
    Nq = Nb = 130
    D = 64
    q, _ = KR.exact_inputs(Nq, Nb, D, seed=4, q_from_bank=False)
    me = torch.arange(Nq, dtype=torch.int32)
    dq = q.cuda()
    # a bank in which every row is masked gives 0
    e = FS.feat_uniformity(dq, dq, None, torch.zeros(Nb, dtype=torch.bool, device="cuda"), 2.0)
    assert e.shape == (Nq,) and not e.any()
    # leave-one-out: the full sum minus the row's own term, which the oracle confirms
    loo = _check_unif(q, q, me, None, 2.0, 0.0)
    full = _check_unif(q, q, None, None, 2.0, 0.0)
    own = torch.exp(-4.0 * (1.0 - (q.double() ** 2).sum(1)))
    assert torch.allclose(full - loo, own, rtol=1e-12, atol=0)
    # e inside a NaN-filled allocation
    buf = torch.full((Nq + 16,), float("nan"), dtype=torch.float64, device="cuda")
    out = FS.feat_uniformity(dq, dq, me.cuda(), None, 2.0, out=buf[8:8 + Nq])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf[8:].data_ptr() and torch.equal(out.cpu(), loo)
    assert torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + Nq:]).all()
    # reruns on random rows are bit-identical, and the inputs keep their bits
    g = torch.Generator().manual_seed(0)
    r = K.normalize_features(torch.randn(Nq, D, generator=g)).cuda()
    keep = r.clone()
    a = FS.feat_uniformity(r, r, me.cuda(), None, 2.0)
    b = FS.feat_uniformity(r, r, me.cuda(), None, 2.0)
    assert torch.equal(a, b) and torch.equal(r.view(torch.int16), keep.view(torch.int16))


def test_uniformity_bad_arguments_and_routing(monkeypatch):
    ext = _ext.load(True)
    q = torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ext.feat_uniformity(q[:, :48], q[:, :48])
    with pytest.raises(RuntimeError, match="t must be positive"):
        ext.feat_uniformity(q, q, t=0.0)
    with pytest.raises(RuntimeError, match="splits"):
        ext.feat_uniformity(q, q, splits=5000)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.feat_uniformity(q.float(), q.float())
    with pytest.raises(RuntimeError, match="self_idx"):
        ext.feat_uniformity(q, q, self_idx=torch.zeros(7, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="bank_valid"):
        ext.feat_uniformity(q, q, bank_valid=torch.ones(7, dtype=torch.bool, device="cuda"))
    flat = torch.zeros(8 * 64 + 8, dtype=torch.bfloat16, device="cuda")
    odd = flat[4:4 + 8 * 64].view(8, 64)  # rows 8 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="feat_uniformity"):
        ext.feat_uniformity(odd, q)
    with pytest.raises(ValueError, match="t must be positive"):
        FS.feat_uniformity(q, q, t=-1.0)
    torch.cuda.synchronize()
    # routing, with a spy on the bindings and on the compositions
    calls = []
    real = _ext.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name in ("feat_gram", "feat_uniformity"):
                return lambda *a, **kw: (calls.append(name), fn(*a, **kw))[1]
            return fn

    monkeypatch.setattr(FS._ext, "load", lambda *a, **kw: Spy())
    ut, gt = FS.feat_uniformity_torch, FS.feat_gram_torch
    monkeypatch.setattr(FS, "feat_uniformity_torch", lambda *a, **kw: (calls.append("unif_torch"), ut(*a, **kw))[1])
    monkeypatch.setattr(FS, "feat_gram_torch", lambda *a, **kw: (calls.append("gram_torch"), gt(*a, **kw))[1])
    qa, ba = KR.exact_inputs(8, 40, 64, seed=15)
    flat[4:4 + 8 * 64] = qa.cuda().reshape(-1)
    want = FR.uniformity_loops(qa, ba)
    assert torch.allclose(FS.feat_uniformity(odd, ba.cuda()).cpu(), want, rtol=1e-12)  # realigned by the Python layer
    assert calls == ["feat_uniformity"]
    e48 = FS.feat_uniformity(qa[:, :48].cuda(), ba[:, :48].cuda())  # no multiple of 32: the composition
    assert calls == ["feat_uniformity", "unif_torch"] and e48.is_cuda
    assert torch.allclose(e48.cpu(), FR.uniformity_loops(qa[:, :48], ba[:, :48]), rtol=1e-5)
    x = FR.exact_rows(9, 40, seed=1).cuda()
    st = FS.feat_gram(x, None, FS.new_state(40, "cuda"))
    assert calls[2:] == ["feat_gram"]
    monkeypatch.setattr(P, "_FEAT_STATS_OURS", False)
    st2 = FS.feat_gram(x, None, FS.new_state(40, "cuda"))
    FS.feat_uniformity(qa.cuda(), ba.cuda())
    assert calls[3:] == ["gram_torch", "unif_torch"]
    assert torch.equal(st["G"], st2["G"]) and torch.equal(st["s"], st2["s"])


# ------------------------------------------------------------------ model level
def _tiny_model():
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel

    kw = dict(layers=2, dim=64, heads=2, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.1)
    pm = PretrainModel(ViTConfig(labels=0, image_mask_ratio=0.75, **kw),
                       DecoderConfig(dec_layers=1, dec_dim=64, dec_heads=2, image_size=32, patch_size=16))
    return pm.to("cuda", torch.bfloat16, seed=0)


def test_evaluate_with_the_kernels_and_with_the_compositions(monkeypatch):
    """val/feat_* through ``evaluate`` with _FEAT_STATS_OURS on and off, with and without labels.

    How the kernel bounds reach the metrics: both arms see the same fp32 features (the model is
    deterministic).  The Gram state of the two arms differs by at most 2 n 2^-53 S per element (kernel
    chain and fp64 matmul, each within n 2^-53 S of the exact sum), a relative perturbation of G of
    about 1e-14 in norm; eigenvalues move by at most that norm (Weyl), singular values by its square
    root relative to sigma_max at worst, so rankme / pr / top1_var / std / rms_norm are compared at
    1e-6 relative -- far above the propagated error, far below any change of meaning.  The
    uniformity's arms are the kernel and the FP32 composition: each is within ref expm1(2 t eps),
    eps = 2 D 2^-24 = 2.3e-5 at D = 192 (the composition's fp32 matmul obeys the same dot-product bound),
    of the oracle, so log(e_sum / pairs) differs by at most 2 * 2 t eps = 16 D 2^-24 = 1.9e-4."""
    from jumbo_mae_tpu_amd.train import pretrain as PT
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    model = _tiny_model()
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (8, 3, 32, 32), generator=g, dtype=torch.uint8) for _ in range(3)]
    labels = [torch.arange(8) % 4 for _ in range(3)]
    labels[2] = labels[2].clone()
    labels[2][5:] = -1  # padding rows
    dev = torch.device("cuda")
    before = model.store.master.clone()

    def run(with_labels, flag=True):
        loader = [(i, y) for i, y in zip(imgs, labels)] if with_labels else list(imgs)
        return PT.evaluate(model, loader, RngStreams({"noise": 0, "dropout": 0, "mixup": 0}, 0, dev), dev, 0, 0.07, None,
                           flag, 2.0)

    keys = {"val/feat_rankme", "val/feat_pr", "val/feat_top1_var", "val/feat_std", "val/feat_rms_norm",
            "val/feat_uniformity", "val/feat_rows", "val/feat_nonfinite"}
    off = run(True, flag=False)
    assert set(off) == {"val/loss"}
    for with_labels, rows in ((True, 21), (False, 24)):
        ours = run(with_labels)
        assert keys <= set(ours) and ours["val/feat_rows"] == rows and ours["val/feat_nonfinite"] == 0
        assert 1.0 <= ours["val/feat_rankme"] <= rows and all(math.isfinite(v) for v in ours.values())
        monkeypatch.setattr(P, "_FEAT_STATS_OURS", False)
        comp = run(with_labels)
        monkeypatch.setattr(P, "_FEAT_STATS_OURS", True)
        print(with_labels, ours, comp)
        for k in keys - {"val/feat_uniformity"}:
            assert abs(ours[k] - comp[k]) <= 1e-6 * abs(comp[k]), (k, ours[k], comp[k])
        assert abs(ours["val/feat_uniformity"] - comp["val/feat_uniformity"]) <= 16 * 192 * 2.0 ** -24
    assert torch.equal(model.store.master, before)  # the monitor leaves the weights alone


# ------------------------------------------------------------------ debug build
DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.debug_build and ext.debug_lines() == {}
    x = (torch.arange(70 * 65, device="cuda").reshape(70, 65) % 7 - 3).float()
    G = torch.zeros(65, 65, dtype=torch.float64, device="cuda")
    s = torch.zeros(65, dtype=torch.float64, device="cuda")
    ext.feat_gram(x, None, G, s)
    q = ((torch.arange(5 * 32, device="cuda").reshape(5, 32) % 5 - 2).float() / 8).bfloat16()
    me = torch.arange(5, dtype=torch.int32, device="cuda")
    e = ext.feat_uniformity(q, q, me, None, 2.0)
    torch.cuda.synchronize()
    assert ext.debug_lines() == {}
    assert torch.equal(G, x.double().t() @ x.double()) and torch.equal(s, x.double().sum(0))
    me[0] = 5                                   # one past the bank: matches no row, and recorded
    e2 = ext.feat_uniformity(q, q, me, None, 2.0)
    torch.cuda.synchronize()
    lines = ext.debug_lines()
    assert set(lines) == {"feat_stats"} and lines["feat_stats"] > 0, lines
    full = ext.feat_uniformity(q, q, None, None, 2.0)
    assert e2[0] == full[0] and torch.equal(e2[1:], e[1:])
    print("FEAT_STATS_DEBUG_OK")
""")


def test_debug_build_checks_the_self_indices():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "FEAT_STATS_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
