"""Attention-rollout kernels (csrc/attn_rollout.hip) on the GPU against the fp64 composition.

The bound, per output tensor: every element of the kernel's result lies within
max(2 E32, 1 fp32 ulp of the largest |reference|) of the fp64 reference, E32 being the largest error of the fp32
torch composition on the same inputs against the same reference.  Both errors are printed per case.

Shapes: S in {1, 3, 52, 64, 65, 199} (one row, less than a tile, a full tile, one row more, four tiles with a
ragged last one) at every head dim, H in {1, 3}, B = 2, C in {1, 3, 8}, alpha in {0, 0.5, 1}.
"""

import os
import subprocess
import sys

import pytest
import torch

import attn_maps_ref as MR
import attn_stats_ref as AR

from jumbo_mae_tpu_amd.ops import attn_maps as AM
from jumbo_mae_tpu_amd.ops import prims as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEQS = (1, 3, 52, 64, 65, 199)
HEAD_DIMS = (32, 64, 80, 96, 128)


def _ext():
    return AM._ext.load()


def test_head_dims_are_the_attention_kernels():
    assert tuple(sorted(_ext().attn_head_dims())) == HEAD_DIMS


def _rows(B, C, S, seed):
    """Random non-negative rows; row 0 a one-hot, the last row (when C > 1) a one-hot on the last position."""
    r = torch.rand(B, C, S, generator=torch.Generator().manual_seed(seed))
    r[:, 0] = 0.0
    r[:, 0, min(1, S - 1)] = 1.0
    if C > 1:
        r[:, C - 1] = 0.0
        r[:, C - 1, S - 1] = 1.0
    return r


def _ref_step(qkv, H, r64, alpha):
    return AM.rollout_step_torch(qkv, H, r64, alpha, torch.float64)


def _check(name, got, comp, ref):
    """The bound of the module docstring; returns (kernel error, E32)."""
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), name
    err = float((got.double() - ref).abs().max())
    e32 = float((comp.double() - ref).abs().max())
    ulp = float(AR.ulp32(ref.abs().max()))
    print(f"attn_maps {name}: kernel {err:.3e} composition {e32:.3e} ulp {ulp:.3e} ratio {err / max(e32, ulp):.3f}")
    assert err <= max(2.0 * e32, ulp), (name, err, e32, ulp)
    return err, e32


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("S", SEQS)
def test_step_against_fp64(S, hd):
    B = 2
    for H in (1, 3):
        qkv = AR.random_qkv(B, S, H, hd, seed=S + hd + H, gain=1.5).to(DEV)  # logits span a few units
        for C in (1, 3, 8):
            r = _rows(B, C, S, seed=C).to(DEV)
            for alpha in (0.0, 0.5, 1.0):
                keep = (qkv.clone(), r.clone())
                got = AM.rollout_step(qkv, H, r, alpha)
                comp = AM.rollout_step_torch(qkv, H, r, alpha, torch.float32)
                _check(f"S={S} hd={hd} H={H} C={C} alpha={alpha}", got, comp, _ref_step(qkv, H, r.double(), alpha))
                assert torch.equal(qkv.view(torch.int16), keep[0].view(torch.int16)) and torch.equal(r, keep[1])
                # every row keeps its sum
                assert float((got.double().sum(-1) - r.double().sum(-1)).abs().max()) <= 1e-5 * max(1.0, S / 8)
                if alpha == 1.0:
                    assert torch.equal(got, r)


@pytest.mark.parametrize("S", [1, 4, 64, 256])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_uniform_attention_bit_for_bit(S, hd):
    """q = 0: out = alpha r + (1 - alpha) mean_q r, exact in fp32 and fp64 for dyadic rows and S a power of two."""
    B, C = 2, 3
    for H in (1, 4):
        qkv = MR.zero_query_qkv(B, S, H, hd, seed=S).to(DEV)
        r = MR.dyadic_rows(B, C, S, seed=H).to(DEV)
        for alpha in (0.0, 0.5, 1.0):
            want = alpha * r.double() + (1.0 - alpha) * r.double().mean(-1, keepdim=True)
            assert torch.equal(_ref_step(qkv, H, r.double(), alpha), want)  # the fp64 composition is exact
            assert torch.equal(AM.rollout_step(qkv, H, r, alpha).double(), want), (H, alpha)


@pytest.mark.parametrize("S", [1, 3, 65, 199])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_permutation_attention_bit_for_bit(S, hd):
    """Every query one-hot on a known key: out is that scatter of r, exactly."""
    B, C = 2, 8
    for H in (1, 2):
        qkv, perm = MR.permutation_qkv(B, S, H, hd, seed=S + H)
        qkv = qkv.to(DEV)
        r = MR.dyadic_rows(B, C, S, seed=3).to(DEV)
        for alpha in (0.0, 0.5):
            want = MR.permutation_step(r, perm, alpha)
            assert torch.equal(_ref_step(qkv, H, r.double(), alpha), want)
            assert torch.equal(AM.rollout_step(qkv, H, r, alpha).double(), want), (H, alpha)


@pytest.mark.parametrize("H", [1, 3])
def test_big_logits_over_four_key_tiles(H):
    """Logits near 2000 whose running maximum moves in each of the four key tiles."""
    B, S, C = 2, 199, 3
    qkv = AR.big_logits_qkv(B, S, H, 64).to(DEV)
    r = _rows(B, C, S, seed=7).to(DEV)
    ref = _ref_step(qkv, H, r.double(), 0.5)
    assert float(torch.einsum("bqd,bkd->bqk", qkv[..., :64].double(), qkv[..., 64 * H:64 * H + 64].double()).max()) / 8 >= 1984
    _check(f"big logits H={H}", AM.rollout_step(qkv, H, r, 0.5), AM.rollout_step_torch(qkv, H, r, 0.5, torch.float32), ref)


def test_rollout_of_four_layers():
    B, S, H, hd, n_cls = 2, 199, 3, 64, 3
    qkvs = [AR.random_qkv(B, S, H, hd, seed=20 + i, gain=1.5).to(DEV) for i in range(4)]
    ref = torch.eye(S, dtype=torch.float64, device=DEV)[:n_cls].expand(B, n_cls, S)
    for x in reversed(qkvs):
        ref = _ref_step(x, H, ref, 0.5)
    calls = []
    real = _ext().attn_rollout_step
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_ext(), "attn_rollout_step", lambda *a: calls.append(1) or real(*a))
        got = AM.rollout(qkvs, H, n_cls, 0.5)
        assert calls == [1] * 4
        mp.setattr(P, "_ATTN_MAPS_OURS", False)
        comp = AM.rollout(qkvs, H, n_cls, 0.5)
        assert calls == [1] * 4
    _check("rollout L=4", got, comp, ref)
    assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-5
    last = AM.rollout(qkvs, H, n_cls, 0.5, mode="last")
    r0 = torch.eye(S, device=DEV)[:n_cls].expand(B, n_cls, S).contiguous()
    _check("last", last, AM.rollout_step_torch(qkvs[-1], H, r0, 0.0, torch.float32), _ref_step(qkvs[-1], H, r0.double(), 0.0))


@pytest.mark.parametrize("S,hd,C", [(65, 80, 3), (199, 128, 8)])
def test_reruns_are_bit_identical(S, hd, C):
    qkv = AR.random_qkv(2, S, 3, hd, seed=4).to(DEV)
    r = _rows(2, C, S, seed=1).to(DEV)
    first = AM.rollout_step(qkv, 3, r, 0.5)
    for _ in range(3):
        assert torch.equal(AM.rollout_step(qkv, 3, r, 0.5), first)


@pytest.mark.parametrize("S,hd,C", [(65, 80, 3), (199, 32, 8), (1, 128, 1)])
def test_poisoned_surroundings(S, hd, C):
    B, H, pad = 2, 2, 4096
    qkv = AR.random_qkv(B, S, H, hd, seed=5)
    r = _rows(B, C, S, seed=2)
    n, nr = qkv.numel(), r.numel()
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[pad:pad + n] = qkv.reshape(-1).to(DEV)
    rbuf = torch.full((nr + 2 * pad,), float("nan"), device=DEV)
    rbuf[pad:pad + nr] = r.reshape(-1).to(DEV)
    obuf = torch.full((nr + 2 * pad,), float("nan"), device=DEV)
    out = obuf[pad:pad + nr].view(B, C, S)
    ret = _ext().attn_rollout_step(buf[pad:pad + n].view(B, S, -1), H, rbuf[pad:pad + nr].view(B, C, S), 0.5, out)
    assert ret.data_ptr() == out.data_ptr()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, AM.rollout_step(qkv.to(DEV), H, r.to(DEV), 0.5))
    for b in (buf, rbuf, obuf):
        assert bool(torch.isnan(b[:pad]).all()) and bool(torch.isnan(b[-pad:]).all())
    assert torch.equal(buf[pad:pad + n].cpu(), qkv.reshape(-1)) and torch.equal(rbuf[pad:pad + nr].cpu(), r.reshape(-1))


@pytest.mark.parametrize("B,S,H,hd", [(2, 65, 2, 64), (2, 199, 3, 80)])
def test_nan_rules(B, S, H, hd):
    qkv = AR.random_qkv(B, S, H, hd, seed=9).view(B, S, 3, H, hd)
    r = _rows(B, 3, S, seed=3).to(DEV)
    clean = AM.rollout_step(qkv.reshape(B, S, -1).to(DEV), H, r, 0.5)
    for which, row, col in ((0, S - 2, hd - 1), (1, S - 2, 0), (0, 0, 0), (1, 0, hd - 1)):  # q rows, k rows
        x = qkv.clone()
        x[0, row, which, H - 1, col] = float("nan")
        got = AM.rollout_step(x.reshape(B, S, -1).to(DEV), H, r, 0.5)
        assert bool(torch.isnan(got[0]).all()), (which, row)
        assert torch.equal(got[1], clean[1]), (which, row)
        comp = AM.rollout_step_torch(x.reshape(B, S, -1).to(DEV), H, r, 0.5)
        assert torch.equal(torch.isnan(comp), torch.isnan(got))
    x = qkv.clone()
    x[:, :, 2] = float("nan")  # v is not read
    assert torch.equal(AM.rollout_step(x.reshape(B, S, -1).to(DEV), H, r, 0.5), clean)
    # +-inf in ONE column of a key against queries that are positive in that column: that key's logits in head 0 are
    # +-inf, every other logit keeps its ordinary size.  +inf: the NaN rule; -inf: p = 0 at that key of that head
    for value, bad in ((float("inf"), True), (float("-inf"), False)):
        x = qkv.clone()
        x[0, :, 0, 0, 0] = x[0, :, 0, 0, 0].abs() + 1
        x[0, 2, 1, 0, 0] = value
        xd = x.reshape(B, S, -1).to(DEV)
        got = AM.rollout_step(xd, H, r, 0.5)
        assert torch.equal(got[1], clean[1])
        if bad:
            assert bool(torch.isnan(got[0]).all())
        else:
            _check(f"-inf key S={S}", got, AM.rollout_step_torch(xd, H, r, 0.5), _ref_step(xd, H, r.double(), 0.5))


def test_routing(monkeypatch):
    qkv = AR.random_qkv(2, 52, 2, 64, seed=2).to(DEV)
    r = _rows(2, 3, 52, seed=0).to(DEV)
    calls = []
    ext = _ext()
    real = ext.attn_rollout_step
    monkeypatch.setattr(ext, "attn_rollout_step", lambda *a: calls.append(1) or real(*a))
    got = AM.rollout_step(qkv, 2, r, 0.5)
    assert calls == [1] and got.shape == r.shape
    x88 = AR.random_qkv(2, 52, 2, 88, seed=2).to(DEV)
    r9 = _rows(2, 9, 52, seed=0).to(DEV)
    for x, rows in ((qkv.float(), r), (x88, r), (qkv, r9)):  # fp32 input; head dim 88; C = 9
        assert torch.equal(AM.rollout_step(x, 2, rows, 0.5), AM.rollout_step_torch(x, 2, rows, 0.5, torch.float32))
        assert calls == [1]
    monkeypatch.setattr(P, "_ATTN_MAPS_OURS", False)
    assert torch.equal(AM.rollout_step(qkv, 2, r, 0.5), AM.rollout_step_torch(qkv, 2, r, 0.5)) and calls == [1]
    monkeypatch.setattr(P, "_ATTN_MAPS_OURS", True)
    assert AM.rollout_step(qkv[:0], 2, r[:0], 0.5).shape == (0, 3, 52) and calls == [1]
    # bad arguments raise before any launch
    for bad in (lambda: AM.rollout_step(qkv[0], 2, r, 0.5), lambda: AM.rollout_step(qkv, 5, r, 0.5),
                lambda: AM.rollout_step(qkv, 2, r[:, :, :51], 0.5), lambda: AM.rollout_step(qkv, 2, r[:1], 0.5),
                lambda: AM.rollout_step(qkv, 2, r.double().bfloat16(), 0.5), lambda: AM.rollout_step(qkv, 2, r.cpu(), 0.5),
                lambda: AM.rollout_step(qkv, 2, r, 1.01), lambda: AM.rollout_step(qkv, 2, r, float("nan"))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: real(qkv[0], 2, r, 0.5), lambda: real(qkv, 5, r, 0.5), lambda: real(qkv.float(), 2, r, 0.5),
                lambda: real(qkv, 2, r9, 0.5), lambda: real(qkv, 2, r[:, :, :51], 0.5), lambda: real(qkv, 2, r.double(), 0.5),
                lambda: real(qkv, 2, r, -0.5), lambda: real(qkv, 2, r, 0.5, r), lambda: real(x88, 2, r, 0.5),
                lambda: real(qkv, 2, r, 0.5, torch.empty(2, 3, 51, device=DEV))):
        with pytest.raises(RuntimeError):
            bad()
    assert calls == [1]


DEBUG_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
import attn_stats_ref as AR
from jumbo_mae_tpu_amd.ops import _ext, attn_maps as AM
assert _ext.variant() == "debug"
for B, S, H, hd, C in ((2, 65, 2, 80, 3), (1, 199, 2, 64, 8), (2, 3, 1, 128, 1)):
    qkv = AR.random_qkv(B, S, H, hd, seed=1).cuda()
    r = torch.rand(B, C, S, generator=torch.Generator().manual_seed(0)).cuda()
    got = AM.rollout_step(qkv, H, r, 0.5)
    want = AM.rollout_step_torch(qkv, H, r, 0.5, torch.float64)
    assert float((got.double() - want).abs().max()) <= 1e-5
lines = _ext.load().debug_lines()
assert not lines, dict(lines)
print("debug ok")
"""


def test_debug_build_check_does_not_fire():
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD.format(tests=tests)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "debug ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ models
def test_models_against_the_composition(monkeypatch):
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.models.mae import PretrainModel

    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (4, 3, 64, 64), dtype=torch.uint8, generator=g).to(DEV)
    vc = ViTConfig(layers=2, dim=128, heads=2, labels=0, image_size=64, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75)
    dc = DecoderConfig(dec_layers=2, dec_dim=64, dec_heads=2, image_size=64, patch_size=16)
    pm = PretrainModel(vc, dc).to(DEV, torch.bfloat16, seed=0)
    fm = FinetuneModel(ViTConfig(layers=2, dim=128, heads=2, labels=10, image_size=64, patch_size=16,
                                 posemb="learnable")).to(DEV, torch.bfloat16, seed=0)
    calls = []
    real = _ext().attn_rollout_step
    monkeypatch.setattr(_ext(), "attn_rollout_step", lambda *a: calls.append(1) or real(*a))
    for name, m in (("pretrain", pm), ("finetune", fm)):
        if name == "finetune":
            rows, _ = m.patches(x, None, None, True, plan=None)
            qkvs = AM.collect_layers(lambda: m.features(rows, 4, None, True), 2)
        else:
            qkvs = AM.collect_layers(lambda: m.features(x), 2)
        assert all(t.shape == (4, 19, 384) and t.dtype == torch.bfloat16 for t in qkvs)  # unmasked: 3 CLS + 16 patches
        for mode in AM.MODES:
            del calls[:]
            ours = m.attention_maps(x, mode=mode)
            assert calls == [1] * (2 if mode == "rollout" else 1)
            monkeypatch.setattr(P, "_ATTN_MAPS_OURS", False)
            comp = m.attention_maps(x, mode=mode)
            monkeypatch.setattr(P, "_ATTN_MAPS_OURS", True)
            assert len(calls) == (2 if mode == "rollout" else 1)
            assert ours["maps"].shape == (4, 3, 4, 4) and ours["cls_mass"].shape == (4, 3)
            ref = torch.eye(19, dtype=torch.float64, device=DEV)[:3].expand(4, 3, 19)
            for qkv, alpha in ([(qkvs[1], 0.0)] if mode == "last" else [(qkvs[1], 0.5), (qkvs[0], 0.5)]):
                ref = _ref_step(qkv, 2, ref, alpha)
            _check(f"{name} {mode} maps", ours["maps"].flatten(2), comp["maps"].flatten(2), ref[:, :, 3:])
            _check(f"{name} {mode} cls_mass", ours["cls_mass"], comp["cls_mass"], ref[:, :, :3].sum(-1))
            total = ours["maps"].double().sum((2, 3)) + ours["cls_mass"].double()
            assert float((total - 1).abs().max()) <= 1e-5


def test_probe_between_graph_replays_leaves_the_eager_bits():
    """Trainer level, where a HIP-graph run is bit-identical to the eager one (tests/test_ema_gpu.py): a probe pass
    between replays changes neither the replayed steps nor what the graph holds."""
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.runtime.graph import StepRunner
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    g = torch.Generator().manual_seed(0)
    data = [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=g).to(DEV),
             torch.randint(0, 10, (8,), generator=g).to(DEV)) for _ in range(3)]
    runs = []
    for graph, probe in ((False, False), (True, False), (True, True)):
        vc = ViTConfig(layers=2, dim=64, heads=2, labels=10, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.0)
        m = FinetuneModel(vc).to(DEV, torch.bfloat16, seed=0)
        opt = FlatOptimizer(m.store, "adamw", lambda c: 1e-3, weight_decay=0.05, num_layers=2)
        tr = Trainer(m, opt, None, RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, DEV))
        step = StepRunner(tr, hip_graph=True) if graph else (lambda micro, tr=tr: tr.train_step(micro))
        maps = []
        for b in data:
            step([b])
            if probe:
                maps.append(m.attention_maps(b[0])["maps"])
        torch.cuda.synchronize()
        runs.append((m, step, maps))
    (m1, _, _), (m0, _, _), (m2, run, maps) = runs
    assert run.graphed is not None and run.graphed.replays == 3
    assert torch.equal(m0.store.master.view(torch.int32), m2.store.master.view(torch.int32))  # graph, no probe
    assert torch.equal(m1.store.master.view(torch.int32), m2.store.master.view(torch.int32))  # eager
    assert len(maps) == 3 and all(t.shape == (8, 3, 2, 2) and bool(torch.isfinite(t).all()) for t in maps)
    assert AM._COLLECTOR is None
