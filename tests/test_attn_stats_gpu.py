"""The attention monitor's kernel (csrc/attn_stats.hip) against the exact reference of tests/attn_stats_ref.py.

Shapes: S in {1, 3, 52, 64, 65, 199, 259} (a single key, CLS only, the encoder shape, an exact tile, one row
over a tile, the decoder shape, five query tiles with a 3-row remainder), head dims 32 / 64 / 80 / 96 / 128,
B and H in 1..3, n_cls in {0, 3, S}.

Bounds, per row (``rows_out``) against the fp64 reference: PMAX, CLS, ZMAX within max(2 x the error of the fp32
torch composition on that row, 1 fp32 ulp); ENT within max(2 x the fp32 composition's error,
2^-22 (1 + max_k |z|)).  The [H, 6] table against the ``math.fsum`` of the kernel's own row values: columns 0-2
within n 2^-53 S* (n = B S rows, S* the sum of magnitudes), the rest exact, reruns bit-identical.  The worst
measured error / bound ratio per head dim is printed (profiles/attn_stats.txt records one run)."""

import math
import os
import subprocess
import sys

import pytest
import torch

import attn_stats_ref as AR

from jumbo_mae_tpu_amd.ops import attn_stats as AS
from jumbo_mae_tpu_amd.ops import prims as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, S, H, hd, n_cls): every S, every head dim, n_cls in {0, 3, S}
CASES = [(3, 1, 2, 64, 0), (2, 1, 3, 80, 1), (2, 3, 3, 32, 3), (1, 3, 2, 128, 0), (2, 52, 3, 64, 3),
         (1, 52, 2, 80, 52), (2, 64, 2, 96, 3), (1, 64, 3, 32, 0), (3, 65, 1, 128, 3), (1, 65, 2, 64, 65),
         (2, 199, 2, 32, 3), (1, 199, 1, 80, 0), (1, 199, 2, 128, 3), (1, 259, 3, 80, 3), (2, 259, 1, 64, 259),
         (1, 259, 2, 96, 0), (1, 259, 1, 128, 3), (1, 259, 2, 32, 3)]


def _run(qkv, H, n_cls):
    B, S, _ = qkv.shape
    rows = torch.full((B, H, S, 4), float("nan"), device=DEV)
    tab = AS.attn_stats(qkv.to(DEV), H, n_cls, rows_out=rows)
    return tab.cpu(), rows.cpu()


def _check_table(tab, rows, B, S):
    want, mags = AR.ref_table(rows)
    assert torch.equal(tab[:, 3:], want[:, 3:]), (tab[:, 3:], want[:, 3:])
    err = (tab[:, :3] - want[:, :3]).abs()
    assert bool((err <= B * S * AR.U53 * mags).all()), (err, mags)


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for hd in sorted(w):
        print(f"\nattn_stats hd {hd}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in w[hd].items()))


_RANDOM = {}


def _random_case(case):
    """(tab, rows, error / bound ratio [B, H, S, 4]) of a case, computed once for the tests that share it."""
    if case not in _RANDOM:
        B, S, H, hd, n_cls = case
        qkv = AR.random_qkv(B, S, H, hd, seed=S + hd)
        ref, zabs = AR.ref_rows(qkv, H, n_cls)
        ref, zabs = torch.from_numpy(ref), torch.from_numpy(zabs)
        c32 = AS.attn_rows_torch(qkv.to(DEV), H, n_cls, torch.float32).cpu().double()
        tab, rows = _run(qkv, H, n_cls)
        comp = 2.0 * (c32 - ref).abs()
        bound = torch.maximum(comp, AR.ulp32(ref))
        bound[..., 0] = torch.maximum(comp[..., 0], 2.0 ** -22 * (1.0 + zabs))
        ratio = (rows.double() - ref).abs() / bound
        print(f"B {B} S {S} H {H} hd {hd} n_cls {n_cls}: worst error / bound " +
              " ".join(f"{n} {float(ratio[..., j].max()):.3f}" for j, n in enumerate(("ENT", "PMAX", "CLS", "ZMAX"))))
        _RANDOM[case] = (qkv, tab, rows, ratio)
    return _RANDOM[case]


@pytest.mark.parametrize("B,S,H,hd,n_cls", CASES)
def test_random_rows_entropy_and_table(worst, B, S, H, hd, n_cls):
    qkv, tab, rows, ratio = _random_case((B, S, H, hd, n_cls))
    assert bool(torch.isfinite(rows).all())
    w = worst.setdefault(hd, {"ENT": 0.0, "PMAX": 0.0, "CLS": 0.0, "ZMAX": 0.0})
    for j, name in enumerate(w):
        w[name] = max(w[name], float(ratio[..., j].max()))
    assert bool((ratio[..., 0] <= 1.0).all()), float(ratio[..., 0].max())
    if n_cls == 0:
        assert not bool(rows[..., 2].any())
    _check_table(tab, rows, B, S)
    assert tab[:, 4].tolist() == [0.0] * H and tab[:, 5].tolist() == [float(B * S)] * H
    tab2, rows2 = _run(qkv, H, n_cls)  # reruns are bit-identical
    assert torch.equal(tab2.view(torch.int64), tab.view(torch.int64)) and torch.equal(rows2.view(torch.int32), rows.view(torch.int32))


@pytest.mark.parametrize("B,S,H,hd,n_cls", CASES)
def test_random_rows_pmax_cls_zmax(B, S, H, hd, n_cls):
    """The logits are exact (fp64 MFMA on the widened bf16 values) and the row sums fp64, so each value is the
    exact one rounded to fp32 once: well inside the 1-ulp floor whatever the fp32 composition does on the row."""
    _, _, rows, ratio = _random_case((B, S, H, hd, n_cls))
    assert bool((ratio[..., 1:] <= 1.0).all()), [float(ratio[..., j].max()) for j in (1, 2, 3)]


@pytest.mark.parametrize("B,S,H,n_cls", [(2, 1, 2, 1), (2, 3, 3, 3), (3, 52, 2, 3), (1, 64, 3, 0), (2, 65, 2, 65),
                                         (1, 199, 3, 3), (2, 259, 2, 3)])
def test_exactly_summable_inputs(B, S, H, n_cls):
    qkv = AR.exact_qkv(B, S, H, 64, seed=S)
    ref, _ = AR.ref_rows(qkv, H, n_cls)
    tab, rows = _run(qkv, H, n_cls)
    zmax = torch.from_numpy(ref[..., 3])
    assert torch.equal(rows[..., 3].double(), zmax)  # multiples of 1/8: exact
    assert torch.equal(tab[:, 3], zmax.amax((0, 2)))
    assert tab[:, 4].tolist() == [0.0] * H and tab[:, 5].tolist() == [float(B * S)] * H
    _check_table(tab, rows, B, S)


def _row_bound(ref, zabs):
    b = AR.ulp32(ref)
    b[..., 0] = 2.0 ** -22 * (1.0 + zabs)
    return b


@pytest.mark.parametrize("S,n_cls", [(1, 1), (3, 3), (52, 3), (64, 0), (65, 3), (199, 199), (259, 3)])
def test_structural_cases(S, n_cls):
    B, H = 2, 2
    _, rows = _run(AR.equal_keys_qkv(B, S, H, 64, seed=S), H, n_cls)
    want = torch.tensor([math.log(S), 1.0 / S, n_cls / S], dtype=torch.float64).expand(B, H, S, 3)
    z = AR.logits(AR.equal_keys_qkv(B, S, H, 64, seed=S), H)
    bound = _row_bound(torch.cat([want, want[..., :1]], -1).clone(), torch.from_numpy(abs(z).max(-1)))
    assert bool(((rows[..., :3].double() - want).abs() <= bound[..., :3]).all())
    for key in {0, S // 2, S - 1}:
        _, rows = _run(AR.one_ahead_qkv(B, S, H, 64, key=key), H, n_cls)
        if S > 1:
            assert bool((rows[..., 0].abs() <= 2.0 ** -22 * 257).all()) and bool((rows[..., 1] == 1.0).all())
            assert bool((rows[..., 2] == (1.0 if key < n_cls else 0.0)).all()) and bool((rows[..., 3] == 256.0).all())


@pytest.mark.parametrize("S", [65, 199, 259])
def test_big_logits_rescale(S):
    qkv = AR.big_logits_qkv(2, S, 2, 64)
    ref, zabs = AR.ref_rows(qkv, 2, 3)
    ref, zabs = torch.from_numpy(ref), torch.from_numpy(zabs)
    tab, rows = _run(qkv, 2, 3)
    assert float(zabs.max()) >= 1984.0
    assert bool(torch.isfinite(rows).all()) and bool((rows[..., 0] >= 0).all())
    assert torch.equal(rows[..., 3].double(), ref[..., 3])
    assert bool(((rows.double() - ref).abs() <= _row_bound(ref, zabs)).all())
    _check_table(tab, rows, 2, S)


def test_poisoned_surroundings():
    B, S, H, hd, n_cls = 2, 65, 2, 80, 3
    qkv = AR.random_qkv(B, S, H, hd, seed=5)
    n, pad = qkv.numel(), 4096
    buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[pad:pad + n] = qkv.reshape(-1).to(DEV)
    view = buf[pad:pad + n].view(B, S, -1)
    out = torch.full((B * H * S * 4 + 2 * pad,), float("nan"), device=DEV)
    rows = out[pad:pad + B * H * S * 4].view(B, H, S, 4)
    tab = AS.attn_stats(view, H, n_cls, rows_out=rows)
    want_tab, want_rows = _run(qkv, H, n_cls)
    assert bool(torch.isfinite(tab).all()) and torch.equal(tab.cpu(), want_tab) and torch.equal(rows.cpu(), want_rows)
    assert bool(torch.isnan(out[:pad]).all()) and bool(torch.isnan(out[-pad:]).all())
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())
    assert torch.equal(buf[pad:pad + n].cpu(), qkv.reshape(-1))


@pytest.mark.parametrize("B,S,H,hd", [(2, 65, 2, 64), (1, 199, 3, 80)])
def test_nonfinite_values(B, S, H, hd):
    qkv = AR.random_qkv(B, S, H, hd, seed=9).view(B, S, 3, H, hd)
    clean_tab, clean_rows = _run(qkv.reshape(B, S, -1), H, 3)
    b, h, r = B - 1, H - 1, S - 2
    x = qkv.clone()
    x[b, r, 0, h, hd - 1] = float("nan")  # one q row
    tab, rows = _run(x.reshape(B, S, -1), H, 3)
    bad = torch.isnan(rows[..., 0])
    assert int(bad.sum()) == 1 and bool(bad[b, h, r]) and tab[:, 4].tolist() == [0.0] * (H - 1) + [1.0]
    assert torch.equal(rows[~bad], clean_rows[~bad]) and torch.equal(tab[:h], clean_tab[:h])
    _check_table(tab, rows, B, S)
    x = qkv.clone()
    x[b, r, 1, h, 0] = float("nan")  # one k row
    tab, rows = _run(x.reshape(B, S, -1), H, 3)
    bad = torch.isnan(rows[..., 0])
    assert int(bad.sum()) == S and bool(bad[b, h].all()) and tab[:, 4].tolist() == [0.0] * (H - 1) + [float(S)]
    assert torch.equal(rows[~bad], clean_rows[~bad]) and torch.equal(tab[:h], clean_tab[:h])
    _check_table(tab, rows, B, S)  # the sums over the remaining rows
    if B == 1:
        assert tab[h].tolist() == [0.0, 0.0, 0.0, float("-inf"), float(S), float(S)]


def test_routing(monkeypatch):
    qkv = AR.random_qkv(2, 52, 2, 64, seed=2).to(DEV)
    calls = []
    ext = AS._ext.load()
    real = ext.attn_stats
    monkeypatch.setattr(ext, "attn_stats", lambda *a: calls.append(1) or real(*a))
    AS.attn_stats(qkv, 2, 3)
    assert calls == [1]
    for x, heads in ((qkv.float(), 2), (AR.random_qkv(2, 52, 2, 48, seed=2).to(DEV), 2)):  # fp32; head dim 48
        rows = torch.empty(2, heads, 52, 4, device=DEV)
        tab = AS.attn_stats(x, heads, 3, rows_out=rows)
        assert calls == [1]
        assert torch.equal(rows, AS.attn_rows_torch(x, heads, 3, torch.float32))
        assert torch.equal(tab, AS.attn_stats_torch(x, heads, 3, torch.float32))
    monkeypatch.setattr(P, "_ATTN_STATS_OURS", False)
    assert torch.equal(AS.attn_stats(qkv, 2, 3), AS.attn_stats_torch(qkv, 2, 3)) and calls == [1]
    monkeypatch.setattr(P, "_ATTN_STATS_OURS", True)
    for bad in (lambda: AS.attn_stats(qkv[0], 2, 3), lambda: AS.attn_stats(qkv, 5, 3), lambda: AS.attn_stats(qkv, 2, 53),
                lambda: AS.attn_stats(qkv, 2, 3, rows_out=torch.empty(2, 2, 52, 3, device=DEV)),
                lambda: AS.attn_stats(qkv, 2, 3, rows_out=torch.empty(2, 2, 52, 4, device=DEV, dtype=torch.float64))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: real(qkv[0], 2, 3, None), lambda: real(qkv, 5, 3, None), lambda: real(qkv, 2, 53, None),
                lambda: real(qkv, 2, 3, torch.empty(2, 2, 52, 3, device=DEV)), lambda: real(qkv.float(), 2, 3, None),
                lambda: real(qkv, 2, 3, torch.empty(2, 2, 52, 4, device=DEV, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            bad()
    assert calls == [1]


DEBUG_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
import attn_stats_ref as AR
from jumbo_mae_tpu_amd.ops import _ext, attn_stats as AS
assert _ext.variant() == "debug"
for B, S, H, hd in ((2, 65, 2, 80), (1, 259, 2, 64), (2, 3, 1, 128)):
    qkv = AR.random_qkv(B, S, H, hd, seed=1)
    tab = AS.attn_stats(qkv.cuda(), H, min(3, S))
    assert torch.equal(tab[:, 4:].cpu(), torch.tensor([[0.0, B * S]] * H, dtype=torch.float64))
    assert bool(torch.isfinite(tab).all())
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


# ------------------------------------------------------------------ models and drivers
def _assert_tables(got, want):
    """Tables of the kernel against those of the fp32 composition on the same qkv: both are within the row bounds
    of the exact values, so the per-row means differ by at most twice the largest row bound (|z| <= 64 assumed and
    checked), maxima by 2 ulp, counts not at all."""
    assert list(got) == list(want)
    for k in got:
        a, b = got[k].cpu(), want[k].cpu()
        assert torch.equal(a[:, 4:], b[:, 4:]) and bool((a[:, 4] == 0).all()), k
        zm = float(torch.maximum(a[:, 3].abs(), b[:, 3].abs()).max())
        assert zm <= 64.0
        n = a[:, 5:6]
        assert bool(((a[:, :3] - b[:, :3]).abs() / n <= 2 * 2.0 ** -22 * (1 + 64.0)).all()), (k, a, b)
        assert bool(((a[:, 3] - b[:, 3]).abs() <= 2 * AR.ulp32(b[:, 3])).all()), k


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
    noise = torch.rand(16, generator=g).to(DEV)
    ours = pm.attention_stats(x, noise=noise), fm.attention_stats(x)
    monkeypatch.setattr(P, "_ATTN_STATS_OURS", False)
    comp = pm.attention_stats(x, noise=noise), fm.attention_stats(x)
    assert list(ours[0]) == ["layer_0", "layer_1", "decoder/dec_layer_0", "decoder/dec_layer_1"]
    assert list(ours[1]) == ["layer_0", "layer_1"]
    _assert_tables(ours[0], comp[0])
    _assert_tables(ours[1], comp[1])
    assert ours[0]["layer_0"][0, 5] == 4 * 7 and ours[0]["decoder/dec_layer_0"][0, 5] == 4 * 19 and ours[1]["layer_1"][0, 5] == 4 * 19


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
        tabs = []
        for b in data:
            step([b])
            if graph:
                tabs.append(m.attention_stats(b[0]))
        torch.cuda.synchronize()
        runs.append((m, step, tabs))
    (m1, _, _), (m0, _, _), (m2, run, tabs) = runs
    assert run.graphed is not None and run.graphed.replays == 3
    assert torch.equal(m0.store.master.view(torch.int32), m2.store.master.view(torch.int32))  # graph, no probe
    assert torch.equal(m1.store.master.view(torch.int32), m2.store.master.view(torch.int32))  # eager
    assert len(tabs) == 3 and all(bool(torch.isfinite(t["layer_1"]).all()) for t in tabs)
    assert not torch.equal(tabs[0]["layer_1"], tabs[2]["layer_1"])


def _driver_runs(tmp_path, variants):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.train import finetune as FT
    from jumbo_mae_tpu_amd.train.cli import finetune_parser

    d = str(tmp_path)
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=1, per_shard=8, classes=4, seed=1, prefix="valid")
    base = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
            "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
            "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cuda",
            "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--learning-rate", "5e-3",
            "--training-steps", "4", "--warmup-steps", "1", "--log-interval", "2", "--eval-interval", "2",
            "--droppath", "0", "--mixup", "0", "--cutmix", "0", "--labels", "4", "--name", "f",
            "--train-dataset-shards", train, "--valid-dataset-shards", valid]
    blobs = {}
    for name, extra in variants:
        out = os.path.join(d, name)
        res = FT.main(finetune_parser().parse_args(base + ["--output-dir", out] + extra))
        with open(os.path.join(out, "f-last.msgpack"), "rb") as f:
            blobs[name] = f.read()
        if "--attn-stats" in extra:
            assert math.isfinite(res["val/attn_entropy_min"]) and "attn/entropy/layer_1" in res
    return blobs


def test_hip_graph_run_with_the_flag_ends_with_the_eager_weights(tmp_path):
    """The driver's deterministic configuration (no Mixup / CutMix, no droppath: device random draws differ between a
    captured and an eager step, tests/test_graph_gpu.py), where a --hip-graph run gives the eager run's bits."""
    blobs = _driver_runs(tmp_path, (("graph_flag", ["--hip-graph", "--attn-stats", "4"]), ("graph", ["--hip-graph"]),
                                    ("eager_flag", ["--attn-stats", "4"]), ("eager", [])))
    assert blobs["graph_flag"] == blobs["graph"] and blobs["eager_flag"] == blobs["eager"]
    assert blobs["graph_flag"] == blobs["eager"]
