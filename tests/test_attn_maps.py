"""Attention maps (ops/attn_maps.py) without a GPU: the torch composition against the plain loops of
tests/attn_maps_ref.py, the exactly summable cases, conservation of the row sums, ``rollout`` against the
explicit matrix product, ``mode="last"``, the NaN rule, argument errors, the collector on both forward paths
beside the attention monitor's, both model methods, both drivers with and without ``--attn-maps 2``
(identical checkpoints and log values, the new keys, the PNG) and the tool on a checkpoint."""

import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_maps_ref as MR
import attn_stats_ref as AR

from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import attn_maps as AM
from jumbo_mae_tpu_amd.ops import attn_stats as AS
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.train import common as C
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser


def test_switch():
    assert P._ATTN_MAPS_OURS is True and AM.MAX_ROWS == 8


def _rows(B, C, S, seed=0):
    r = torch.rand(B, C, S, generator=torch.Generator().manual_seed(seed))
    r[:, 0] = 0.0
    r[:, 0, min(1, S - 1)] = 1.0  # a one-hot row
    return r


# ------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("B,S,H,hd,C,alpha", [(1, 1, 1, 8, 1, 0.5), (2, 3, 2, 8, 3, 0.5), (2, 7, 3, 16, 2, 0.0),
                                               (1, 19, 2, 48, 9, 0.25), (1, 19, 2, 48, 3, 1.0)])
def test_composition_against_loops(B, S, H, hd, C, alpha):
    qkv = AR.random_qkv(B, S, H, hd, seed=S, gain=2.0)
    r = _rows(B, C, S, seed=C)
    ref = torch.from_numpy(MR.ref_step(qkv, H, r, alpha))
    got = AM.rollout_step_torch(qkv, H, r, alpha, torch.float64)
    assert got.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-13
    for x in (qkv, qkv.float()):  # bf16 and fp32 input
        got = AM.rollout_step_torch(x, H, r, alpha, torch.float32)
        assert got.dtype == torch.float32 and float((got.double() - ref).abs().max()) <= 2e-6
    assert torch.equal(AM.rollout_step(qkv, H, r, alpha), got)  # the CPU path is the fp32 composition
    # every row keeps its sum
    assert float((got.double().sum(-1) - r.double().sum(-1)).abs().max()) <= 1e-5
    assert float((AM.rollout_step_torch(qkv, H, r, alpha, torch.float64).sum(-1) - r.double().sum(-1)).abs().max()) <= 1e-13


@pytest.mark.parametrize("S", [1, 4, 64])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_uniform_attention_is_exact(S, alpha):
    B, H, C = 2, 2, 3
    r = MR.dyadic_rows(B, C, S, seed=S)
    got = AM.rollout_step_torch(MR.zero_query_qkv(B, S, H, 16), H, r, alpha, torch.float64)
    want = alpha * r.double() + (1.0 - alpha) * r.double().mean(-1, keepdim=True)
    assert torch.equal(got, want.expand_as(got))


@pytest.mark.parametrize("S,H,hd", [(1, 1, 8), (5, 2, 16), (70, 2, 32)])
def test_permutation_attention_is_exact(S, H, hd):
    B, C, alpha = 2, 3, 0.5
    qkv, perm = MR.permutation_qkv(B, S, H, hd, seed=S)
    r = MR.dyadic_rows(B, C, S, seed=1)
    want = MR.permutation_step(r, perm, alpha)
    assert torch.equal(AM.rollout_step_torch(qkv, H, r, alpha, torch.float64), want)
    assert torch.equal(AM.rollout_step_torch(qkv, H, r, alpha, torch.float32), want.float())
    if S <= 5:
        assert np.array_equal(MR.ref_step(qkv, H, r, alpha), want.numpy())


def test_rollout_is_the_matrix_product():
    B, S, H, hd, n_cls, alpha = 2, 9, 2, 16, 3, 0.5
    qkvs = [AR.random_qkv(B, S, H, hd, seed=10 + i, gain=1.5) for i in range(3)]
    prod = np.eye(S)[None].repeat(B, 0)
    for x in reversed(qkvs):  # row c of A_L ... A_1
        prod = prod @ MR.mean_matrix(x, H, alpha)
    got = AM.rollout(qkvs, H, n_cls, alpha)
    assert got.shape == (B, n_cls, S) and got.dtype == torch.float32
    assert float((got.double() - torch.from_numpy(prod[:, :n_cls])).abs().max()) <= 2e-6
    assert float((got.double().sum(-1) - 1).abs().max()) <= 1e-5
    maps = AM.patch_maps(got, n_cls, 2, 3)
    assert maps.shape == (B, n_cls, 2, 3) and torch.equal(maps.flatten(2), got[:, :, n_cls:])
    # mode "last": the head-mean attention of the CLS rows in the last layer
    last = AM.rollout(qkvs, H, n_cls, alpha, mode="last")
    want = torch.from_numpy(MR.ref_probs(qkvs[-1], H).mean(1)[:, :n_cls])
    assert float((last.double() - want).abs().max()) <= 2e-6
    assert torch.equal(last, AM.rollout(qkvs[-1:], H, n_cls, 0.0))
    out = AM.maps_and_mass(qkvs, H, n_cls, 2, 3, alpha)
    assert torch.equal(out["maps"], maps) and torch.equal(out["cls_mass"], got[:, :, :n_cls].sum(-1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nan_rule(dtype):
    B, S, H, hd, C = 2, 6, 2, 8, 3
    base = AR.random_qkv(B, S, H, hd, seed=1).view(B, S, 3, H, hd)
    r = _rows(B, C, S)
    clean = AM.rollout_step_torch(base.reshape(B, S, -1), H, r, 0.5, dtype)

    def run(edit):
        x = base.clone()
        edit(x)
        x = x.reshape(B, S, -1)
        got = AM.rollout_step_torch(x, H, r, 0.5, dtype)
        assert np.array_equal(np.isnan(MR.ref_step(x, H, r, 0.5)), torch.isnan(got).numpy())
        return got

    for edit in (lambda x: x[0, 4, 0, 1, 3].fill_(float("nan")),  # a NaN in one q row
                 lambda x: x[0, 2, 1, 0, 0].fill_(float("nan"))):  # a NaN in one k row
        got = run(edit)
        assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], clean[1])

    def inf_key(value):
        def edit(x):
            x[0, :, 0, 0] = x[0, :, 0, 0].abs() + 1  # positive queries: the logit is value itself
            x[0, 2, 1, 0] = value
        return edit
    got = run(inf_key(float("inf")))
    assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], clean[1])
    got = run(inf_key(float("-inf")))  # p = 0 at that key of head 0
    assert bool(torch.isfinite(got).all()) and torch.equal(got[1], clean[1])
    # a NaN in v is not read
    x = base.clone()
    x[:, :, 2] = float("nan")
    assert torch.equal(AM.rollout_step_torch(x.reshape(B, S, -1), H, r, 0.5, dtype), clean)


def test_empty_and_bad_arguments():
    qkv = AR.random_qkv(1, 4, 2, 8)
    r = torch.zeros(1, 3, 4)
    assert AM.rollout_step(qkv[:0], 2, r[:0], 0.5).shape == (0, 3, 4)
    assert AM.rollout_step(qkv[:, :0], 2, r[:, :, :0], 0.5).shape == (1, 3, 0)
    for bad in (lambda: AM.rollout_step(qkv[0], 2, r, 0.5),  # rank
                lambda: AM.rollout_step(qkv, 5, r, 0.5),  # 3 D not divisible by the heads
                lambda: AM.rollout_step(qkv, 0, r, 0.5),
                lambda: AM.rollout_step(qkv, 2, r[0], 0.5),
                lambda: AM.rollout_step(qkv, 2, torch.zeros(1, 3, 5), 0.5),  # S
                lambda: AM.rollout_step(qkv, 2, torch.zeros(2, 3, 4), 0.5),  # B
                lambda: AM.rollout_step(qkv, 2, torch.zeros(1, 0, 4), 0.5),  # C = 0
                lambda: AM.rollout_step(qkv, 2, r.to(torch.bfloat16), 0.5),
                lambda: AM.rollout_step(qkv.to(torch.float16), 2, r, 0.5),
                lambda: AM.rollout_step(qkv, 2, r, -0.1),
                lambda: AM.rollout_step(qkv, 2, r, 1.5),
                lambda: AM.rollout_step(qkv, 2, r, float("nan")),
                lambda: AM.rollout([], 2, 3),
                lambda: AM.rollout([qkv], 2, 0),
                lambda: AM.rollout([qkv], 2, 5),  # n_cls > S
                lambda: AM.rollout([qkv], 2, 3, mode="first"),
                lambda: AM.rollout([qkv, qkv[:, :3]], 2, 3),
                lambda: AM.patch_maps(torch.zeros(1, 3, 7), 3, 2, 3)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ collector and models
def _finetune_model(labels=10):
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=labels, image_size=32, patch_size=16, posemb="learnable",
                   droppath=0.0)
    return FinetuneModel(vc).to("cpu", torch.float32, seed=0)


def _pretrain_model():
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=0, image_size=32, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75)
    dc = DecoderConfig(dec_layers=2, dec_dim=32, dec_heads=2, image_size=32, patch_size=16)
    return PretrainModel(vc, dc).to("cpu", torch.float32, seed=0)


def _images(n=4, seed=0):
    return torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_collector_beside_the_attention_monitor(monkeypatch):
    m, x = _finetune_model(), _images(seed=1)
    rows, _ = m.patches(x, None, None, True, plan=None)
    run = lambda: m.features(rows, 4, None, True)  # noqa: E731
    per_path = {}
    for per_op in ("0", "1"):
        monkeypatch.setenv("JMAE_PER_OP", per_op)
        ref = run()
        alone = AS.collect_layers(["layer_0", "layer_1"], run, 3)
        with torch.no_grad(), AS.collecting(3) as tabs, AM.collecting() as got:
            both = run()
        assert AM._COLLECTOR is None and AS._COLLECTOR is None
        assert torch.equal(both, ref)  # the forward is unchanged
        assert len(got) == 2 and got.heads == 2 and all(t.shape == (4, 7, 192) and not t.requires_grad for t in got)
        assert len(tabs) == 2 and all(torch.equal(a, b) for a, b in zip(tabs, alone.values()))
        assert torch.equal(AS.attn_stats(got[1], 2, 3), tabs[1])  # the collected tensor is that layer's qkv
        per_path[per_op] = got
        assert torch.equal(run(), ref) and AM._COLLECTOR is None  # outside the context nothing is collected
    for a, b in zip(per_path["0"], per_path["1"]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError):
        with AM.collecting():
            with AM.collecting():
                pass
    assert AM._COLLECTOR is None
    with pytest.raises(RuntimeError):  # a layer count that does not match
        AM.collect_layers(run, 3)
    assert AM._COLLECTOR is None


@pytest.mark.parametrize("kind", ["finetune", "pretrain"])
@pytest.mark.parametrize("mode", ["rollout", "last"])
def test_model_attention_maps(kind, mode):
    m = _finetune_model() if kind == "finetune" else _pretrain_model()
    x = _images(seed=2)
    before = m.store.master.clone()
    state = torch.random.get_rng_state()
    out = m.attention_maps(x, mode=mode)
    assert torch.equal(torch.random.get_rng_state(), state) and torch.equal(m.store.master, before)
    assert sorted(out) == ["cls_mass", "maps"]
    assert out["maps"].shape == (4, 3, 2, 2) and out["cls_mass"].shape == (4, 3)
    assert out["maps"].dtype == out["cls_mass"].dtype == torch.float32
    assert bool((out["maps"] > 0).all()) and bool((out["cls_mass"] > 0).all())
    total = out["maps"].double().sum((2, 3)) + out["cls_mass"].double()
    assert float((total - 1).abs().max()) <= 1e-5
    # against the definition on the qkv tensors of the unmasked det=True forward
    if kind == "finetune":
        rows, _ = m.patches(x, None, None, True, plan=None)
        got = AM.collect_layers(lambda: m.features(rows, 4, None, True), 2)
    else:
        got = AM.collect_layers(lambda: m.features(x), 2)
    assert all(t.shape == (4, 7, 192) for t in got)  # every patch: 3 CLS + 4
    r = torch.eye(7)[:3].expand(4, 3, 7)
    steps = [(got[1], 0.0)] if mode == "last" else [(got[1], 0.5), (got[0], 0.5)]
    for qkv, alpha in steps:
        r = torch.from_numpy(MR.ref_step(qkv, 2, r, alpha))
    assert float((out["maps"].double().flatten(2) - r[:, :, 3:]).abs().max()) <= 2e-6
    assert float((out["cls_mass"].double() - r[:, :, :3].sum(-1)).abs().max()) <= 2e-6
    assert torch.equal(m.attention_maps(x, mode=mode)["maps"], out["maps"])


def test_panel_and_values():
    img = _images(2, seed=3)
    maps = torch.rand(2, 3, 2, 2, generator=torch.Generator().manual_seed(0))
    maps[0, 0] = torch.tensor([[0.0, 0.0], [0.0, 2.0]])
    pil = C.attn_map_panel(img, maps)
    assert pil.size == (4 * 32, 2 * 32) and pil.mode == "RGB"
    a = np.asarray(pil)
    assert np.array_equal(a[:, :32], img.permute(0, 2, 3, 1).reshape(64, 32, 3).numpy())  # the originals
    ramp = C.attn_map_ramp()
    assert ramp.shape == (256, 3) and ramp.dtype == np.uint8 and ramp[0].tolist() == [0, 0, 0] and ramp[255].tolist() == [255] * 3
    assert bool((np.diff(ramp.astype(int).sum(1)) >= 0).all())  # brightness never falls
    src = img[0].permute(1, 2, 0).numpy().astype(float)
    assert np.array_equal(a[:16, 32:48], np.round(0.4 * src[:16, :16]).astype(np.uint8))  # map 0: black
    assert np.array_equal(a[16:32, 48:64], np.round(0.4 * src[16:, 16:] + 0.6 * 255).astype(np.uint8))  # its max: white
    assert np.array_equal(np.asarray(C.attn_map_panel(img, maps * 3.0)), a)  # each map is divided by its max
    vals = C.attn_map_values({"maps": torch.full((2, 3, 2, 2), 0.125), "cls_mass": torch.full((2, 3), 0.5)})
    assert vals["val/attn_map_entropy"] == pytest.approx(math.log(4)) and vals["val/attn_map_cls_mass"] == 0.5
    one = torch.zeros(1, 1, 2, 2)
    one[0, 0, 1, 1] = 0.3
    assert C.attn_map_values({"maps": one, "cls_mass": torch.zeros(1, 1)})["val/attn_map_entropy"] == 0.0


# ------------------------------------------------------------------ drivers
COMMON = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--learning-rate", "5e-3",
          "--training-steps", "4", "--warmup-steps", "1", "--log-interval", "2", "--eval-interval", "2",
          "--droppath", "0.1"]
FINETUNE = COMMON + ["--labels", "4", "--name", "f"]
PRETRAIN = COMMON + ["--auto-augment", "none", "--labels", "0", "--dec-layers", "1", "--dec-dim", "64", "--dec-heads", "2",
                     "--dec-droppath", "0.1", "--name", "p"]
FLAG = ["--attn-maps", "2"]
NEW = ("val/attn_map_entropy", "val/attn_map_cls_mass")
VOLATILE = ("perf/", "time")


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=1, per_shard=8, classes=4, seed=1, prefix="valid")
    return train, valid


def _args(which, shards, out, extra=()):
    parser, base = (finetune_parser, FINETUNE) if which == "f" else (pretrain_parser, PRETRAIN)
    return parser().parse_args(base + ["--train-dataset-shards", shards[0], "--valid-dataset-shards", shards[1],
                                       "--output-dir", out, *extra])


@pytest.fixture(scope="module")
def runs(shards, tmp_path_factory):
    outs = {}
    for which, main in (("f", FT.main), ("p", PT.main)):
        for name, extra in (("with", FLAG), ("without", [])):
            out = str(tmp_path_factory.mktemp(which + name))
            main(_args(which, shards, out, extra))
            outs[which, name] = out
    return outs


def _log(out, which):
    return [json.loads(line) for line in open(os.path.join(out, f"{which}-metrics.jsonl"))]


@pytest.mark.parametrize("which", ["f", "p"])
def test_driver_with_the_flag_changes_nothing_else(runs, which):
    a, b = runs[which, "with"], runs[which, "without"]
    with open(os.path.join(a, f"{which}-last.msgpack"), "rb") as fa, open(os.path.join(b, f"{which}-last.msgpack"), "rb") as fb:
        assert fa.read() == fb.read()
    ra, rb = _log(a, which), _log(b, which)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        common = [k for k in y if not k.startswith(VOLATILE) and "time" not in k and k != "config"]
        assert common and {k: x[k] for k in common} == {k: y[k] for k in common}
        assert set(x) - set(y) <= set(NEW), set(x) - set(y)
    assert not any(k in r for r in rb for k in NEW)
    assert not [f for f in os.listdir(b) if f.endswith(".png")]


@pytest.mark.parametrize("which", ["f", "p"])
def test_driver_logs_the_values_and_writes_the_panels(runs, which):
    from PIL import Image

    out = runs[which, "with"]
    evals = [r for r in _log(out, which) if "val/loss" in r]
    assert [r["step"] for r in evals] == [0, 2, 4]  # the sanity evaluation included
    for r in evals:
        assert 0 < r["val/attn_map_entropy"] <= math.log(4) + 1e-9  # a 2 x 2 patch grid
        assert 0 < r["val/attn_map_cls_mass"] < 1
        with Image.open(os.path.join(out, f"{which}-attn-{r['step']:07d}.png")) as im:
            assert im.size == ((1 + 3) * 32, 2 * 32) and im.mode == "RGB"  # original + 3 CLS tokens, 2 images
    assert sorted(f for f in os.listdir(out) if "-attn-" in f) == [f"{which}-attn-{s:07d}.png" for s in (0, 2, 4)]
    assert evals[0]["val/attn_map_entropy"] != evals[2]["val/attn_map_entropy"]  # the weights move


def test_flag_defaults():
    for parser in (pretrain_parser, finetune_parser):
        a = parser().parse_args([])
        assert a.attn_maps == 0 and a.attn_maps_mode == "rollout"
        a = parser().parse_args(["--attn-maps", "8", "--attn-maps-mode", "last"])
        assert a.attn_maps == 8 and a.attn_maps_mode == "last"
        with pytest.raises(SystemExit):
            parser().parse_args(["--attn-maps-mode", "first"])


# ------------------------------------------------------------------ tool
def test_attn_maps_tool(runs, shards, tmp_path, capsys):
    from PIL import Image

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("attn_maps_tool", os.path.join(root, "tools", "attn_maps.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for which, base in (("p", PRETRAIN), ("f", FINETUNE)):
        model = [a for a in base if a not in ("--name", which)]
        ckpt = os.path.join(runs[which, "with"], f"{which}-last.msgpack")
        png = str(tmp_path / f"{which}.png")
        out = tool.main(model + ["--valid-dataset-shards", shards[1], "--ckpt", ckpt, "--n", "2", "--out", png] +
                        (["--finetune"] if which == "f" else []))
        last = [r for r in _log(runs[which, "with"], which) if "val/loss" in r][-1]
        assert out["images"] == 2 and out["cls_tokens"] == 3 and out["grid"] == [2, 2] and out["size"] == [128, 64]
        # the checkpoint is the run's last state: the tool reproduces the last evaluation's values and panel
        for k, v in out["values"].items():
            assert v == pytest.approx(last[k], rel=1e-6), k
        with Image.open(png) as a, Image.open(os.path.join(runs[which, "with"], f"{which}-attn-0000004.png")) as b:
            assert np.array_equal(np.asarray(a), np.asarray(b))
        assert json.loads(capsys.readouterr().out.splitlines()[-1])["mode"] == "rollout"
        out = tool.main(model + ["--valid-dataset-shards", shards[1], "--ckpt", ckpt, "--n", "2", "--out", png,
                                 "--attn-maps-mode", "last"] + (["--finetune"] if which == "f" else []))
        assert out["mode"] == "last" and out["values"]["val/attn_map_entropy"] != last["val/attn_map_entropy"]
        capsys.readouterr()
