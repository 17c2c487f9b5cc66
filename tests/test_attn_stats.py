"""Attention monitor (ops/attn_stats.py) without a GPU: the torch composition against the exact reference of
tests/attn_stats_ref.py (brute-force loops, ``math.fsum``), the structural cases, ``n_cls`` at 0 and S, the
NaN / inf row rule, the collector on both forward paths, both model methods, both drivers with and without
``--attn-stats 4`` (identical checkpoints and log values, the new keys) and the tool on a checkpoint."""

import importlib.util
import json
import math
import os

import pytest
import torch

import attn_stats_ref as AR

from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import attn_stats as AS
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser


def test_switch_and_columns():
    assert P._ATTN_STATS_OURS is True and AS.COLS == AR.COLS


# ------------------------------------------------------------------ the torch composition
def _assert_rows(got: torch.Tensor, ref, tol):
    ref = torch.from_numpy(ref)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got.double()), nan)
    err = (got.double() - ref).abs()
    assert bool((err[~nan] <= tol).all()), float(err[~nan].max())


@pytest.mark.parametrize("B,S,H,hd,n_cls", [(1, 1, 1, 8, 1), (2, 3, 2, 8, 3), (2, 7, 3, 16, 0), (1, 19, 2, 48, 3),
                                            (1, 19, 2, 48, 19)])
def test_composition_against_loops(B, S, H, hd, n_cls):
    qkv = AR.random_qkv(B, S, H, hd, seed=S, gain=2.0)
    ref, _ = AR.ref_rows(qkv, H, n_cls)
    _assert_rows(AS.attn_rows_torch(qkv, H, n_cls, torch.float64), ref, 1e-12)
    _assert_rows(AS.attn_rows_torch(qkv, H, n_cls, torch.float32), ref, 2e-5)
    _assert_rows(AS.attn_rows_torch(qkv.float(), H, n_cls, torch.float32), ref, 2e-5)  # fp32 input
    rows = torch.full((B, H, S, 4), float("nan"))
    tab = AS.attn_stats(qkv, H, n_cls, rows_out=rows)  # the CPU path is the fp32 composition
    assert tab.dtype == torch.float64 and tab.shape == (H, 6)
    assert torch.equal(rows, AS.attn_rows_torch(qkv, H, n_cls, torch.float32))
    want, mags = AR.ref_table(rows)
    assert torch.equal(tab[:, 3:], want[:, 3:])
    assert bool(((tab[:, :3] - want[:, :3]).abs() <= B * S * AR.U53 * mags).all())
    assert tab[:, 4].tolist() == [0.0] * H and tab[:, 5].tolist() == [float(B * S)] * H
    if n_cls == 0:
        assert not bool(rows[..., 2].any())
    if n_cls == S:
        assert bool(((rows[..., 2] - 1).abs() <= 1e-6).all())


@pytest.mark.parametrize("S,n_cls", [(1, 1), (5, 0), (5, 3), (70, 3), (70, 70)])
def test_structural_cases(S, n_cls):
    rows = AS.attn_rows_torch(AR.equal_keys_qkv(2, S, 2, 64), 2, n_cls, torch.float64)
    want = torch.tensor([math.log(S), 1.0 / S, n_cls / S], dtype=torch.float64)
    assert bool(((rows[..., :3] - want).abs() <= 1e-12).all())
    rows = AS.attn_rows_torch(AR.one_ahead_qkv(2, S, 2, 64), 2, n_cls, torch.float64)
    if S > 1:
        assert bool((rows[..., 0].abs() <= 1e-100).all()) and bool(((rows[..., 1] - 1).abs() <= 1e-100).all())
        assert bool((rows[..., 3] == 256.0).all())
        assert bool(((rows[..., 2] - (1.0 if n_cls == S else 0.0)).abs() <= 1e-100).all())
    big = AS.attn_rows_torch(AR.big_logits_qkv(1, S, 1, 64), 1, n_cls, torch.float32)
    assert bool(torch.isfinite(big).all()) and bool((big[..., 0] >= 0).all()) and float(big[..., 3].max()) >= 1984.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nonfinite_rows(dtype):
    B, S, H, hd = 2, 6, 2, 8
    base = AR.random_qkv(B, S, H, hd, seed=1).view(B, S, 3, H, hd)
    clean = AS.attn_rows_torch(base.reshape(B, S, -1), H, 2, dtype)

    def run(edit):
        x = base.clone()
        edit(x)
        x = x.reshape(B, S, -1)
        rows = AS.attn_rows_torch(x, H, 2, dtype)
        ref, _ = AR.ref_rows(x, H, 2)
        assert torch.equal(torch.isnan(rows[..., 0]), torch.from_numpy(ref[..., 0] != ref[..., 0]))
        return rows, AS.table_from_rows(rows.float())

    # a NaN in one q row: that row of that head
    rows, tab = run(lambda x: x[1, 4, 0, 1, 3].fill_(float("nan")))
    bad = torch.isnan(rows[..., 0])
    assert int(bad.sum()) == 1 and bool(bad[1, 1, 4]) and tab[:, 4].tolist() == [0.0, 1.0]
    keep = ~bad
    assert torch.equal(rows[keep], clean[keep])
    assert float(rows[1, 1, 4, 3]) == float("-inf")  # the maxima pass over NaN
    # a NaN in one k row: every row of its (b, h)
    rows, tab = run(lambda x: x[0, 2, 1, 0, 0].fill_(float("nan")))
    bad = torch.isnan(rows[..., 0])
    assert int(bad.sum()) == S and bool(bad[0, 0].all()) and tab[:, 4].tolist() == [float(S), 0.0]
    assert torch.equal(rows[~bad], clean[~bad])
    want = AS.table_from_rows(torch.where(bad[..., None], torch.full_like(clean, float("nan")), clean).float())
    assert torch.equal(tab, want)
    # +inf in k: inf - inf; -inf logits alone leave the row good (p = 0 adds 0)
    def inf_key(value):
        def edit(x):
            x[0, :, 0, 0] = x[0, :, 0, 0].abs() + 1  # positive queries: the logit is value itself
            x[0, 2, 1, 0] = value
        return edit
    rows, tab = run(inf_key(float("inf")))
    assert bool(torch.isnan(rows[0, 0, :, 0]).all()) and tab[0, 4] == S and tab[1, 4] == 0
    rows, tab = run(inf_key(float("-inf")))
    assert bool(torch.isfinite(rows[..., :3]).all()) and tab[:, 4].tolist() == [0.0, 0.0]
    # no good row at all: ZMAX = -inf, sums 0
    x = base.clone()
    x[:, :, 1, 0] = float("nan")
    tab = AS.attn_stats(x.reshape(B, S, -1), H, 2)
    assert tab[0].tolist() == [0.0, 0.0, 0.0, float("-inf"), float(B * S), float(B * S)]


def test_bad_arguments():
    qkv = AR.random_qkv(1, 4, 2, 8)
    with pytest.raises(ValueError):
        AS.attn_stats(qkv[0], 2, 0)  # rank
    with pytest.raises(ValueError):
        AS.attn_stats(qkv, 5, 0)  # 3 D not divisible by the heads
    with pytest.raises(ValueError):
        AS.attn_stats(qkv, 2, 5)  # n_cls > S
    with pytest.raises(ValueError):
        AS.attn_stats(qkv, 2, -1)
    with pytest.raises(ValueError):
        AS.attn_stats(qkv, 2, 0, rows_out=torch.zeros(1, 2, 4, 3))
    with pytest.raises(ValueError):
        AS.attn_stats(qkv, 2, 0, rows_out=torch.zeros(1, 2, 4, 4, dtype=torch.float64))


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


@pytest.mark.parametrize("per_op", ["0", "1"])
def test_collector_visits_every_layer_once_in_order(monkeypatch, per_op):
    monkeypatch.setenv("JMAE_PER_OP", per_op)
    seen = []
    real = AS.attn_stats

    def spy(qkv, heads, n_cls, rows_out=None):
        seen.append((tuple(qkv.shape), heads, n_cls))
        return real(qkv, heads, n_cls, rows_out)
    monkeypatch.setattr(AS, "attn_stats", spy)
    m = _pretrain_model()
    x = _images()
    noise = torch.rand(4, generator=torch.Generator().manual_seed(3))
    ref = m.reconstruct(x, noise=noise)["err"]  # outside the context: nothing is collected
    assert seen == [] and AS._COLLECTOR is None
    got = m.attention_stats(x, noise=noise)
    assert list(got) == ["layer_0", "layer_1", "decoder/dec_layer_0", "decoder/dec_layer_1"]
    # encoder: 3 CLS + 1 kept patch, 2 heads of 32; decoder: 3 + 4 tokens, 2 heads of 16
    assert seen == [((4, 4, 192), 2, 3)] * 2 + [((4, 7, 96), 2, 3)] * 2
    for name, tab in got.items():
        S = 4 if name.startswith("layer") else 7
        assert tab.shape == (2, 6) and tab.dtype == torch.float64
        assert tab[:, 4].tolist() == [0.0, 0.0] and tab[:, 5].tolist() == [4.0 * S] * 2
        ent = tab[:, 0] / tab[:, 5]
        assert bool((ent > 0).all()) and bool((ent <= math.log(S) + 1e-6).all())
        assert bool((tab[:, 2] / tab[:, 5] > 0).all()) and bool((tab[:, 1] / tab[:, 5] >= 1.0 / S - 1e-6).all())
    assert AS._COLLECTOR is None
    seen.clear()
    assert torch.equal(m.reconstruct(x, noise=noise)["err"], ref) and seen == []  # and the forward is unchanged
    with pytest.raises(RuntimeError):
        with AS.collecting(3):
            with AS.collecting(3):
                pass
    assert AS._COLLECTOR is None


def test_both_forward_paths_collect_the_same_tables(monkeypatch):
    m, x = _finetune_model(), _images(seed=1)
    monkeypatch.setenv("JMAE_PER_OP", "0")
    fused = m.attention_stats(x)
    monkeypatch.setenv("JMAE_PER_OP", "1")
    per_op = m.attention_stats(x)
    assert list(fused) == list(per_op) == ["layer_0", "layer_1"]
    for k in fused:
        assert torch.allclose(fused[k], per_op[k], rtol=1e-5, atol=1e-6), k
    # against the definition on the model's own qkv of layer 0
    enc = m.encoder
    rows, _ = m.patches(x, None, None, True, plan=None)
    h = enc.embed_rows(rows, None, 4)
    a = enc.layers[0].attn
    from jumbo_mae_tpu_amd.ops import functional as Fn
    qkv = Fn.linear(enc.layers[0].norm1(h).view(-1, 64), a.qkv_k, a.qkv_b).view(4, 7, 192)
    assert torch.allclose(AS.attn_stats(qkv, 2, 3), per_op["layer_0"], rtol=1e-5, atol=1e-6)
    # the model is untouched and no gradient state appears
    assert m.store.grad is None or not bool(m.store.grad.any())


def test_summarize():
    tab = torch.tensor([[6.0, 3.0, 1.5, 2.5, 0.0, 6.0], [2.0, 4.0, 1.0, 7.0, 2.0, 6.0]], dtype=torch.float64)
    vals, lines = AS.summarize({"layer_0": tab, "decoder/dec_layer_0": tab * torch.tensor([2.0, 1, 1, 1, 0, 1])})
    assert vals["attn/entropy/layer_0"] == pytest.approx((1.0 + 0.5) / 2)
    assert vals["attn/entropy_min/layer_0"] == pytest.approx(0.5)
    assert vals["attn/max_logit/layer_0"] == 7.0
    assert vals["attn/max_prob/layer_0"] == pytest.approx((0.5 + 1.0) / 2)
    assert vals["attn/cls_mass/layer_0"] == pytest.approx((0.25 + 0.25) / 2)
    assert vals["val/attn_entropy_min"] == pytest.approx(0.5) and vals["val/attn_max_logit"] == 7.0
    assert lines == ["attention monitor: layer_0 head 1: 2 of 6 rows have no finite entropy"]
    assert all(isinstance(v, float) for v in vals.values())


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
FLAG = ["--attn-stats", "4"]
KINDS = ("entropy", "entropy_min", "max_logit", "max_prob", "cls_mass")
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


def _rows(out, which):
    return [json.loads(line) for line in open(os.path.join(out, f"{which}-metrics.jsonl"))]


def _is_new(k):
    return k.startswith("attn/") or k in ("val/attn_entropy_min", "val/attn_max_logit")


@pytest.mark.parametrize("which", ["f", "p"])
def test_driver_with_the_flag_changes_nothing_else(runs, which):
    a, b = runs[which, "with"], runs[which, "without"]
    with open(os.path.join(a, f"{which}-last.msgpack"), "rb") as fa, open(os.path.join(b, f"{which}-last.msgpack"), "rb") as fb:
        assert fa.read() == fb.read()
    ra, rb = _rows(a, which), _rows(b, which)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        common = [k for k in y if not k.startswith(VOLATILE) and "time" not in k and k != "config"]
        assert common and {k: x[k] for k in common} == {k: y[k] for k in common}
        assert all(_is_new(k) for k in set(x) - set(y)), set(x) - set(y)
    assert not any(_is_new(k) for r in rb for k in r)
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_resume_state
    sa, sb = (load_resume_state(os.path.join(d, f"{which}-last.state.pt")) for d in (a, b))
    for k in ("mu", "nu"):
        assert torch.equal(sa["optimizer"][k], sb["optimizer"][k])


@pytest.mark.parametrize("which", ["f", "p"])
def test_driver_logs_the_attention_values(runs, which):
    evals = [r for r in _rows(runs[which, "with"], which) if "val/loss" in r]
    assert [r["step"] for r in evals] == [0, 2, 4]  # the sanity evaluation included
    layers = ["layer_0", "layer_1"] + (["decoder/dec_layer_0"] if which == "p" else [])
    for r in evals:
        assert {k.split("/", 2)[2] for k in r if k.startswith("attn/entropy/")} == set(layers)
        for name in layers:
            S = 7 if which == "f" or name.startswith("decoder") else 4  # 3 CLS + 4 patches, 1 of them kept
            for kind in KINDS:
                assert math.isfinite(r[f"attn/{kind}/{name}"]), (kind, name)
            assert 0 < r[f"attn/entropy_min/{name}"] <= r[f"attn/entropy/{name}"] <= math.log(S) + 1e-6
            assert 1.0 / S - 1e-6 <= r[f"attn/max_prob/{name}"] <= 1 and 0 < r[f"attn/cls_mass/{name}"] <= 1 + 1e-6
        assert r["val/attn_entropy_min"] == min(r[f"attn/entropy_min/{n}"] for n in layers)
        assert r["val/attn_max_logit"] == max(r[f"attn/max_logit/{n}"] for n in layers)
    # the weights move, and the same probe images show it
    assert evals[0]["attn/entropy/layer_1"] != evals[2]["attn/entropy/layer_1"]


def test_flag_default():
    for parser in (pretrain_parser, finetune_parser):
        assert parser().parse_args([]).attn_stats == 0
        assert parser().parse_args(["--attn-stats", "64"]).attn_stats == 64


# ------------------------------------------------------------------ tool
def test_attn_stats_tool(runs, shards, capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("attn_stats_tool", os.path.join(root, "tools", "attn_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for which, base in (("p", PRETRAIN), ("f", FINETUNE)):
        model = [a for a in base if a not in ("--name", which)]
        ckpt = os.path.join(runs[which, "with"], f"{which}-last.msgpack")
        out = tool.main(model + ["--valid-dataset-shards", shards[1], "--ckpt", ckpt, "--n", "4"] +
                        (["--finetune"] if which == "f" else []))
        last = [r for r in _rows(runs[which, "with"], which) if "val/loss" in r][-1]
        assert out["images"] == 4 and out["layers"] == (3 if which == "p" else 2)
        # the checkpoint is the run's last state: the tool reproduces the last evaluation's values
        for k, v in out["values"].items():
            assert v == pytest.approx(last[k], rel=1e-6), k
        text = capsys.readouterr().out
        assert text.count("layer_1") == 2 and "entropy" in text.splitlines()[0]
