"""Norm monitor (optim/monitor.py) without a GPU: ``seg_stats_torch`` against the exact reference of
tests/norm_stats_ref.py on the hand-built chunk tables, the layer groups, both drivers with and without
``--log-norms layer`` (identical checkpoints and log values, the new keys), a forced non-finite gradient
(the leaves are named before the abort; a skipped step reports no update) and ZeRO-1 on two gloo ranks
against the replicated run."""

import json
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import norm_stats_ref as NR
import optim_ref as R
from test_dist import _free_port, _init

from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.optim import flat, monitor as M
from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
from jumbo_mae_tpu_amd.train.engine import Trainer

TABLES = ("runs64", "partial", "prod")


@pytest.fixture(scope="module")
def tables():
    return NR.tables(flat.CHUNK)


def frozen_of(tab) -> tuple:
    return (3, 4) if tab.nseg == 7 else (1,)


def test_switch_exists():
    assert P._NORMS_OURS is True and M.COLS == NR.COLS


# ------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("with_old", [True, False])
def test_torch_composition_against_fsum(tables, name, with_old):
    tab = tables[name]
    spec = R.spec_for(tab)
    meta = R.make_meta("adamw", spec, frozen_of(tab))
    p, g = R.make_inputs(tab, spec, 3)
    noise, _ = R.make_inputs(tab, spec, 4)
    old = (p + 1e-2 * noise) if with_old else None
    # non-finite values in every buffer, the 7- and 1-element chunks included; a frozen gradient of NaN
    for k in range(tab.nseg):
        idx = torch.nonzero(tab.seg_of == k).flatten()
        g[idx[0]] = float("inf")
        p[idx[-1]] = float("nan")
        if old is not None and idx.numel() > 2:
            old[idx[1]] = float("-inf")
    for k in frozen_of(tab):
        g[tab.seg_of == k] = float("nan")
    ref, terms = NR.ref_stats(tab, meta, p, g, old)
    keep = [t.clone() for t in (p, g)]
    got = M.seg_stats_torch(p, g, old, tab.rows, meta, tab.nseg)
    assert got.dtype == torch.float64
    NR.assert_stats(got, ref, terms, name)
    assert torch.equal(p.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(
        g.view(torch.int32), keep[1].view(torch.int32))
    for k in frozen_of(tab):
        assert got[k, [0, 2, 3, 4]].tolist() == [0, 0, 0, 0] and got[k, 5] == 1 and got[k, 6] > 0
    if not with_old:
        assert not bool(got[:, 2].any())
    # seg_stats: the same table off the GPU, also into a given tensor; no rows: zeros
    out = torch.full((tab.nseg, 7), float("nan"), dtype=torch.float64)
    assert M.seg_stats(p, g, old, tab.rows, meta, out=out) is out and torch.equal(out, got)
    none = M.seg_stats_torch(p, g, old, tab.rows[:0], meta, tab.nseg)
    assert none.shape == (tab.nseg, 7) and not bool(none.any())


def test_a_segment_without_rows_gets_zeros(tables):
    tab = tables["runs64"]
    rows = tab.rows[(tab.rows[:, 2] != 2) & (tab.rows[:, 2] != 5)]
    cut = R.table_from_rows("cut", rows, tab.n, tab.nseg)
    spec = R.spec_for(tab)
    meta = R.make_meta("adamw", spec)
    p, g = R.make_inputs(tab, spec, 8)
    ref, terms = NR.ref_stats(cut, meta, p, g, None)
    got = M.seg_stats_torch(p, g, None, cut.rows, meta, cut.nseg)
    NR.assert_stats(got, ref, terms, "cut")
    assert not bool(got[2].any()) and not bool(got[5].any()) and bool(got[1, 6] > 0)


# ------------------------------------------------------------------ groups
def _finetune_model(dtype=torch.float32, labels=10):
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=labels, image_size=32, patch_size=16, posemb="learnable",
                   droppath=0.0)
    return FinetuneModel(vc).to("cpu", dtype, seed=0)


def _pretrain_model():
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=0, image_size=32, patch_size=16, posemb="sincos2d",
                   image_mask_ratio=0.75)
    dc = DecoderConfig(dec_layers=2, dec_dim=32, dec_heads=2, image_size=32, patch_size=16)
    return PretrainModel(vc, dc).to("cpu", torch.float32, seed=0)


def _opt(m, kind="adamw", **kw):
    return FlatOptimizer(m.store, kind, lambda c: 1e-2, weight_decay=0.05, num_layers=2, **kw)


def test_group_names():
    ft = M.NormMonitor(_opt(_finetune_model()), "layer")
    assert ft.groups == ["embed", "cls_tokens", "jumbo_mlp", "layer_0", "layer_1", "norm", "head"]
    pt = M.NormMonitor(_opt(_pretrain_model()), "layer")
    assert pt.groups == ["embed", "cls_tokens", "jumbo_mlp", "layer_0", "layer_1", "norm", "image_mask_embedding",
                         "decoder_proj", "decoder/dec_layer_0", "decoder/dec_layer_1", "decoder/dec_norm",
                         "decoder_image_output"]
    assert ft.group_of.numel() == len(ft.store.segments)
    for s, gi in zip(ft.store.segments, ft.group_of.tolist()):
        assert ft.groups[gi] == M.group_name(s.path) and ft.groups[gi] in s.key
    assert M.group_name(("model", "layer_11", "ff", "w1", "kernel")) == "layer_11"
    assert M.group_name(("decoder_model", "dec_layer_3", "norm1", "scale")) == "decoder/dec_layer_3"
    with pytest.raises(ValueError):
        M.NormMonitor(ft.opt, "everything")


# ------------------------------------------------------------------ monitor around Trainer steps
def _batch(n=8, labels=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g),
            torch.randint(0, labels, (n,), generator=g))


@pytest.mark.parametrize("kind", ["adamw", "lars"])
def test_monitor_around_a_step(kind):
    runs = {}
    for with_mon in (True, False):
        m = _finetune_model()
        opt = _opt(m, kind, clip_grad=0.5)
        tr = Trainer(m, opt)
        mon = M.NormMonitor(opt, "layer") if with_mon else None
        for k in range(2):
            tr.train_step([_batch(seed=k)])
        before = m.store.master.clone()
        if mon is not None:
            mon.begin()
        tr.train_step([_batch(seed=2)])
        runs[with_mon] = (m, opt, mon, before)
    m, opt, mon, before = runs[True]
    stats = mon.collect()
    s = m.store
    want = M.seg_stats_torch(s.master, s.grad, before, opt.chunks, opt.meta, opt.nseg)
    assert torch.equal(stats, want)
    d = mon.summary(stats)
    used = torch.zeros(s.total, dtype=torch.bool)
    for sg in s.segments:
        used[sg.offset:sg.offset + sg.numel] = True
    assert d["train/grad_norm"] == pytest.approx(float(s.grad[used].double().norm()), rel=1e-12)
    assert d["train/param_norm"] == pytest.approx(float(s.master[used].double().norm()), rel=1e-12)
    upd = float((s.master.double() - before.double())[used].norm())
    assert upd > 0 and d["train/update_norm"] == pytest.approx(upd, rel=1e-12)
    assert d["train/update_ratio"] == pytest.approx(upd / d["train/param_norm"], rel=1e-12)
    assert d["train/grad_absmax"] == float(s.grad[used].abs().max())
    assert d["train/nonfinite_grads"] == 0 and d["train/nonfinite_params"] == 0
    assert d["train/clip_scale"] == min(1.0, 0.5 / d["train/grad_norm"])
    assert all(isinstance(v, float) for v in d.values())
    for name in mon.groups:
        for kind_ in ("grad", "param", "update_ratio"):
            assert math.isfinite(d[f"norms/{kind_}/{name}"])
    assert sum(d[f"norms/grad/{n}"] ** 2 for n in mon.groups) == pytest.approx(d["train/grad_norm"] ** 2, rel=1e-12)
    assert mon.bad_leaves() == []
    # a second collect without begin(): no snapshot for that step, D2 = 0 and nothing else changes
    again = mon.collect()
    assert not bool(again[:, 2].any()) and torch.equal(again[:, [0, 1, 3, 4, 5, 6]], stats[:, [0, 1, 3, 4, 5, 6]])
    # the global level has no per-group keys
    assert not any(k.startswith("norms/") for k in M.NormMonitor(opt, "global").summary(stats))
    # and the monitor changed nothing: weights and moments bit-identical to the run without it
    m0, opt0, _, _ = runs[False]
    assert torch.equal(m.store.master.view(torch.int32), m0.store.master.view(torch.int32))
    for k in ("mu", "nu", "trace"):
        if getattr(opt, k) is not None:
            assert torch.equal(getattr(opt, k).view(torch.int32), getattr(opt0, k).view(torch.int32)), k


def _nan_loss_call(at_call: int):
    """A ``FinetuneModel.__call__`` whose ``at_call``-th training forward returns a NaN loss."""
    calls = {"n": 0}
    fwd = FinetuneModel.forward

    def call(self, *a, **k):
        o = fwd(self, *a, **k)
        if not k.get("det", True):
            calls["n"] += 1
            if calls["n"] == at_call:
                o["loss"] = o["loss"] * float("nan")
        return o
    return call


def test_skipped_step_reports_no_update(monkeypatch):
    m = _finetune_model()
    opt = _opt(m)
    tr = Trainer(m, opt, skip_nonfinite=True)
    mon = M.NormMonitor(opt, "global")
    tr.train_step([_batch()])
    monkeypatch.setattr(FinetuneModel, "__call__", _nan_loss_call(1))
    mon.begin()
    tr.train_step([_batch(seed=1)])
    assert tr.skipped_steps == 1
    d = mon.summary(mon.collect())
    assert d["train/update_norm"] == 0.0 and d["train/update_ratio"] == 0.0
    assert d["train/nonfinite_grads"] > 0 and d["train/nonfinite_params"] == 0 and d["train/param_norm"] > 0
    lines = mon.bad_leaves()
    assert 0 < len(lines) <= 8
    keys = {s.key: s for s in m.store.segments}
    for line in lines:
        key, rest = line.split(": ")
        g, p, n = (int(x) for x in (rest.split()[0], rest.split()[3], rest.split()[-1]))
        assert key in keys and g > 0 and p == 0 and n == keys[key].numel and rest.endswith(f"non-finite params of {n}")


# ------------------------------------------------------------------ drivers
COMMON = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--learning-rate", "5e-3",
          "--training-steps", "4", "--warmup-steps", "1", "--log-interval", "2", "--eval-interval", "4",
          "--droppath", "0.1", "--clip-grad", "0.5"]
FINETUNE = COMMON + ["--labels", "4", "--name", "f"]
PRETRAIN = COMMON + ["--auto-augment", "none", "--labels", "0", "--dec-layers", "1", "--dec-dim", "64", "--dec-heads", "2",
                     "--dec-droppath", "0.1", "--name", "p"]
LAYER = ["--log-norms", "layer"]
GLOBAL_KEYS = ("train/grad_norm", "train/param_norm", "train/update_norm", "train/update_ratio", "train/grad_absmax",
               "train/nonfinite_grads", "train/nonfinite_params", "train/clip_scale")
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
        for name, extra in (("with", LAYER), ("without", [])):
            out = str(tmp_path_factory.mktemp(which + name))
            main(_args(which, shards, out, extra))
            outs[which, name] = out
    return outs


def _rows(out, which):
    return [json.loads(line) for line in open(os.path.join(out, f"{which}-metrics.jsonl"))]


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
        new = set(x) - set(y)
        assert all(k in GLOBAL_KEYS or k.startswith("norms/") for k in new), new
    assert not any(k in GLOBAL_KEYS or k.startswith("norms/") for r in rb for k in r)
    from jumbo_mae_tpu_amd.ckpt.checkpoint import load_resume_state
    sa, sb = (load_resume_state(os.path.join(d, f"{which}-last.state.pt")) for d in (a, b))
    for k in ("mu", "nu"):
        assert torch.equal(sa["optimizer"][k], sb["optimizer"][k])


@pytest.mark.parametrize("which", ["f", "p"])
def test_driver_logs_the_norms(runs, which):
    logged = [r for r in _rows(runs[which, "with"], which) if "train/loss" in r]
    assert [r["step"] for r in logged] == [2, 4]
    groups = (["embed", "cls_tokens", "jumbo_mlp", "layer_0", "layer_1", "norm"] +
              (["head"] if which == "f" else ["image_mask_embedding", "decoder_proj", "decoder/dec_layer_0",
                                              "decoder/dec_norm", "decoder_image_output"]))
    for r in logged:
        for k in GLOBAL_KEYS:
            assert k in r and math.isfinite(r[k]), (k, r.get(k))
        assert {k.split("/", 2)[2] for k in r if k.startswith("norms/grad/")} == set(groups)
        for name in groups:
            for kind in ("grad", "param", "update_ratio"):
                assert math.isfinite(r[f"norms/{kind}/{name}"]) and r[f"norms/{kind}/{name}"] >= 0
        assert r["train/grad_norm"] > 0 and r["train/update_norm"] > 0 and r["train/nonfinite_grads"] == 0
        assert r["train/update_ratio"] == pytest.approx(r["train/update_norm"] / r["train/param_norm"], rel=1e-12)
        assert r["train/clip_scale"] == min(1.0, 0.5 / r["train/grad_norm"])
        assert r["train/grad_absmax"] <= r["train/grad_norm"]
        assert sum(r[f"norms/grad/{n}"] ** 2 for n in groups) == pytest.approx(r["train/grad_norm"] ** 2, rel=1e-12)


def test_forced_nonfinite_gradient_names_its_leaves(shards, tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(FinetuneModel, "__call__", _nan_loss_call(2))  # the first logged step
    with pytest.raises(FloatingPointError):
        FT.main(_args("f", shards, str(tmp_path), ["--log-norms", "global"]))
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "non-finite grads" in ln]
    assert 0 < len(lines) <= 8, out[-2000:]
    assert lines[0].startswith("model/embed/wte/kernel: 49152 non-finite grads, ") and lines[0].endswith(" of 49152")
    # without the flag the abort names nothing
    with pytest.raises(FloatingPointError):
        monkeypatch.setattr(FinetuneModel, "__call__", _nan_loss_call(2))
        FT.main(_args("f", shards, str(tmp_path / "b")))
    assert "non-finite grads" not in capsys.readouterr().out


def test_flag_choices_and_default():
    for parser in (pretrain_parser, finetune_parser):
        assert parser().parse_args([]).log_norms == "off"
        for v in ("off", "global", "layer"):
            assert parser().parse_args(["--log-norms", v]).log_norms == v
        with pytest.raises(SystemExit):
            parser().parse_args(["--log-norms", "leaf"])
    import argparse
    assert M.make_monitor(argparse.Namespace(log_norms="off"), None) is None


# ------------------------------------------------------------------ ZeRO-1, two gloo ranks
def _zero1_worker(rank, world, port, out):
    _init(rank, world, port)
    from jumbo_mae_tpu_amd.parallel.ddp import GradReducer
    res = {}
    for mode in ("rep", "bf16", "fp32"):
        m = _finetune_model(dtype=torch.bfloat16)
        dist.broadcast(m.store.master, 0)
        m.store.sync_shadow()
        opt = _opt(m, "adamw")
        red = GradReducer(m.store, bucket_mb=0.01, shard=mode != "rep", gather_dtype=mode if mode != "rep" else "bf16")
        tr = Trainer(m, opt, red, None)
        mon = M.NormMonitor(opt, "layer")
        for k in range(3):
            x, y = _batch(8 * world, seed=k)
            if k == 2:
                mon.begin()
            tr.train_step([(x[rank * 8:(rank + 1) * 8], y[rank * 8:(rank + 1) * 8])])
        stats = mon.collect()
        owned = 0 if opt._owned_rows is None else int(opt._owned_rows[:, 1].sum())
        res[mode] = {"stats": stats, "shard": red.shard, "owned": owned, "summary": mon.summary(stats)}
    torch.save(res, f"{out}.{rank}")
    dist.destroy_process_group()


def test_zero1_owned_rows_sum_to_the_replicated_table(tmp_path):
    out = str(tmp_path / "z")
    mp.spawn(_zero1_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    per_rank = [torch.load(f"{out}.{rank}", weights_only=True) for rank in range(2)]
    for r in per_rank:
        rep = r["rep"]["stats"]
        assert not r["rep"]["shard"] and int((rep[:, 0] > 0).sum()) > rep.shape[0] // 2 and float(rep[:, 2].sum()) > 0
        for mode in ("bf16", "fp32"):
            z = r[mode]
            assert z["shard"] and 0 < z["owned"] < int(rep[:, 6].sum())
            got = z["stats"]
            assert torch.equal(got[:, 3:], rep[:, 3:]), mode  # GMAX and the counts
            # the partition changes the summation order: n 2^-53 relative, n the segment's elements
            bound = rep[:, 6:7] * NR.U53 * rep[:, :3]
            err = (got[:, :3] - rep[:, :3]).abs()
            assert bool((err <= bound).all()), (mode, float((err - bound).max()))
            assert set(z["summary"]) == set(r["rep"]["summary"])
    for mode in ("rep", "bf16", "fp32"):  # every rank holds the same table
        assert torch.equal(per_rank[0][mode]["stats"], per_rank[1][mode]["stats"]), mode
