"""Weight EMA (optim/ema.py) without a GPU: the decay schedule, the torch update path against the
float64 oracle of tests/ema_ref.py, split per-bucket updates, skipped steps, ZeRO-1 on two gloo ranks,
and the finetune driver with and without ``--ema-decay`` (logs, the EMA-best checkpoint, resume)."""

import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ema_ref as ER
from test_dist import _free_port, _init

from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params, load_pretrained_params, load_resume_state
from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
from jumbo_mae_tpu_amd.config import ViTConfig
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
from jumbo_mae_tpu_amd.optim.ema import WeightEma, decay_at, omd_at
from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
from jumbo_mae_tpu_amd.train.engine import Trainer


# ------------------------------------------------------------------ schedule
def test_decay_schedule():
    assert decay_at(0.9999, 0) == 0.1 and ER.decay_at(0.9999, 0) == 0.1
    # (1 + t) / (10 + t) reaches 0.9 at t = 80 exactly: 81 / 90
    assert decay_at(0.9, 79) == 80 / 89 < 0.9 and decay_at(0.9, 80) == 0.9 and decay_at(0.9, 81) == 0.9
    # 0.99 at t = 890 (891 / 900); the step before is still on the warm-up
    assert decay_at(0.99, 889) == 890 / 899 < 0.99 and decay_at(0.99, 890) == 0.99
    for decay, t in ((0.9999, 0), (0.9999, 7), (0.9, 500), (0.99, 3), (0.0, 5)):
        assert decay_at(decay, t) == ER.decay_at(decay, t)
        want = float(np.float32(1.0 - min(decay, (1 + t) / (10 + t))))
        assert omd_at(decay, t) == want == ER.omd_at(decay, t)
    assert omd_at(0.9999, 10 ** 6) == float(np.float32(1.0 - 0.9999))
    assert omd_at(0.9, 0) == float(np.float32(0.9))
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            WeightEma(_model().store, bad)


# ------------------------------------------------------------------ torch path
def _model(linear=False, dtype=torch.float32, labels=10):
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=labels, image_size=32, patch_size=16, posemb="learnable",
                   droppath=0.0, linear_probing=linear, batch_norm=linear)
    return FinetuneModel(vc).to("cpu", dtype, seed=0)


def _batch(n=8, labels=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g),
            torch.randint(0, labels, (n,), generator=g))


def _live(store):
    live = torch.zeros(store.total, dtype=torch.bool)
    for s in store.segments:
        if s.trainable:
            live[s.offset:s.offset + s.numel] = True
    return live


LR = {"adamw": 1e-2, "lamb": 1e-2, "lars": 1.0, "sgd": 0.1}


@pytest.mark.parametrize("kind,linear", [("adamw", False), ("lamb", False), ("lars", True), ("sgd", True)])
def test_torch_path_matches_the_oracle(kind, linear):
    runs = {}
    for with_ema in (True, False):
        m = _model(linear)
        opt = FlatOptimizer(m.store, kind, lambda c: LR[kind], weight_decay=0.05, num_layers=2)
        ema = None
        if with_ema:
            ema = WeightEma(m.store, 0.99)
            opt.attach_ema(ema)
        tr = Trainer(m, opt)
        e0 = m.store.master.clone()
        snaps, losses = [], []
        for k in range(3):
            losses.append(float(tr.train_step([_batch(seed=k)])["loss"]))
            snaps.append(m.store.master.clone())
        runs[with_ema] = (m, opt, ema, e0, snaps, losses)
    m, opt, ema, e0, snaps, losses = runs[True]
    assert ema.updates == 3
    live = _live(m.store)
    assert not torch.equal(snaps[2][live], e0[live])  # the weights moved
    ref, bound = ER.run(e0, snaps, 0.99, live)
    err = (ema.ema.double() - ref).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(err[live].max()) < 1e-6 and not torch.equal(ema.ema[live], e0[live])
    # nothing outside the trainable segments: frozen segments and padding stay the initial copy
    assert torch.equal(ER.bits(ema.ema)[~live], ER.bits(e0)[~live])
    if linear:
        frozen = ~live & (snaps[2] != 0)
        assert bool(frozen.any()) and torch.equal(ema.ema[frozen], m.store.master[frozen])
    # the run without the average: same weights, losses and moments, bit for bit
    m0, opt0, _, _, snaps0, losses0 = runs[False]
    assert losses == losses0 and torch.equal(ER.bits(snaps[2]), ER.bits(snaps0[2]))
    for k in ("mu", "nu", "trace"):
        if getattr(opt, k) is not None:
            assert torch.equal(ER.bits(getattr(opt, k)), ER.bits(getattr(opt0, k))), k


def test_zero_increment_keeps_the_bits():
    m = _model()
    ema = WeightEma(m.store, 0.9)
    live = _live(m.store)
    with torch.no_grad():
        m.store.master[:4] = torch.tensor([-0.0, 0.0, 1.5, -2.0])
        ema.ema[:4] = torch.tensor([-0.0, -0.0, 1.5, 3.0])
    before = ema.ema.clone()
    ema.omd = 0.0  # omd == 0: nothing moves, -0.0 included
    ema.update_torch(live)
    assert torch.equal(ER.bits(ema.ema), ER.bits(before))
    ema.omd = 0.5  # p == e keeps the bits of e; the last element moves half way
    ema.update_torch(live)
    assert torch.equal(ER.bits(ema.ema[:3]), ER.bits(before[:3])) and float(ema.ema[3]) == 0.5


# ------------------------------------------------------------------ split updates
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_split_updates_give_the_same_bits(kind):
    out = {}
    for split in (False, True):
        m = _model()
        opt = FlatOptimizer(m.store, kind, lambda c: LR[kind], weight_decay=0.05, num_layers=2)
        ema = WeightEma(m.store, 0.9)
        opt.attach_ema(ema)
        n = m.store.total
        cuts = [(0, 8192), (8192, 3 * 8192)]  # two planned buckets; everything past them is "the rest"
        if split:
            opt.plan_ranges(cuts)
        for k in range(2):
            m.store.grad.copy_(torch.randn(n, generator=torch.Generator().manual_seed(k)) * 1e-2)
            opt.prepare()
            if split:
                for lo, hi in reversed(cuts):
                    opt.launch_range(lo, hi)
                opt.launch_rest()
            else:
                opt.launch()
            opt.finish()
        out[split] = (m.store.master.clone(), ema.ema.clone(), ema.updates)
    assert out[True][2] == out[False][2] == 2
    assert torch.equal(ER.bits(out[True][0]), ER.bits(out[False][0]))
    assert torch.equal(ER.bits(out[True][1]), ER.bits(out[False][1]))
    assert not torch.equal(out[True][1], out[True][0])


# ------------------------------------------------------------------ skipped step
def test_skipped_step_leaves_the_average_alone():
    m = _model()
    opt = FlatOptimizer(m.store, "adamw", lambda c: 1e-2, weight_decay=0.05, num_layers=2)
    ema = WeightEma(m.store, 0.9)
    opt.attach_ema(ema)
    tr = Trainer(m, opt, skip_nonfinite=True)
    tr.train_step([_batch()])
    assert ema.updates == 1 and tr.skipped_steps == 0
    before = ema.ema.clone()
    fwd = m.forward

    def forward(*a, **k):  # an injected non-finite loss
        o = fwd(*a, **k)
        o["loss"] = o["loss"] * float("nan")
        return o

    m.forward = forward
    m.__class__.__call__ = lambda self, *a, **k: self.forward(*a, **k)
    try:
        tr.train_step([_batch(seed=1)])
    finally:
        m.__class__.__call__ = FinetuneModel.forward
    assert tr.skipped_steps == 1 and ema.updates == 1
    assert torch.equal(ER.bits(ema.ema), ER.bits(before))
    m.forward = fwd
    tr.train_step([_batch(seed=2)])  # and the next real step uses the decay of update 1
    assert ema.updates == 2 and ema.omd == omd_at(0.9, 1)


# ------------------------------------------------------------------ swap on the CPU, state io
def test_swapped_restores_and_state_round_trips():
    m = _model(dtype=torch.bfloat16)
    s = m.store
    ema = WeightEma(s, 0.9)
    with torch.no_grad():
        ema.ema.add_(torch.randn(s.total, generator=torch.Generator().manual_seed(3)) * 0.01)
    used = torch.zeros(s.total, dtype=torch.bool)
    for sg in s.segments:
        used[sg.offset:sg.offset + sg.numel] = True
    old = (s.master.clone(), s.shadow.clone(), ema.ema.clone(), s.version)
    with ema.swapped():
        assert torch.equal(s.master[used], old[2][used]) and torch.equal(ema.ema[used], old[0][used])
        assert torch.equal(s.shadow[used], old[2][used].to(torch.bfloat16)) and s.version > old[3]
        v_in = s.version
    assert s.version > v_in
    for now, was in zip((s.master, s.shadow, ema.ema), old):
        assert torch.equal(ER.bits(now), ER.bits(was))
    ema.updates = 5
    d = ema.state_dict()
    assert d["ema"].dtype == torch.float32 and d["ema"].device.type == "cpu" and d["updates"] == 5 and d["decay"] == 0.9
    other = WeightEma(s, 0.9)
    d2 = dict(d, ema=torch.cat([d["ema"], torch.zeros(64)]))  # a store padded further: the prefix rule
    other.load_state_dict(d2)
    assert other.updates == 5 and torch.equal(ER.bits(other.ema), ER.bits(ema.ema))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(d, ema=d["ema"][:s.used_numel() - 1]))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(d, ema=torch.cat([d["ema"], torch.ones(4)])))


# ------------------------------------------------------------------ ZeRO-1, two gloo ranks
def _zero1_worker(rank, world, port, out):
    _init(rank, world, port)
    from jumbo_mae_tpu_amd.parallel.ddp import GradReducer
    res = {}
    for mode in ("rep", "bf16", "fp32"):
        m = _model(dtype=torch.bfloat16)
        dist.broadcast(m.store.master, 0)
        m.store.sync_shadow()
        opt = FlatOptimizer(m.store, "adamw", lambda c: 1e-2, weight_decay=0.05, num_layers=2)
        red = GradReducer(m.store, bucket_mb=0.01, shard=mode != "rep", gather_dtype=mode if mode != "rep" else "bf16")
        ema = WeightEma(m.store, 0.99)
        opt.attach_ema(ema)
        tr = Trainer(m, opt, red, None)
        for k in range(3):
            x, y = _batch(8 * world, seed=k)
            tr.train_step([(x[rank * 8:(rank + 1) * 8], y[rank * 8:(rank + 1) * 8])])
        shadow = m.store.shadow.clone()
        whole_before = torch.equal(m.store.master.to(torch.bfloat16), shadow)
        ema.gather()
        master, avg = m.store.master.clone(), ema.ema.clone()
        cast_ok = torch.equal(master.to(torch.bfloat16), shadow)
        with ema.swapped():
            inside = torch.equal(ER.bits(m.store.master), ER.bits(avg))
        restored = all(torch.equal(ER.bits(a), ER.bits(b))
                       for a, b in ((m.store.master, master), (m.store.shadow, shadow), (ema.ema, avg)))
        res[mode] = {"ema": avg, "master": master, "updates": ema.updates, "cast_ok": cast_ok, "inside": inside,
                     "restored": restored, "whole_before": whole_before, "shard": red.shard}
    torch.save(res, f"{out}.{rank}")
    dist.destroy_process_group()


def test_zero1_owned_pieces_gather_to_the_replicated_average(tmp_path):
    out = str(tmp_path / "z")
    mp.spawn(_zero1_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for rank in range(2):
        r = torch.load(f"{out}.{rank}", weights_only=True)
        rep = r["rep"]
        assert not rep["shard"] and rep["updates"] == 3 and not torch.equal(rep["ema"], rep["master"])
        for mode in ("bf16", "fp32"):
            z = r[mode]
            assert z["shard"] and z["updates"] == 3
            assert torch.equal(ER.bits(z["ema"]), ER.bits(rep["ema"])), (rank, mode)
            assert torch.equal(ER.bits(z["master"]), ER.bits(rep["master"])), (rank, mode)
            assert z["cast_ok"] and z["inside"] and z["restored"], (rank, mode, z)
        assert not r["bf16"]["whole_before"]  # the bf16 gather leaves the master sharded between checkpoints


# ------------------------------------------------------------------ driver
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--labels", "4",
          "--learning-rate", "5e-3", "--training-steps", "6", "--warmup-steps", "1", "--log-interval", "1",
          "--eval-interval", "2", "--droppath", "0.1", "--name", "f"]
EMA = ["--ema-decay", "0.9"]


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=2, per_shard=11, classes=4, seed=1, prefix="valid")
    return train, valid


def _args(shards, out, extra=()):
    train, valid = shards
    return finetune_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                  "--output-dir", out, *extra])


@pytest.fixture(scope="module")
def runs(shards, tmp_path_factory):
    outs = {}
    for name, extra in (("with", EMA), ("without", [])):
        out = str(tmp_path_factory.mktemp(name))
        outs[name] = (out, FT.main(_args(shards, out, extra)))
    return outs


def _rows(out):
    return [json.loads(line) for line in open(os.path.join(out, "f-metrics.jsonl"))]


EMA_KEYS = ("val/ema_loss", "val/ema_acc1", "val/ema_acc5", "val/ema_acc1/best")
VOLATILE = ("perf/", "time")


def test_driver_with_the_flag_changes_nothing_else(runs):
    (a, res_a), (b, res_b) = runs["with"], runs["without"]
    with open(os.path.join(a, "f-last.msgpack"), "rb") as fa, open(os.path.join(b, "f-last.msgpack"), "rb") as fb:
        assert fa.read() == fb.read()
    ra, rb = _rows(a), _rows(b)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        # the config row records the flag and the output directory
        common = [k for k in y if not k.startswith(VOLATILE) and "time" not in k and k != "config"]
        assert common and all(k in x for k in common)
        assert {k: x[k] for k in common} == {k: y[k] for k in common}
        assert set(x) - set(y) <= set(EMA_KEYS)
    assert not any(k.startswith("val/ema") for r in rb for k in r) and "val/ema_acc1" not in res_b
    assert not os.path.exists(os.path.join(b, "f-ema-best.msgpack"))
    sa, sb = (load_resume_state(os.path.join(d, "f-last.state.pt")) for d in (a, b))
    assert "ema" not in sb and sa["ema"]["updates"] == 6 and sa["ema"]["decay"] == 0.9
    for k in ("mu", "nu"):
        assert torch.equal(sa["optimizer"][k], sb["optimizer"][k])


def test_driver_logs_the_ema_metrics_and_writes_the_best(runs, shards):
    out, res = runs["with"]
    evals = [r for r in _rows(out) if "val/loss" in r]
    assert [r["step"] for r in evals] == [0, 2, 4, 6]  # the sanity evaluation and every second step
    for r in evals:
        assert all(k in r for k in EMA_KEYS), r
        assert 0.0 <= r["val/ema_acc1"] <= r["val/ema_acc5"] <= 1.0
    # before the first update the average IS the weights
    assert evals[0]["val/ema_loss"] == evals[0]["val/loss"] and evals[0]["val/ema_acc1"] == evals[0]["val/acc1"]
    assert evals[-1]["val/ema_loss"] != evals[-1]["val/loss"]
    best = max(r["val/ema_acc1"] for r in evals[1:])
    assert evals[-1]["val/ema_acc1/best"] == best == res["val/ema_acc1/best"]
    path = os.path.join(out, "f-ema-best.msgpack")
    assert os.path.exists(path) == (best > 0)
    if best == 0:
        return
    # the file is an ordinary params tree with the leaves of "last".  --pretrained-ckpt's loader takes
    # every leaf of it but the head, which that flag re-initialises by design (a finetune starts a new
    # head); so the logged numbers are reproduced from the whole tree, loaded the way --resume loads one:
    # the accuracy AND the loss of the evaluation that wrote the file (the first to reach the best)
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.utils.rng import RngStreams
    args = _args(shards, out)
    model = FT.build_model(args, torch.device("cpu"), torch.float32)
    last = flatten_tree(load_params(os.path.join(out, "f-last.msgpack")))
    saved = flatten_tree(load_params(path))
    assert set(saved) == set(last) and all(np.shape(saved[k]) == np.shape(last[k]) for k in last)
    lines = []
    merged = flatten_tree(load_pretrained_params(path, model.flax_params(), lines.append))
    body = [k for k in saved if "head" not in k]
    assert len(body) > 10 and f"{len(body)} pretrained leaves loaded" in lines[-1]
    assert all(np.array_equal(merged[k], saved[k]) for k in body)
    model.store.load_flax_tree(load_params(path), strict=True)
    _, valid_loader = create_dataloaders(args, 0, 1, 0, device_augment=False, device_valid=False)
    got = FT.evaluate(model, valid_loader, RngStreams({"mixup": 0, "dropout": 0, "noise": 0}, 0, "cpu"),
                      torch.device("cpu"))
    wrote = next(r for r in evals[1:] if r["val/ema_acc1"] == best)
    assert got["val/acc1"] == wrote["val/ema_acc1"] and got["val/loss"] == wrote["val/ema_loss"]


@pytest.mark.parametrize("stop", [4, 3])
def test_interrupted_run_resumes_the_average(runs, shards, tmp_path, stop, capsys):
    out = str(tmp_path)
    FT.main(_args(shards, out, EMA + ["--stop-after-steps", str(stop)]))
    assert max(r["step"] for r in _rows(out)) <= stop
    capsys.readouterr()
    res = FT.main(_args(shards, out, EMA + ["--resume", "auto"]))
    assert f"restored the weight EMA after {stop} updates" in capsys.readouterr().out
    ref_out, ref = runs["with"]
    assert res["final_step"] == 6
    sa, sb = (load_resume_state(os.path.join(d, "f-last.state.pt")) for d in (ref_out, out))
    assert sb["ema"]["updates"] == 6 and torch.equal(ER.bits(sa["ema"]["ema"]), ER.bits(sb["ema"]["ema"]))
    assert sa["best"] == sb["best"] and "val/ema_acc1" in sb["best"]
    for k in EMA_KEYS:
        assert res[k] == ref[k], k
    last = {r["step"]: r for r in _rows(out) if "val/ema_loss" in r}
    want = {r["step"]: r for r in _rows(ref_out) if "val/ema_loss" in r}
    for step in (s for s in want if s > stop):
        assert all(last[step][k] == want[step][k] for k in EMA_KEYS), step


def test_resume_without_ema_state_starts_from_the_weights(runs, shards, tmp_path, capsys):
    out = str(tmp_path)
    FT.main(_args(shards, out, ["--stop-after-steps", "4"]))  # no flag: a sidecar without the average
    assert "ema" not in load_resume_state(os.path.join(out, "f-last.state.pt"))
    capsys.readouterr()
    res = FT.main(_args(shards, out, EMA + ["--resume", "auto"]))
    assert "no weight EMA in the resume state: the average starts from the restored weights" in capsys.readouterr().out
    st = load_resume_state(os.path.join(out, "f-last.state.pt"))
    assert st["ema"]["updates"] == 2 and res["final_step"] == 6
    first = next(r for r in _rows(out) if "val/ema_loss" in r)  # the resumed run's sanity evaluation
    assert first["step"] == 4 and first["val/ema_loss"] == first["val/loss"]


# ------------------------------------------------------------------ flags
def test_flag_range_and_scope():
    assert finetune_parser().parse_args([]).ema_decay == 0.0
    assert finetune_parser().parse_args(["--ema-decay", "0.9999"]).ema_decay == 0.9999
    assert finetune_parser().parse_args(["--mode", "linear", "--ema-decay", "0"]).ema_decay == 0.0
    for bad in ("1.0", "-0.1", "2"):
        with pytest.raises(SystemExit):
            finetune_parser().parse_args(["--ema-decay", bad])
    with pytest.raises(SystemExit):
        pretrain_parser().parse_args(["--ema-decay", "0.9"])
