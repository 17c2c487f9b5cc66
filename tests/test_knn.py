"""k-NN monitor on the CPU: the torch compositions (ops/knn.py, the oracles of csrc/knn.hip) against
brute-force Python loops, ``knn_classify``, ``PretrainModel.features`` and the ``--knn-k`` flag of
``main_pretrain`` (one process and two gloo ranks)."""

import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import knn_ref as KR
from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.ops import knn as K
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser


# ------------------------------------------------------------------ compositions
@pytest.mark.parametrize("Nq,Nb,D,k", [(37, 203, 96, 1), (37, 203, 96, 5), (37, 203, 96, 20), (37, 203, 96, 64),
                                       (70, 13, 32, 20)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_topk_composition_tie_rules(Nq, Nb, D, k, dtype):
    q, bank = KR.exact_inputs(Nq, Nb, D, seed=Nq + k)
    ridx, rsim = KR.brute_topk(q, bank, k)
    idx, sim = K.knn_topk_torch(q, bank, k, dtype=dtype)
    assert idx.dtype == torch.int32 and sim.dtype == dtype
    assert torch.equal(idx, ridx)
    assert torch.equal(sim.double(), rsim)  # exactly summable inputs: no rounding in either precision
    # ties between different indices are present, and resolved by ascending index
    tied = (sim[:, 1:] == sim[:, :-1]) & (idx[:, 1:] >= 0)
    if k > 1:
        assert tied.any() and (idx[:, 1:][tied] > idx[:, :-1][tied]).all()
    if Nb < k:
        assert (idx[:, Nb:] == -1).all() and torch.isinf(sim[:, Nb:]).all() and (sim[:, Nb:] < 0).all()


def test_topk_composition_leave_one_out():
    q, _ = KR.exact_inputs(150, 150, 64, seed=3, q_from_bank=False)
    bank = q.clone()
    bank[100:110] = bank[0:10]  # duplicates at other indices
    q = bank.clone()
    me = torch.arange(150)
    idx, sim = K.knn_topk_torch(q, bank, 20, self_idx=me)
    ridx, rsim = KR.brute_topk(q, bank, 20, self_idx=me)
    assert torch.equal(idx, ridx) and torch.equal(sim.double(), rsim)
    assert not (idx == me[:, None].to(torch.int32)).any()
    for r in range(10):  # the copy of row r is its nearest neighbour, and vice versa
        assert idx[r, 0] == 100 + r and idx[100 + r, 0] == r
    # the dispatcher on the CPU is the composition
    i2, s2 = K.knn_topk(q, bank, 20, self_idx=me)
    assert torch.equal(i2, idx) and torch.equal(s2, sim)


@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("classes", [10, 1000])
def test_vote_composition(k, classes):
    idx, sim, bank_labels, labels = KR.vote_inputs(129, k, classes)
    pred, h1, h5 = K.knn_vote_torch(idx, sim, bank_labels, labels, 0.07)
    rp, r1, r5 = KR.brute_vote(idx, sim, bank_labels, labels, 0.07)
    assert torch.equal(pred, rp) and torch.equal(h1, r1) and torch.equal(h5, r5)
    assert not h1[labels == -1].any() and not h5[labels == -1].any()
    assert (h5 | ~h1).all()
    if k >= 4:  # the constructed tie: classes 1 and 3 with equal scores, the smaller id first
        assert pred[1].tolist() == [1, 3, -1, -1, -1]
    assert (pred[128] == -1).all()  # no neighbour at all
    p2, a1, a5 = K.knn_vote(idx, sim, bank_labels, labels, 0.07)
    assert torch.equal(p2, pred) and torch.equal(a1, h1) and torch.equal(a5, h5)


def _clusters(classes, per, D, noise, seed):
    g = torch.Generator().manual_seed(seed)
    cent = torch.nn.functional.normalize(torch.randn(classes, D, generator=g), dim=-1)
    x = cent.repeat_interleave(per, 0) + noise * torch.randn(classes * per, D, generator=g)
    return K.normalize_features(x), torch.arange(classes).repeat_interleave(per)


def test_normalize_features():
    x = torch.randn(5, 48) * 7
    f = K.normalize_features(x)
    assert f.dtype == torch.bfloat16 and torch.equal(f, torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16))


def test_classify_leave_one_out_and_bank():
    feats, labels = _clusters(6, 10, 64, 0.02, seed=0)
    h1, h5 = K.knn_classify(feats, labels, 5, 0.07)
    assert h1.all() and h5.all()
    # padded rows (-1): dropped from the bank, never a hit, and the other rows' answers do not move
    pf = torch.cat([feats[:7], feats[3:5], feats[7:]])
    pl = torch.cat([labels[:7], torch.tensor([-1, -1]), labels[7:]])
    g1, g5 = K.knn_classify(pf, pl, 5, 0.07)
    assert not g1[7:9].any() and not g5[7:9].any()
    assert torch.equal(torch.cat([g1[:7], g1[9:]]), h1)
    # leave-one-out really leaves the row out: with k = 1 a unique row finds its class mate, not itself
    idx, _ = K.knn_topk(feats, feats, 1, torch.arange(60))
    assert (idx[:, 0] != torch.arange(60)).all()
    # with a bank: no leave-one-out, wrong bank labels give wrong answers
    b1, b5 = K.knn_classify(feats[::2], labels[::2], 5, 0.07, bank=feats[1::2], bank_labels=labels[1::2])
    assert b1.all() and b5.all()
    w1, _ = K.knn_classify(feats[::2], labels[::2], 5, 0.07, bank=feats[1::2], bank_labels=(labels[1::2] + 1) % 6)
    assert not w1.any()
    # a bank with -1 rows and self indices into the unfiltered bank (the driver's gathered layout)
    s1, s5 = K.knn_classify(pf, pl, 5, 0.07, bank=pf, bank_labels=pl, self_idx=torch.arange(62))
    assert torch.equal(s1, g1) and torch.equal(s5, g5)
    e1, e5 = K.knn_classify(feats, labels, 5, 0.07, bank=feats, bank_labels=torch.full((60,), -1))
    assert not e1.any() and not e5.any()


def test_k_above_64_fails_early():
    feats, labels = _clusters(2, 4, 32, 0.02, seed=1)
    for fn in (lambda: K.knn_classify(feats, labels, 65, 0.07), lambda: K.knn_topk(feats, feats, 65),
               lambda: K.knn_topk_torch(feats, feats, 0)):
        with pytest.raises(ValueError, match="k must be in 1..64"):
            fn()
    args = pretrain_parser().parse_args(["--knn-k", "65"])
    with pytest.raises(ValueError, match="k must be in 1..64"):
        PT.main(args)  # before any model, loader or process group exists


def test_switch_exists():
    assert P._KNN_OURS is True


# ------------------------------------------------------------------ features
def test_pretrain_features_equal_finetune_features():
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.ops import mae as mae_ops

    kw = dict(layers=2, dim=64, heads=2, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.1)
    pm = PretrainModel(ViTConfig(labels=0, image_mask_ratio=0.75, **kw),
                       DecoderConfig(dec_layers=1, dec_dim=64, dec_heads=2, image_size=32, patch_size=16)).to("cpu", seed=0)
    fm = FinetuneModel(ViTConfig(labels=10, **kw)).to("cpu", seed=1)
    src, dst = pm.store.to_flax_tree(), fm.store.to_flax_tree()
    dst["model"] = {**src["model"], "head": dst["model"]["head"]}
    fm.store.load_flax_tree(dst, strict=True)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (8, 3, 32, 32), generator=g, dtype=torch.uint8)
    state = torch.get_rng_state()
    f = pm.features(img)
    assert torch.equal(torch.get_rng_state(), state)  # no random stream is touched
    assert f.shape == (8, 192) and f.dtype == torch.float32 and torch.isfinite(f).all() and not f.requires_grad
    assert torch.equal(pm.features(img), f)
    rows = mae_ops.mixed_patches(img, None, 16, fm.store.compute_dtype)
    with torch.no_grad():
        assert torch.equal(fm.features(rows, 8), f)


# ------------------------------------------------------------------ driver
S = 32
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", str(S),
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--auto-augment", "none", "--augment-repeats", "1",
          "--labels", "0", "--dec-layers", "1", "--dec-dim", "64", "--dec-heads", "2", "--learning-rate", "5e-3",
          "--training-steps", "2", "--warmup-steps", "1", "--log-interval", "1", "--eval-interval", "2",
          "--droppath", "0.1", "--dec-droppath", "0.1", "--name", "p"]


def test_flags_are_pretrain_only_and_off_by_default():
    a = pretrain_parser().parse_args([])
    assert a.knn_k == 0 and a.knn_temperature == 0.07
    a = pretrain_parser().parse_args(["--knn-k", "0", "--knn-temperature", "0.1"])
    assert a.knn_k == 0 and a.knn_temperature == 0.1
    with pytest.raises(SystemExit):
        finetune_parser().parse_args(["--knn-k", "5"])


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=2, per_shard=11, classes=4, seed=1, prefix="valid")
    return train, valid


@pytest.fixture(scope="module")
def runs(shards, tmp_path_factory):
    train, valid = shards
    outs = {}
    for name, extra in (("with", ["--knn-k", "5"]), ("zero", ["--knn-k", "0"]), ("without", [])):
        out = str(tmp_path_factory.mktemp(name))
        args = pretrain_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                      "--output-dir", out, *extra])
        outs[name] = (out, PT.main(args))
    return outs


def _rows(out):
    return [json.loads(line) for line in open(os.path.join(out, "p-metrics.jsonl"))]


def test_driver_logs_knn_accuracy(runs):
    out, res = runs["with"]
    rows = [r for r in _rows(out) if "val/loss" in r]
    assert len(rows) == 2  # the sanity evaluation and the last step
    for r in rows + [res]:
        assert 0.0 <= r["val/knn_acc1"] <= r["val/knn_acc5"] <= 1.0, r
    # 22 labelled validation images: the accuracies are multiples of 1 / 22
    assert abs(rows[0]["val/knn_acc1"] * 22 - round(rows[0]["val/knn_acc1"] * 22)) < 1e-9


def test_driver_without_the_flag_is_untouched(runs):
    for name in ("without", "zero"):
        out, res = runs[name]
        assert not any("val/knn_acc1" in r or "val/knn_acc5" in r for r in _rows(out))
        assert "val/knn_acc1" not in res and "val/knn_acc5" not in res
        a = flatten_tree(load_params(os.path.join(out, "p-last.msgpack")))
        b = flatten_tree(load_params(os.path.join(runs["with"][0], "p-last.msgpack")))
        assert set(a) == set(b)
        for k in a:  # the monitor takes nothing from the training streams: bit-identical final weights
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "/".join(k)
        la = [r["val/loss"] for r in _rows(out) if "val/loss" in r]
        lb = [r["val/loss"] for r in _rows(runs["with"][0]) if "val/loss" in r]
        assert la == lb


def test_no_labels_is_one_log_line():
    class Model:
        def evaluate(self, images, valid, rngs):
            return {"loss": torch.tensor(2.0), "num_samples": torch.tensor(4.0)}

        def features(self, images):
            raise AssertionError("no labels: no features")

    class Rngs:
        def fork(self):
            return self

        def as_dict(self):
            return {}

    lines = []
    res = PT.evaluate(Model(), [torch.zeros(4, 3, 8, 8, dtype=torch.uint8)], Rngs(), torch.device("cpu"), 5, 0.07,
                      lines.append)
    assert res == {"val/loss": 0.5}
    assert len(lines) == 1 and "no labels" in lines[0]


# ------------------------------------------------------------------ two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_args(shards, out):
    train, valid = shards
    return pretrain_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                  "--output-dir", out, "--knn-k", "5"])


def _evaluate_once(args, rank, world):
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    device = torch.device("cpu")
    model = PT.build_model(args, device, torch.float32)
    rngs = RngStreams({"mixup": 0, "dropout": 0, "noise": 0}, rank, device)
    _, valid_loader = create_dataloaders(args, rank, world, 0, device_augment=False, device_valid=False)
    return PT.evaluate(model, valid_loader, rngs, device, args.knn_k, args.knn_temperature)


def _gloo_worker(rank, world, port, shards, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from jumbo_mae_tpu_amd.parallel import dist as pdist
    pdist.init_distributed("cpu")
    res = _evaluate_once(_eval_args(shards, out), rank, world)
    torch.save(res, os.path.join(out, f"res{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(shards, tmp_path):
    one = _evaluate_once(_eval_args(shards, str(tmp_path)), 0, 1)
    mp.spawn(_gloo_worker, args=(2, _free_port(), shards, str(tmp_path)), nprocs=2, join=True)
    two = [torch.load(os.path.join(str(tmp_path), f"res{r}.pt"), weights_only=True) for r in range(2)]
    assert two[0] == two[1]
    for key in ("val/knn_acc1", "val/knn_acc5"):
        assert two[0][key] == one[key], (key, one, two)
    assert 0.0 <= one["val/knn_acc1"] <= one["val/knn_acc5"] <= 1.0


# ------------------------------------------------------------------ tool
def test_knn_eval_tool(shards, capsys):
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("knn_eval", os.path.join(root, "tools", "knn_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    train, valid = shards
    model = [a for a in DRIVER if a not in ("--name", "p")]
    loo = tool.main(model + ["--valid-dataset-shards", valid, "--k", "5"])
    assert loo["leave_one_out"] and loo["queries"] == 22 and loo["bank"] == 22 and loo["D"] == 192
    assert 0.0 <= loo["acc1"] <= loo["acc5"] <= 1.0
    # the monitor's number at the sanity evaluation of the same initialization
    args = pretrain_parser().parse_args(DRIVER + ["--valid-dataset-shards", valid, "--knn-k", "5"])
    assert abs(_evaluate_once(args, 0, 1)["val/knn_acc1"] - loo["acc1"]) < 1e-6
    banked = tool.main(model + ["--valid-dataset-shards", valid, "--bank-dataset-shards", train, "--bank-images", "12",
                                "--k", "5"])
    assert not banked["leave_one_out"] and banked["queries"] == 22 and banked["bank"] == 12
    rnd = tool.main(["--random-rows", "50", "--dim", "32", "--k", "5", "--device", "cpu"])
    assert rnd["D"] == 96 and rnd["bank"] == 50
    assert len(capsys.readouterr().out.strip().splitlines()) == 3  # one JSON line per run
    # the timing baseline computes the same lists where there are no ties
    g = torch.Generator().manual_seed(0)
    f = K.normalize_features(torch.randn(40, 64, generator=g))
    me = torch.arange(40)
    i1, s1 = K.knn_topk_torch(f, f, 5, me)
    i2, s2 = tool.topk_chunked_torch(f, f, 5, me, rows=16, cols=12)
    assert torch.equal(i1.long(), i2) and torch.allclose(s1, s2, atol=1e-6)
