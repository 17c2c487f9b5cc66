"""Distillation without a GPU: the definition ``kd_loss_torch`` (ops/functional.py) against the closed
form of tests/distill_ref.py and ``gradcheck``, the flags, and the finetune driver with
``--teacher-ckpt`` on the CPU (logs, the teacher's sanity evaluation, alpha 0, checkpoints)."""

import json
import os

import pytest
import torch
import torch.nn.functional as F

import distill_ref as D

from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.ops import functional as Fn
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser

CASES = [("soft", 1.0), ("soft", 2.5), ("hard", 1.0), ("hard", 2.5)]


def _zu(seed=0, B=3, L=5, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn(B, L, generator=g)).to(dtype), (2.0 * torch.randn(B, L, generator=g)).to(dtype)


# ------------------------------------------------------------------ definition
@pytest.mark.parametrize("mode, T", CASES)
def test_definition_matches_closed_form_and_gradcheck(mode, T):
    z, u = _zu()
    kd64, dz64, t, agree64 = D.closed_form(z, u, T, mode)
    zz = z.clone().requires_grad_(True)
    kd, agree = Fn.kd_loss_torch(zz, u, T, mode)
    assert kd.dtype == torch.float64 and agree.dtype == torch.bool and kd.shape == agree.shape == (3,)
    assert torch.allclose(kd, kd64, rtol=1e-12, atol=1e-14) and torch.equal(agree, agree64)
    w = torch.tensor([0.3, 1.0, 2.0], dtype=torch.float64)
    (dz,) = torch.autograd.grad(kd, zz, w)
    assert torch.allclose(dz, dz64 * w[:, None], rtol=1e-12, atol=1e-14)
    assert torch.autograd.gradcheck(lambda x: Fn.kd_loss_torch(x, u, T, mode)[0], (z.clone().requires_grad_(True),))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T", [1.0, 2.5])
def test_soft_against_itself_is_exactly_zero(dtype, T):
    z, _ = _zu(1, 4, 9, dtype)
    zz = z.clone().requires_grad_(True)
    kd, agree = Fn.kd_loss_torch(zz, z.clone(), T, "soft")
    (dz,) = torch.autograd.grad(kd.sum(), zz)
    assert torch.equal(kd, torch.zeros_like(kd)) and torch.equal(dz, torch.zeros_like(dz)) and agree.all()


def test_hard_is_cross_entropy_against_the_teacher_argmax():
    z, u = _zu(2, 6, 7)
    for T in (1.0, 3.0):  # T is ignored
        kd, _ = Fn.kd_loss_torch(z, u, T, "hard")
        assert torch.allclose(kd, F.cross_entropy(z, u.argmax(-1), reduction="none"), rtol=1e-13, atol=0)


def test_ties_pick_the_lowest_index():
    u = torch.tensor([[1.0, 5.0, 5.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 7.0, 7.0]])
    z = torch.tensor([[0.0, 3.0, 3.0, 3.0], [9.0, 0.0, 0.0, 9.0], [0.0, 0.0, 1.0, 2.0]])
    assert Fn.argmax_first(u).tolist() == [1, 0, 2] == D.argmax_first(u).tolist()
    kd, agree = Fn.kd_loss_torch(z, u, 1.0, "hard")
    assert agree.tolist() == [True, True, False]  # arg-max z: 1, 0, 3
    assert torch.equal(kd, -torch.log_softmax(z, -1)[torch.arange(3), torch.tensor([1, 0, 2])])


@pytest.mark.parametrize("T", [1.0, 2.5])
def test_soft_gradient_rows_sum_to_zero_and_the_teacher_gets_none(T):
    z, u = _zu(3, 5, 11)
    zz, uu = z.clone().requires_grad_(True), u.clone().requires_grad_(True)
    kd, agree = Fn.kd_loss_torch(zz, uu, T, "soft")
    kd.sum().backward()
    assert zz.grad.sum(-1).abs().max().item() < 1e-14 and uu.grad is None and not agree.requires_grad
    zz.grad = None
    Fn.kd_loss_torch(zz, uu, T, "hard")[0].sum().backward()
    assert uu.grad is None and zz.grad is not None
    assert Fn.kd_loss(zz, uu, T, "soft")[0].requires_grad  # the CPU path of the op is the definition
    with pytest.raises(KeyError):
        Fn.kd_loss_torch(z, u, 1.0, "medium")
    with pytest.raises(ValueError):
        Fn.kd_loss_torch(z, u, 0.0, "soft")


@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1025])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_oracle_does_not_cancel_on_the_structured_rows(L, dtype):
    """Two algebraic forms of the soft value agree in fp64 to far below an fp32 ulp on every row of
    ``pair_rows``, the +-60 rows included: the GPU test needs no second oracle for them."""
    z, u, names = D.pair_rows(L, dtype)
    for T in (1.0, 2.0, 4.0):
        a = D.closed_form(z, u, T, "soft")[0]
        b = D.soft_split64(z, u, T)
        assert ((a - b).abs() <= 1e-3 * D.ulp32(a) + 1e-300).all(), (T, [n for n, bad in zip(names, (a - b).abs() > 1e-3 * D.ulp32(a)) if bad])
        assert (a >= 0).all()


# ------------------------------------------------------------------ flags
def test_flags_range_and_scope():
    a = finetune_parser().parse_args([])
    assert a.teacher_ckpt == "" and a.distill_alpha == 0.5 and a.distill_temperature == 1.0 and a.distill_mode == "soft"
    assert a.teacher_layers is None and a.teacher_dim is None and a.teacher_heads is None and not a.teacher_layerscale
    a = finetune_parser().parse_args(["--teacher-ckpt", "x.msgpack", "--teacher-layers", "24", "--teacher-dim", "1024",
                                      "--teacher-heads", "16", "--teacher-layerscale", "--distill-alpha", "1",
                                      "--distill-temperature", "3", "--distill-mode", "hard"])
    assert (a.teacher_layers, a.teacher_dim, a.teacher_heads, a.teacher_layerscale) == (24, 1024, 16, True)
    assert (a.distill_alpha, a.distill_temperature, a.distill_mode) == (1.0, 3.0, "hard")
    for bad in (["--distill-alpha", "1.5"], ["--distill-alpha", "-0.1"], ["--distill-temperature", "0"],
                ["--distill-temperature", "-1"], ["--distill-mode", "medium"]):
        with pytest.raises(SystemExit):
            finetune_parser().parse_args(bad)
    for flag in (["--teacher-ckpt", "x"], ["--distill-alpha", "0.5"], ["--distill-mode", "soft"]):
        with pytest.raises(SystemExit):
            pretrain_parser().parse_args(flag)


# ------------------------------------------------------------------ driver
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
          "--patch-size", "16", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--labels", "4",
          "--learning-rate", "5e-3", "--warmup-steps", "1", "--log-interval", "1", "--eval-interval", "2"]
PLAIN = ["--dropout", "0", "--droppath", "0", "--mixup", "0", "--cutmix", "0"]


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=2, per_shard=11, classes=4, seed=1, prefix="valid")
    return train, valid


def _run(shards, out, name, extra):
    train, valid = shards
    args = finetune_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                  "--output-dir", out, "--name", name, *extra])
    return FT.main(args)


def _rows(out, name):
    return [json.loads(line) for line in open(os.path.join(out, f"{name}-metrics.jsonl"))]


@pytest.fixture(scope="module")
def teacher(shards, tmp_path_factory):
    """A 2-layer teacher trained for four steps: (its -last prefix, the run's result)."""
    out = str(tmp_path_factory.mktemp("teacher"))
    res = _run(shards, out, "t", ["--layers", "2", "--training-steps", "4", "--droppath", "0.1"])
    return os.path.join(out, "t-last"), res


STUDENT = ["--layers", "1", "--training-steps", "4", "--droppath", "0.1"]


@pytest.fixture(scope="module")
def students(shards, teacher, tmp_path_factory):
    """1-layer students: without a teacher, with one (soft, the defaults), with one at alpha 0."""
    ckpt = teacher[0] + ".msgpack"
    kd = ["--teacher-ckpt", ckpt, "--teacher-layers", "2"]
    outs = {}
    for name, extra in (("plain", []), ("kd", kd), ("alpha0", kd + ["--distill-alpha", "0"])):
        out = str(tmp_path_factory.mktemp(name))
        outs[name] = (out, _run(shards, out, "f", STUDENT + extra))
    return outs


KD_TRAIN = ("train/kd_loss", "train/kd_agree", "train/cls_loss")
KD_VAL = ("val/teacher_acc1", "val/teacher_acc5", "val/teacher_loss")


def test_driver_logs_the_distillation_metrics(students, teacher):
    out, res = students["kd"]
    rows = _rows(out, "f")
    train = [r for r in rows if "train/loss" in r]
    assert [r["step"] for r in train] == [1, 2, 3, 4]
    for r in train:
        assert all(k in r for k in KD_TRAIN), r
        assert r["train/kd_loss"] > 0 and 0.0 <= r["train/kd_agree"] <= 1.0
        want = 0.5 * r["train/cls_loss"] + 0.5 * r["train/kd_loss"]
        assert abs(r["train/loss"] - want) <= 1e-6 * abs(want)
    evals = [r for r in rows if "val/loss" in r]
    assert [r["step"] for r in evals] == [0, 2, 4]
    assert all(k in evals[0] for k in KD_VAL)  # at the sanity evaluation and only there
    assert not any(k.startswith("val/teacher") for r in evals[1:] for k in r)
    # the teacher loaded correctly: its own run's final validation, reproduced
    assert evals[0]["val/teacher_acc1"] == teacher[1]["val/acc1"] == res["val/teacher_acc1"]
    assert evals[0]["val/teacher_loss"] == teacher[1]["val/loss"]
    # without the flag nothing of it appears
    assert not any(k.startswith(("val/teacher", "train/kd", "train/cls_loss")) for r in _rows(students["plain"][0], "f")
                   for k in r)


def test_alpha_zero_is_the_run_without_a_teacher_and_checkpoints_hold_the_student(students):
    (a, _), (b, _), (c, _) = students["alpha0"], students["plain"], students["kd"]
    with open(os.path.join(a, "f-last.msgpack"), "rb") as fa, open(os.path.join(b, "f-last.msgpack"), "rb") as fb:
        assert fa.read() == fb.read()  # the final master, bit for bit
    ra = [r for r in _rows(a, "f") if "train/loss" in r]
    rb = [r for r in _rows(b, "f") if "train/loss" in r]
    assert [r["train/loss"] for r in ra] == [r["train/loss"] for r in rb]
    assert all(r["train/loss"] == r["train/cls_loss"] for r in ra)
    plain = flatten_tree(load_params(os.path.join(b, "f-last.msgpack")))
    kd = flatten_tree(load_params(os.path.join(c, "f-last.msgpack")))
    assert set(kd) == set(plain) and all(kd[k].shape == plain[k].shape for k in plain)
    assert any((kd[k] != plain[k]).any() for k in plain)  # the teacher did train it
    assert sorted(os.listdir(c)) == sorted(os.listdir(b)) or set(os.listdir(c)) - set(os.listdir(b)) <= {"f-best.msgpack", "f-best.state.pt"}


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_student_started_from_the_teacher_agrees_with_it(shards, teacher, tmp_path, mode):
    """The student resumes the teacher's own run (same architecture, nothing random in the forward):
    at the first step its logits are the teacher's, so the soft kd is 0 and the agreement 1 (hard: the
    cross-entropy against its own arg-max, and the agreement 1).  The teacher is rebuilt from the flag on
    a resumed run."""
    out = str(tmp_path)
    _run(shards, out, "f", ["--layers", "2", "--training-steps", "5", "--resume", teacher[0], "--teacher-ckpt",
                            teacher[0] + ".msgpack", "--distill-mode", mode, *PLAIN])
    first = next(r for r in _rows(out, "f") if "train/loss" in r)
    assert first["step"] == 5 and first["train/kd_agree"] == 1.0
    if mode == "soft":
        assert first["train/kd_loss"] == 0.0
    else:
        assert first["train/kd_loss"] > 0.0


def test_teacher_of_the_wrong_shape_fails_with_the_leaf(shards, teacher, tmp_path):
    ckpt = teacher[0] + ".msgpack"
    with pytest.raises(ValueError, match=r"shape mismatch model/\S+"):
        _run(shards, str(tmp_path), "f", STUDENT + ["--teacher-ckpt", ckpt, "--teacher-layers", "2", "--teacher-dim", "32"])
    with pytest.raises(KeyError, match=r"no leaf model/layer_2/"):
        _run(shards, str(tmp_path), "f", STUDENT + ["--teacher-ckpt", ckpt, "--teacher-layers", "3"])


def test_a_frozen_model_has_no_gradient_buffer():
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=1, dim=32, heads=2, labels=4, image_size=32, patch_size=16, posemb="learnable")
    t = FinetuneModel(vc).freeze().to("cpu", seed=1)  # (the student's seed would make its logits the student's)
    assert t.store.grad is None and t.store.num_params(True) == 0 and t.store.num_params() > 0
    s = FinetuneModel(vc).to("cpu")
    with pytest.raises(ValueError):
        s.attach_teacher(FinetuneModel(vc).to("cpu"))  # not frozen
    with pytest.raises(ValueError):
        s.attach_teacher(t, alpha=1.5)
    s.attach_teacher(t, 1.0, 2.0, "soft")
    imgs = torch.randint(0, 256, (4, 3, 32, 32), dtype=torch.uint8)
    out = s(imgs, torch.tensor([0, 1, 2, 3]))
    assert set(out) == {"loss", "acc1", "acc5", "cls_loss", "kd_loss", "kd_agree"}
    assert out["loss"].item() == out["kd_loss"].item()  # alpha 1: the teacher alone
    before = t.store.master.clone()
    out["loss"].backward()
    assert s.store.grad.abs().sum() > 0 and torch.equal(t.store.master, before)
    assert set(s.evaluate(imgs, torch.tensor([0, 1, 2, 3]))) == {"loss", "acc1", "acc5", "num_samples"}
