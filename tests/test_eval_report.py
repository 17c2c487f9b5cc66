"""The evaluation report without a GPU: the torch compositions of ops/eval_report.py against the plain-loop
reference of tests/eval_report_ref.py (exactly), the hits against ``cls_loss_torch``, batch-split and rank
invariance of the integer state, ``summary()`` on a hand-computed example, bin edges, the JSON, the flags
and the finetune driver with ``--eval-report`` on the CPU."""

import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_report_ref as R

from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.ops import eval_report as E
from jumbo_mae_tpu_amd.ops import functional as Fn
from jumbo_mae_tpu_amd.train import finetune as FT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser

N_BINS = 15


def _state_of(logits, labels, mode="ce", n_bins=N_BINS, splits=None):
    L = logits.shape[1]
    rep = E.EvalReport(L, n_bins, mode)
    for idx in (splits or [torch.arange(logits.shape[0])]):
        rep.update(logits[idx], labels[idx])
    return rep


# ------------------------------------------------------------------ definition against the loops
@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1025])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mode", ["ce", "bce"])
def test_compositions_equal_the_loop_reference(L, dtype, mode):
    z, y, names = R.structured_rows(L, dtype)
    pred, rank, conf = E.eval_rows_torch(z, y, mode)
    p_ref, r_ref, _, c_ref = R.rows_ref(z, y, mode)
    assert pred.dtype == rank.dtype == torch.int32 and conf.dtype == torch.float32
    assert pred.tolist() == p_ref and rank.tolist() == r_ref, names
    assert conf.numpy().tobytes() == np.array(c_ref, dtype=np.float32).tobytes(), names
    _, _, _, _, _, q, b = E.row_terms(y, pred, rank, conf, L, N_BINS)
    want = [R.q_and_bin(c, N_BINS) for c in c_ref]
    assert q.tolist() == [w[0] for w in want] and b.tolist() == [w[1] for w in want]
    # what the names promise
    for n, p, r in zip(names, p_ref, r_ref):
        if n in ("all -inf", "NaN row", "+inf row", "padded"):
            assert (p, r) == (-1, -1), n
        if n.startswith("max tied 2 / last"):
            assert p == 2 and r == (0 if n.endswith("label 2") else 1)
        if n.startswith("label lowest of five"):
            assert r == (1 if n.endswith("True") else 0)
        if n.startswith("label highest of five"):
            assert r == (5 if n.endswith("True") else 4)
    state = torch.zeros(E.layout(L, N_BINS)["words"], dtype=torch.int64)
    E.eval_accumulate_torch(y, pred, rank, conf, L, N_BINS, state)
    ref = R.accumulate_ref(R.zero_state(L, N_BINS), y.tolist(), p_ref, r_ref, c_ref, L, N_BINS)
    assert R.words(L, N_BINS) == state.numel() and np.array_equal(state.numpy(), ref)
    bad = 3 + (L == 1)  # all -inf, NaN, +inf; with one class the -inf element is the whole row
    assert int(state[2]) == 1 and int(state[1]) == bad and int(state[0]) == len(names) - 1 - bad


@pytest.mark.parametrize("L", [3, 8, 1000])
@pytest.mark.parametrize("mode", ["ce", "bce"])
def test_hits_equal_cls_loss(L, mode):
    """Random and structured finite rows against ``cls_loss_torch``.  Its ``topk`` leaves the order of equal
    logits to the backend, so on the rows where a tie can decide a hit (all-equal rows, the equal -60 / +60
    classes, a tied maximum, the label among five tied classes) the same composition is evaluated with a
    stable descending sort -- csrc/loss.hip's
    rule, ``cls_loss_ref.hits_stable``, the reference tests/test_cls_loss_gpu.py holds the kernel to."""
    from cls_loss_ref import hits_stable, targets32
    g = torch.Generator().manual_seed(L)
    z, y, names = R.structured_rows(L, torch.bfloat16)
    keep = [i for i, n in enumerate(names) if n not in ("all -inf", "NaN row", "+inf row", "padded")]
    names = [names[i] for i in keep] + ["random"] * 40
    z = torch.cat([z[keep].float(), (4.0 * torch.randn(40, L, generator=g)).bfloat16().float()])
    y = torch.cat([y[keep], torch.randint(0, L, (40,), generator=g)])
    _, rank, _ = E.eval_rows_torch(z, y, mode)
    h1, h5 = rank == 0, (rank >= 0) & (rank < min(5, L))
    s1, s5 = hits_stable(z, targets32(y, L))
    assert torch.equal(h1, s1) and torch.equal(h5, s5)
    _, a1, a5 = Fn.cls_loss_torch(z, y, None, 0.0, mode)
    free = torch.tensor([not any(w in n for w in ("tied", "all equal", "60")) for n in names])
    assert free.sum() >= 43 and torch.equal(h1[free], a1.bool()[free]) and torch.equal(h5[free], a5.bool()[free])


def test_state_is_invariant_under_batch_splits_and_order():
    g = torch.Generator().manual_seed(0)
    B, L = 700, 8
    z = (4.0 * torch.randn(B, L, generator=g)).bfloat16()
    y = torch.randint(-1, L, (B,), generator=g)
    z[5, 3] = float("nan")
    one = _state_of(z, y).state
    perm = torch.randperm(7, generator=g)
    seven = _state_of(z, y, splits=[torch.arange(100 * int(i), 100 * int(i) + 100) for i in perm]).state
    each = _state_of(z, y, splits=[torch.tensor([int(i)]) for i in torch.randperm(B, generator=g)]).state
    assert torch.equal(one, seven) and torch.equal(one, each)
    v = E.views(one, L, N_BINS)
    assert int(v["rows"] + v["nonfinite"] + v["padded"]) == B and int(v["padded"]) == int((y == -1).sum())
    assert int(v["confusion"].sum()) == int(v["rows"]) == int(v["count"].sum()) == int(v["bins"][:, 0].sum())
    assert torch.equal(v["confusion"].sum(1), v["count"]) and torch.equal(v["confusion"].sum(0), v["predicted"])
    assert torch.equal(v["confusion"].diagonal(), v["hit1"])


# ------------------------------------------------------------------ two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_data():
    g = torch.Generator().manual_seed(3)
    return (4.0 * torch.randn(90, 8, generator=g)).bfloat16(), torch.randint(-1, 8, (90,), generator=g)


def _gloo_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from jumbo_mae_tpu_amd.parallel import dist as pdist
    pdist.init_distributed("cpu")
    z, y = _rank_data()
    rep = E.EvalReport(8, N_BINS, "ce")
    rep.update(z[rank::world], y[rank::world])
    rep.all_reduce()
    torch.save(rep.state, os.path.join(out, f"state{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path):
    z, y = _rank_data()
    one = _state_of(z, y)
    one.all_reduce()  # nothing at world size 1
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    two = [torch.load(os.path.join(str(tmp_path), f"state{r}.pt"), weights_only=True) for r in range(2)]
    assert torch.equal(two[0], two[1]) and torch.equal(two[0], one.state)


# ------------------------------------------------------------------ summary, bins, JSON
def _hand_report():
    """3 classes, 3 bins; rows (label, pred, rank, conf): class 0: two right at 0.5 and 0.75; class 1: one
    right at 0.25, one predicted as 2 at 0.875 (rank 1); class 2: unseen; one padded, one non-finite."""
    rep = E.EvalReport(3, 3, "ce")
    y = torch.tensor([0, 0, 1, 1, -1, 2])
    pred = torch.tensor([0, 0, 1, 2, -1, -1], dtype=torch.int32)
    rank = torch.tensor([0, 0, 0, 1, -1, -1], dtype=torch.int32)
    conf = torch.tensor([0.5, 0.75, 0.25, 0.875, 0.0, 0.0])
    E.eval_accumulate(y, pred, rank, conf, 3, 3, rep.state)
    return rep


def test_summary_against_hand_computed_values():
    rep = _hand_report()
    s = rep.summary()
    # bins [0, 1/3): {0.25: hit}; [1/3, 2/3): {0.5: hit}; [2/3, 1]: {0.75: hit, 0.875: miss}
    assert rep.v["bins"].tolist() == [[1, 1, 1 << 30], [1, 1, 1 << 31], [2, 1, (3 << 30) + (7 << 29)]]
    ece = (1 / 4) * abs(1.0 - 0.25) + (1 / 4) * abs(1.0 - 0.5) + (2 / 4) * abs(0.5 - 0.8125)
    assert s == {"val/mean_class_acc1": 0.75, "val/mean_class_acc5": 1.0, "val/worst_class_acc1": 0.5, "val/ece": ece,
                 "val/mce": 0.75, "val/mean_conf": (0.5 + 0.75 + 0.25 + 0.875) / 4, "val/classes_seen": 2.0,
                 "val/nonfinite_rows": 1.0}
    assert rep.v["count"].tolist() == [2, 2, 0] and rep.v["predicted"].tolist() == [2, 1, 1]
    assert rep.confusion().tolist() == [[2, 0, 0], [0, 1, 1], [0, 0, 0]]
    assert set(rep.summary("val/ema_")) == {k.replace("val/", "val/ema_") for k in s}
    empty = E.EvalReport(3, 3).summary()
    assert empty["val/ece"] == 0.0 and empty["val/classes_seen"] == 0.0


@pytest.mark.parametrize("n_bins", [1, 3, 10, 15, 64])
def test_bin_edges(n_bins):
    """conf at k / n_bins rounded to fp32 and its two fp32 neighbours: the bin is floor(conf * n_bins) of the
    fp32 value widened exactly, so a rounded-down edge stays in the bin below; conf = 1.0 is in the last."""
    edges = torch.tensor([k / n_bins for k in range(n_bins + 1)], dtype=torch.float64).float()
    conf = torch.cat([torch.nextafter(edges, torch.tensor(-1.0)), edges, torch.nextafter(edges, torch.tensor(2.0))])
    conf = conf[(conf >= 0) & (conf <= 1)]
    assert (conf == 1.0).any()
    n = conf.numel()
    z = torch.zeros(n, dtype=torch.int32)
    _, _, _, _, _, q, b = E.row_terms(torch.zeros(n, dtype=torch.int64), z, z, conf, 2, n_bins)
    for c, qi, bi in zip(conf.tolist(), q.tolist(), b.tolist()):
        import fractions
        f = fractions.Fraction(c)  # exact
        assert bi == min(n_bins - 1, int(f * n_bins)) and (qi, bi) == R.q_and_bin(np.float32(c), n_bins)
    assert b[conf == 1.0].tolist() == [n_bins - 1]


def test_json_schema_and_confused_pairs_order():
    rep = E.EvalReport(5, 4, "ce")
    cells = {(0, 1): 3, (2, 4): 3, (1, 0): 3, (3, 3): 9, (4, 0): 1, (0, 2): 5, (2, 1): 1}
    y, p = [], []
    for (t, q), n in cells.items():
        y += [t] * n
        p += [q] * n
    n = len(y)
    pred = torch.tensor(p, dtype=torch.int32)
    rank = (pred != torch.tensor(y)).int()
    E.eval_accumulate(torch.tensor(y), pred, rank, torch.full((n,), 0.6), 5, 4, rep.state)
    j = json.loads(rep.dumps(12))
    assert set(j) == {"step", "labels", "mode", "rows", "padded", "nonfinite", "worst_class", "metrics", "bins",
                      "per_class", "confused_pairs"}
    assert (j["step"], j["labels"], j["rows"], j["padded"], j["nonfinite"]) == (12, 5, n, 0, 0)
    assert j["metrics"] == rep.summary() and j["worst_class"] == 0
    assert [set(b) for b in j["bins"]] == [{"lo", "hi", "count", "acc", "conf"}] * 4
    assert [b["count"] for b in j["bins"]] == [0, 0, n, 0] and j["bins"][0]["acc"] is None
    assert abs(j["bins"][2]["conf"] - float(np.float32(0.6))) < 1e-9
    assert (j["bins"][2]["lo"], j["bins"][2]["hi"]) == (0.5, 0.75)
    assert [set(c) for c in j["per_class"]] == [{"id", "count", "acc1", "acc5", "predicted", "top_confusion"}] * 5
    assert j["per_class"][0] == {"id": 0, "count": 8, "acc1": 0.0, "acc5": 1.0, "predicted": 4,
                                 "top_confusion": {"pred": 2, "count": 5}}
    assert j["per_class"][3]["top_confusion"] is None and j["per_class"][3]["acc1"] == 1.0
    assert [(c["true"], c["pred"], c["count"]) for c in j["confused_pairs"]] == \
        [(0, 2, 5), (0, 1, 3), (1, 0, 3), (2, 4, 3), (2, 1, 1), (4, 0, 1)]
    big = E.EvalReport(E.MATRIX_MAX_L + 1, 4)
    assert big.confusion() is None and "confusion" not in big.v and big.to_json()["confused_pairs"] == []
    assert big.state.numel() == 3 + 12 + 4 * (E.MATRIX_MAX_L + 1) == R.words(E.MATRIX_MAX_L + 1, 4)
    with pytest.raises(ValueError):
        E.EvalReport(5, 65)
    with pytest.raises(KeyError):
        E.EvalReport(5, 15, "hinge")


# ------------------------------------------------------------------ flags
def test_flags():
    a = finetune_parser().parse_args([])
    assert a.eval_report is False and a.eval_report_bins == 15
    a = finetune_parser().parse_args(["--eval-report", "--eval-report-bins", "64", "--mode", "linear"])
    assert a.eval_report is True and a.eval_report_bins == 64
    for bad in (["--eval-report-bins", "0"], ["--eval-report-bins", "65"]):
        with pytest.raises(SystemExit):
            finetune_parser().parse_args(bad)
    with pytest.raises(SystemExit):
        pretrain_parser().parse_args(["--eval-report"])


# ------------------------------------------------------------------ driver
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
          "--patch-size", "16", "--layers", "1", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--labels", "4",
          "--learning-rate", "5e-3", "--warmup-steps", "1", "--log-interval", "1", "--eval-interval", "2",
          "--training-steps", "4", "--droppath", "0.1", "--name", "f"]
OLD_VAL = ("val/loss", "val/acc1", "val/acc5")
NEW = ("mean_class_acc1", "mean_class_acc5", "worst_class_acc1", "ece", "mce", "mean_conf", "classes_seen",
       "nonfinite_rows")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=2, per_shard=11, classes=4, seed=1, prefix="valid")
    outs = {}
    for name, extra in (("plain", []), ("report", ["--eval-report", "--eval-report-bins", "5"]),
                        ("ema", ["--eval-report", "--ema-decay", "0.5"]), ("ema_plain", ["--ema-decay", "0.5"])):
        out = str(tmp_path_factory.mktemp(name))
        args = finetune_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", valid,
                                                      "--output-dir", out, *extra])
        outs[name] = (out, FT.main(args))
    outs["valid"] = valid
    return outs


def _evals(out):
    rows = [json.loads(line) for line in open(os.path.join(out, "f-metrics.jsonl"))]
    return [r for r in rows if "val/loss" in r]


def test_driver_writes_the_files_and_the_report_agrees_with_acc1(runs):
    out, res = runs["report"]
    evals = _evals(out)
    assert [r["step"] for r in evals] == [0, 2, 4]  # the sanity evaluation included
    for r in evals:
        assert all("val/" + k in r for k in NEW)
        j = json.load(open(os.path.join(out, f"f-report-{r['step']:07d}.json")))
        cm = np.load(os.path.join(out, f"f-confusion-{r['step']:07d}.npy"))
        assert j["step"] == r["step"] and j["rows"] == 22 and j["nonfinite"] == 0 and len(j["bins"]) == 5
        assert cm.shape == (4, 4) and cm.dtype == np.int64 and int(cm.sum()) == 22
        assert sum(c["count"] for c in j["per_class"]) == 22
        hit1 = sum(round(c["acc1"] * c["count"]) for c in j["per_class"] if c["count"])
        assert hit1 == int(np.trace(cm)) and hit1 / j["rows"] == r["val/acc1"]
        assert j["metrics"] == {"val/" + k: r["val/" + k] for k in NEW}
        assert 0.0 <= r["val/ece"] <= r["val/mce"] <= 1.0 and r["val/classes_seen"] == 4.0
    assert all("val/" + k in res for k in NEW)
    assert not any(f.endswith((".json", ".npy")) and ("report" in f or "confusion" in f)
                   for f in os.listdir(runs["plain"][0]))


@pytest.mark.parametrize("a, b", [("report", "plain"), ("ema", "ema_plain")])
def test_driver_flag_changes_nothing_else(runs, a, b):
    (oa, _), (ob, _) = runs[a], runs[b]
    for f in ("f-last.msgpack", "f-best.msgpack"):
        pa, pb = os.path.join(oa, f), os.path.join(ob, f)
        assert os.path.exists(pa) == os.path.exists(pb)
        if os.path.exists(pa):
            assert open(pa, "rb").read() == open(pb, "rb").read(), f
    ea, eb = _evals(oa), _evals(ob)
    keys = OLD_VAL + (tuple(k.replace("val/", "val/ema_") for k in OLD_VAL) if a == "ema" else ())
    assert [[r[k] for k in keys] for r in ea] == [[r[k] for k in keys] for r in eb]
    assert not any(k.split("/")[-1] in NEW for r in eb for k in r)


def test_driver_ema_report(runs):
    out, res = runs["ema"]
    for r in _evals(out):
        assert all("val/ema_" + k in r and "val/" + k in r for k in NEW)
        j = json.load(open(os.path.join(out, f"f-ema-report-{r['step']:07d}.json")))
        assert j["metrics"] == {"val/ema_" + k: r["val/ema_" + k] for k in NEW}
        assert os.path.exists(os.path.join(out, f"f-ema-confusion-{r['step']:07d}.npy"))
        hit1 = sum(round(c["acc1"] * c["count"]) for c in j["per_class"] if c["count"])
        assert hit1 / j["rows"] == r["val/ema_acc1"]


# ------------------------------------------------------------------ tool
def test_eval_report_tool(runs, tmp_path, capsys):
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_report_tool", os.path.join(root, "tools", "eval_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, res = runs["report"]
    path, rows = str(tmp_path / "report.json"), str(tmp_path / "rows.npz")
    j = tool.main(DRIVER + ["--ckpt", os.path.join(out, "f-last.msgpack"), "--valid-dataset-shards", runs["valid"],
                            "--eval-report-bins", "5", "--out", path, "--dump-rows", rows])
    last = json.load(open(os.path.join(out, "f-report-0000004.json")))
    assert json.load(open(path)) == j
    assert j["metrics"]["val/acc1"] == res["val/acc1"] and j["metrics"]["val/loss"] == res["val/loss"]
    for k in ("rows", "padded", "nonfinite", "bins", "per_class", "confused_pairs", "worst_class"):
        assert j[k] == last[k], k
    z = np.load(rows)
    assert set(z.files) == {"label", "pred", "rank", "conf"}
    assert all(z[k].shape == (z["label"].shape[0],) for k in z.files)
    assert int((z["label"] != -1).sum()) == 22 and int((z["rank"] == 0).sum()) == round(res["val/acc1"] * 22)
    text = capsys.readouterr().out
    assert "val/ece" in text and "worst classes" in text
