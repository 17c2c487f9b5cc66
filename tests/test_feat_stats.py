"""Representation monitor on the CPU: the torch compositions (ops/feat_stats.py, the oracles of
csrc/feat_stats.hip) against plain loops, ``summary`` on closed forms, the ``--feat-stats`` flag of
``main_pretrain`` (one process and two gloo ranks, with and without validation labels) and
tools/feat_stats.py."""

import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import feat_stats_ref as FR
import knn_ref as KR
from jumbo_mae_tpu_amd.ckpt.checkpoint import load_params
from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
from jumbo_mae_tpu_amd.ops import feat_stats as FS
from jumbo_mae_tpu_amd.ops import knn as K
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.train import pretrain as PT
from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser

KEYS = {"val/feat_rankme", "val/feat_pr", "val/feat_top1_var", "val/feat_std", "val/feat_rms_norm",
        "val/feat_uniformity", "val/feat_rows", "val/feat_nonfinite"}


# ------------------------------------------------------------------ compositions
def test_gram_composition_equals_the_loops():
    x = FR.exact_rows(37, 24, seed=0)
    valid = torch.arange(37) % 3 != 1
    bad = x.clone()
    bad[~valid] = float("nan")  # a NaN row behind the mask is selected out
    G, s, n, _ = FR.gram_loops(x, valid)
    for dtype in (torch.float64, torch.float32):  # exactly summable: no rounding in either precision
        st = FS.feat_gram_torch(bad, valid, FS.new_state(24, "cpu"), dtype=dtype)
        assert torch.equal(st["G"], G) and torch.equal(st["s"], s) and float(st["n"]) == n == 25
    # the dispatcher on the CPU is the composition; two batches add up; n = 0 changes nothing
    st = FS.feat_gram(bad[:20], valid[:20], FS.new_state(24, "cpu"))
    st = FS.feat_gram(bad[20:], valid[20:], st)
    st = FS.feat_gram(bad[:0], valid[:0], st)
    st = FS.feat_gram(bad, torch.zeros(37, dtype=torch.bool), st)
    assert torch.equal(st["G"], G) and torch.equal(st["s"], s) and float(st["n"]) == 25
    # a strided view
    wide = torch.full((37, 40), float("nan"))
    wide[:, 3:27] = x
    st = FS.feat_gram(wide[:, 3:27], valid, FS.new_state(24, "cpu"))
    assert torch.equal(st["G"], G) and torch.equal(st["s"], s)
    # random values, no mask: fp64 against the correctly rounded loops
    g = torch.Generator().manual_seed(1)
    r = torch.randn(19, 7, generator=g)
    G, s, n, S = FR.gram_loops(r)
    st = FS.feat_gram(r, None, FS.new_state(7, "cpu"))
    assert ((st["G"] - G).abs() <= n * 2.0 ** -53 * S).all() and float(st["n"]) == 19
    with pytest.raises(ValueError, match="x must be"):
        FS.feat_gram(r, None, FS.new_state(8, "cpu"))


def test_uniformity_composition_equals_the_loops():
    q, bank = KR.exact_inputs(23, 41, 32, seed=2)
    g = torch.Generator().manual_seed(2)
    self_idx = torch.randint(-1, 41, (23,), generator=g)
    bank_valid = torch.rand(41, generator=g) < 0.7
    bad = bank.clone()
    bad[~bank_valid] = float("nan")
    for si, bv, b in ((None, None, bank), (self_idx, None, bank), (None, bank_valid, bad), (self_idx, bank_valid, bad)):
        ref = FR.uniformity_loops(q, b, si, bv, 2.0)
        e = FS.feat_uniformity_torch(q, b, si, bv, 2.0, dtype=torch.float64, block_elems=300)
        assert e.dtype == torch.float64 and torch.allclose(e, ref, rtol=1e-14, atol=0)
        assert torch.allclose(FS.feat_uniformity(q, b, si, bv, 2.0), ref, rtol=1e-14, atol=0)  # the CPU path: fp64
    # n = 0 on either side, a bank that is masked entirely, a strided view
    assert FS.feat_uniformity(q[:0], bank).shape == (0,)
    assert not FS.feat_uniformity(q, bank[:0]).any()
    assert not FS.feat_uniformity(q, bank, None, torch.zeros(41, dtype=torch.bool)).any()
    wide = torch.zeros(41, 64, dtype=torch.bfloat16)
    wide[:, 16:48] = bank
    assert torch.equal(FS.feat_uniformity_torch(q, wide[:, 16:48], self_idx, None, 0.5, dtype=torch.float64),
                       FS.feat_uniformity_torch(q, bank, self_idx, None, 0.5, dtype=torch.float64))
    with pytest.raises(ValueError, match="t must be positive"):
        FS.feat_uniformity(q, bank, t=0.0)


def test_switch_exists():
    assert P._FEAT_STATS_OURS is True


# ------------------------------------------------------------------ summary
def _state(x):
    st = FS.feat_gram_torch(x, None, FS.new_state(x.shape[1], "cpu"))
    return st["G"], st["s"], int(st["n"])


def _uniformity_terms(x, t):
    f = K.normalize_features(x)
    n = f.shape[0]
    e = FS.feat_uniformity_torch(f, f, torch.arange(n), None, t, dtype=torch.float64)
    return float(e.sum()), float(n * (n - 1))


def _rankme(sig, m):
    sig = sorted(sig, reverse=True)[:m]
    p = [v / sum(sig) + 1e-7 for v in sig]
    return math.exp(-sum(v * math.log(v) for v in p))


@pytest.mark.parametrize("r,D,reps", [(1, 8, 2), (3, 8, 1), (5, 16, 4), (16, 16, 2)])
def test_summary_equal_energy_directions(r, D, reps):
    """Rows +a e_k and -a e_k for k < r, ``reps`` times: mean zero, C = G / n has r equal eigenvalues."""
    a = 3.0
    rows = torch.cat([a * torch.eye(D)[:r], -a * torch.eye(D)[:r]]).repeat(reps, 1)
    n = rows.shape[0]
    out = FS.summary(*_state(rows))
    assert out["val/feat_rows"] == n and out["val/feat_nonfinite"] == 0
    assert abs(out["val/feat_pr"] - r) <= 1e-12 * r
    assert abs(out["val/feat_top1_var"] - 1.0 / r) <= 1e-12
    # r equal singular values and min(n, D) - r zeros
    sigma = a * math.sqrt(n / r)
    want = _rankme([sigma] * r + [0.0] * (D - r), min(n, D))
    assert abs(out["val/feat_rankme"] - want) <= 1e-12 * want
    assert abs(out["val/feat_rms_norm"] - a) <= 1e-12 * a
    assert abs(out["val/feat_std"] - r * a / math.sqrt(r) / D) <= 1e-12  # r dimensions with variance a^2 / r
    assert "val/feat_uniformity" not in out  # pairs == 0: left out


def test_summary_identical_rows():
    """One row n times: no variance at all.  feat_std is 0, feat_pr and feat_top1_var are left out (no
    eigenvalue of C above its rounding level), the uniformity of coinciding points is 0."""
    g = torch.Generator().manual_seed(3)
    row = torch.randn(1, 24, generator=g)
    x = row.repeat(13, 1)
    out = FS.summary(*_state(x), *_uniformity_terms(FR.exact_rows(1, 32, seed=5).abs().add(0.125).repeat(13, 1), 2.0))
    assert out["val/feat_std"] == 0.0
    assert "val/feat_pr" not in out and "val/feat_top1_var" not in out
    assert abs(out["val/feat_uniformity"]) <= 4 * 2.0 * 2.0 ** -8  # bf16 unit rows: |1 - s| <= 2^-8 or so
    assert abs(out["val/feat_rankme"] - _rankme([1.0] + [0.0] * 12, 13)) <= 1e-6  # one direction
    assert all(math.isfinite(v) for v in out.values())
    # rows whose normalised bf16 form has norm exactly 1: exactly 0
    one = torch.zeros(1, 32)
    one[0, 3] = 2.5
    e_sum, pairs = _uniformity_terms(one.repeat(7, 1), 2.0)
    assert FS.summary(*_state(one.repeat(7, 1)), e_sum, pairs)["val/feat_uniformity"] == 0.0


@pytest.mark.parametrize("t", [0.5, 2.0])
def test_summary_orthogonal_unit_rows(t):
    x = torch.eye(32)[:9] * 4.0  # normalised by the monitor's own step
    out = FS.summary(*_state(x), *_uniformity_terms(x, t))
    assert abs(out["val/feat_uniformity"] + 2 * t) <= 1e-12


def test_summary_takes_min_n_D_values_and_handles_no_rows():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 12, generator=g)  # n < D: 5 singular values enter, not 12
    out = FS.summary(*_state(x))
    sv = torch.linalg.svdvals(x.double()).tolist()
    assert abs(out["val/feat_rankme"] - _rankme(sv, 5)) <= 1e-9
    assert abs(out["val/feat_rankme"] - _rankme(sv + [0.0] * 7, 12)) > 1e-7  # the 7 zeros would show
    assert FS.summary(torch.zeros(4, 4), torch.zeros(4), 0, 0.0, 0.0, 3) == {"val/feat_rows": 0.0,
                                                                          "val/feat_nonfinite": 3.0}
    zero = FS.summary(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), 6, 0.0, 30.0)
    assert "val/feat_uniformity" not in zero  # every term underflowed: no -inf in the log
    assert set(FS.summary(*_state(x), 3.0, 20.0)) == set(FS.KEYS) == KEYS
    assert "val/feat_rankme" not in zero and zero["val/feat_std"] == 0.0 and zero["val/feat_rms_norm"] == 0.0


def _four_decades():
    """fp32 [96, 48] with singular values 10^0 .. 10^-4, log-spaced."""
    g = torch.Generator().manual_seed(7)
    U, _ = torch.linalg.qr(torch.randn(96, 48, generator=g, dtype=torch.float64))
    V, _ = torch.linalg.qr(torch.randn(48, 48, generator=g, dtype=torch.float64))
    sv = torch.logspace(0, -4, 48, dtype=torch.float64)
    return ((U * sv) @ V.t()).float()


def test_rankme_against_svdvals_over_four_decades():
    """RankMe from eigvalsh of the fp64 Gram matrix against RankMe from ``torch.linalg.svdvals`` of
    the fp64 feature matrix.  Measured disagreement between the two fp64 routes on this fixture, on the
    CPU: 1.1e-11 absolute (rankme = 13.88); the tolerance is ten times that.  An fp32 Gram matrix is off
    by 5.2e-4 on the same fixture, which is what the fp64 state is for."""
    x = _four_decades()
    G, s, n = _state(x)
    got = FS.summary(G, s, n)["val/feat_rankme"]
    want = _rankme(torch.linalg.svdvals(x.double()).tolist(), 48)
    print(f"rankme: eigvalsh(G) {got!r}, svdvals {want!r}, |diff| {abs(got - want):.3e}")
    assert abs(got - want) <= 1.1e-10
    st32 = FS.feat_gram_torch(x, None, FS.new_state(48, "cpu"), dtype=torch.float32)
    assert abs(FS.summary(st32["G"], st32["s"], n)["val/feat_rankme"] - want) > 1e-4


# ------------------------------------------------------------------ driver
S = 32
DRIVER = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", str(S),
          "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
          "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cpu",
          "--train-batch-size", "8", "--valid-batch-size", "8", "--auto-augment", "none", "--augment-repeats", "1",
          "--labels", "0", "--dec-layers", "1", "--dec-dim", "64", "--dec-heads", "2", "--learning-rate", "5e-3",
          "--training-steps", "2", "--warmup-steps", "1", "--log-interval", "1", "--eval-interval", "2",
          "--droppath", "0.1", "--dec-droppath", "0.1", "--name", "p"]


def test_flags_are_pretrain_only_off_by_default_and_checked_early():
    a = pretrain_parser().parse_args([])
    assert a.feat_stats is False and a.feat_uniformity_t == 2.0
    a = pretrain_parser().parse_args(["--feat-stats", "--feat-uniformity-t", "0.5"])
    assert a.feat_stats is True and a.feat_uniformity_t == 0.5
    with pytest.raises(SystemExit):
        finetune_parser().parse_args(["--feat-stats"])
    for bad in ("0", "-1", "nan"):
        with pytest.raises(ValueError, match="--feat-uniformity-t must be positive"):
            PT.main(pretrain_parser().parse_args(["--feat-stats", "--feat-uniformity-t", bad]))  # before any work


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jpeg"))
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=2, per_shard=11, classes=4, seed=1, prefix="valid")
    return train, valid


def _strip_labels(pattern, out_dir):
    """Copies of the shards without their .cls members: a validation set that has no labels."""
    import tarfile

    from jumbo_mae_tpu_amd.data.shards import shard_list

    os.makedirs(out_dir, exist_ok=True)
    names = []
    for i, src in enumerate(shard_list(pattern)):
        dst = os.path.join(out_dir, f"nolabel-{i:06d}.tar")
        with tarfile.open(src) as tin, tarfile.open(dst, "w") as tout:
            for m in tin.getmembers():
                if not m.name.endswith(".cls"):
                    tout.addfile(m, tin.extractfile(m))
        names.append(dst)
    return os.path.join(out_dir, "nolabel-{%06d..%06d}.tar" % (0, len(names) - 1))


@pytest.fixture(scope="module")
def runs(shards, tmp_path_factory):
    train, valid = shards
    nolabel = _strip_labels(valid, str(tmp_path_factory.mktemp("nolabel")))
    outs = {}
    for name, v, extra in (("with", valid, ["--feat-stats"]), ("without", valid, []),
                           ("both", valid, ["--feat-stats", "--knn-k", "5"]), ("knn", valid, ["--knn-k", "5"]),
                           ("nolabel", nolabel, ["--feat-stats"])):
        out = str(tmp_path_factory.mktemp(name))
        args = pretrain_parser().parse_args(DRIVER + ["--train-dataset-shards", train, "--valid-dataset-shards", v,
                                                      "--output-dir", out, *extra])
        outs[name] = (out, PT.main(args))
    return outs


def _rows(out):
    return [json.loads(line) for line in open(os.path.join(out, "p-metrics.jsonl"))]


def test_driver_logs_the_keys_at_every_evaluation(runs):
    for name in ("with", "both", "nolabel"):
        out, res = runs[name]
        rows = [r for r in _rows(out) if "val/loss" in r]
        assert len(rows) == 2  # the sanity evaluation and the last step
        for r in rows + [res]:
            assert KEYS <= set(r), (name, sorted(r))
            assert r["val/feat_rows"] == 22 and r["val/feat_nonfinite"] == 0
            assert 1.0 <= r["val/feat_rankme"] <= 22 and 1.0 <= r["val/feat_pr"] <= 21 + 1e-9
            assert 0.0 < r["val/feat_top1_var"] <= 1.0 and r["val/feat_std"] > 0 and r["val/feat_rms_norm"] > 0
            assert math.isfinite(r["val/feat_uniformity"])
    # with --knn-k as well: both monitors, each with the numbers it has alone
    both, knn, alone = _rows(runs["both"][0]), _rows(runs["knn"][0]), _rows(runs["with"][0])
    for rb, rk, ra in zip(*[[r for r in rows if "val/loss" in r] for rows in (both, knn, alone)]):
        assert rb["val/knn_acc1"] == rk["val/knn_acc1"] and rb["val/knn_acc5"] == rk["val/knn_acc5"]
        assert all(rb[k] == ra[k] for k in KEYS)


def test_driver_without_labels_sees_the_same_features(runs):
    lab = [r for r in _rows(runs["with"][0]) if "val/loss" in r]
    nol = [r for r in _rows(runs["nolabel"][0]) if "val/loss" in r]
    for a, b in zip(lab, nol):  # same images, same weights: the labels play no part
        assert all(a[k] == b[k] for k in KEYS)


def test_driver_without_the_flag_is_untouched(runs):
    out, res = runs["without"]
    assert not any(k.startswith("val/feat_") for r in _rows(out) for k in r)
    assert not any(k.startswith("val/feat_") for k in res)
    wout = runs["with"][0]
    assert open(os.path.join(out, "p-last.msgpack"), "rb").read() == open(os.path.join(wout, "p-last.msgpack"), "rb").read()
    a = flatten_tree(load_params(os.path.join(out, "p-last.msgpack")))
    b = flatten_tree(load_params(os.path.join(wout, "p-last.msgpack")))
    assert set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    ra, rb = _rows(out), _rows(wout)
    assert len(ra) == len(rb)
    skip = ("perf/", "train_time", "time", "config")
    for x, y in zip(ra, rb):  # every logged value but the clocks and the flags, and nothing new but val/feat_*
        assert {k: v for k, v in x.items() if not k.startswith(skip)} == \
            {k: v for k, v in y.items() if not k.startswith(skip) and not k.startswith("val/feat_")}


# ------------------------------------------------------------------ two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _monitor_inputs():
    """fp32 rows from tests/knn_ref.py exact_inputs (exactly summable), 45 of them: 3 padding rows, 1 NaN row."""
    _, bank = KR.exact_inputs(1, 45, 32, seed=11)
    x = bank.float() + 0.0
    valid = torch.ones(45, dtype=torch.bool)
    valid[torch.tensor([4, 20, 44])] = False
    x[7, 3] = float("nan")
    return x, valid


def _monitor_run(x, valid, batch):
    mon = PT.FeatMonitor(2.0)
    for r0 in range(0, x.shape[0], batch):
        mon.update(x[r0:r0 + batch], None, valid[r0:r0 + batch])
    out = mon.finish()
    return out, {k: v.clone() for k, v in mon.state.items()}


def _gloo_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from jumbo_mae_tpu_amd.parallel import dist as pdist
    pdist.init_distributed("cpu")
    x, valid = _monitor_inputs()
    sl = slice(0, 25) if rank == 0 else slice(25, 45)  # shards of different length: one is padded in the gather
    torch.save(_monitor_run(x[sl], valid[sl], 8), os.path.join(out, f"res{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(tmp_path):
    x, valid = _monitor_inputs()
    one, st1 = _monitor_run(x, valid, 16)
    assert one["val/feat_rows"] == 41 and one["val/feat_nonfinite"] == 1 and KEYS <= set(one)
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    two = [torch.load(os.path.join(str(tmp_path), f"res{r}.pt"), weights_only=True) for r in range(2)]
    assert two[0][0] == two[1][0]
    for k in ("G", "s", "n"):  # exactly summable: the all-reduced state is bit-equal
        assert torch.equal(two[0][1][k], st1[k]) and torch.equal(two[1][1][k], st1[k])
    for k in one:
        assert abs(two[0][0][k] - one[k]) <= 1e-12 * abs(one[k]), (k, one[k], two[0][0][k])


# ------------------------------------------------------------------ tool
def test_feat_stats_tool(shards, capsys):
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("feat_stats_tool", os.path.join(root, "tools", "feat_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, valid = shards
    model = [a for a in DRIVER if a not in ("--name", "p")]
    row = tool.main(model + ["--valid-dataset-shards", valid])
    assert KEYS <= set(row) and row["val/feat_rows"] == 22 and row["D"] == 192
    # the monitor's numbers at the sanity evaluation of the same initialization
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.utils.rng import RngStreams

    args = pretrain_parser().parse_args(DRIVER + ["--valid-dataset-shards", valid, "--feat-stats"])
    device = torch.device("cpu")
    net = PT.build_model(args, device, torch.float32)
    _, loader = create_dataloaders(args, 0, 1, 0, device_augment=False, device_valid=False)
    res = PT.evaluate(net, loader, RngStreams({"mixup": 0, "dropout": 0, "noise": 0}, 0, device), device, 0, 0.07, None,
                      True, 2.0)
    assert all(abs(res[k] - row[k]) <= 1e-9 * max(1.0, abs(res[k])) for k in KEYS)
    rnd = tool.main(["--random-rows", "50", "--dim", "32", "--device", "cpu"])
    assert rnd["D"] == 96 and rnd["val/feat_rows"] == 50
    assert len(capsys.readouterr().out.strip().splitlines()) == 2  # one JSON line per run
