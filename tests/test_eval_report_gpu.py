"""The evaluation-report kernels (csrc/eval_report.hip) on the GPU.

``jm_eval_rows`` against the definition evaluated in fp64 on the CPU (``eval_rows_torch`` on the same,
already rounded logits): ``pred``, ``rank`` and the non-finite flag (``pred == -1``) exactly; ``conf`` within
max(2 x the error of the fp32 torch composition on the same input, 1 fp32 ulp) of the unrounded fp64 value --
the rule of tests/test_cls_loss_gpu.py: the bound comes from the path being replaced, never from the kernel.
Every case runs twice and must be bit-identical.

``jm_eval_accumulate`` on hand-built per-row inputs against the plain-loop reference of
tests/eval_report_ref.py: every state word exactly.

Model and driver level: the report of ``FinetuneModel.evaluate`` and of ``main_finetune --eval-report``."""

import json
import os

import numpy as np
import pytest
import torch

import eval_report_ref as R
from cls_loss_ref import ulp32

from jumbo_mae_tpu_amd.ops import eval_report as E

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _check_rows(z, y, mode, what):
    """The row kernel on GPU tensors (``z`` maybe a view), twice, against the fp64 oracle; returns its outputs."""
    ext = _ext()
    a = ext.eval_rows(z, y, E.MODES.index(mode))
    b = ext.eval_rows(z, y, E.MODES.index(mode))
    torch.cuda.synchronize()
    pred, rank, conf = a
    assert pred.dtype == rank.dtype == torch.int32 and conf.dtype == torch.float32
    assert all(t.shape == (z.shape[0],) for t in a)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), what
    zc, yc = z.cpu(), y.cpu()
    p64, r64, c64 = E.eval_rows_torch(zc, yc, mode, torch.float64, round_conf=False)
    _, _, c32 = E.eval_rows_torch(zc, yc, mode, torch.float32, round_conf=False)
    assert torch.equal(pred.cpu(), p64) and torch.equal(rank.cpu(), r64), what
    err = (conf.cpu().double() - c64).abs()
    bound = torch.maximum(2.0 * (c32.double() - c64).abs(), ulp32(c64))
    worst = (err / bound).max().item()
    print(f"{what}: conf err / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst, int((err / bound).argmax()))
    assert ((conf >= 0) & (conf <= 1)).all() and (conf[pred < 0] == 0).all()
    return pred, rank, conf


# L = 1, 3, 8; 1000: the presets; 1003: odd row bases; 1024 / 1025: the last wave-per-row length and the first
# workgroup-per-row one; 21841: many passes per thread
SHAPES = [(B, L) for B in (1, 3, 130) for L in (1, 3, 8, 1000, 1003)] + [(3, 1024), (3, 1025), (2, 21841)]


@pytest.mark.parametrize("B, L", SHAPES)
def test_rows_random_logits(B, L):
    gen = torch.Generator().manual_seed(1000 * B + L)
    z = 4.0 * torch.randn(B, L, generator=gen)
    y = torch.randint(0, L, (B,), generator=gen)
    for dtype in DTYPES:
        for mode in E.MODES:
            _check_rows(z.to(dtype).cuda(), y.cuda(), mode, f"B={B} L={L} {str(dtype)[6:]} {mode}")


@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1025])
def test_rows_structured(L):
    for dtype in DTYPES:
        z, y, names = R.structured_rows(L, dtype)
        for mode in E.MODES:
            pred, rank, conf = _check_rows(z.cuda(), y.cuda(), mode, f"structured L={L} {str(dtype)[6:]} {mode}")
            p_ref, r_ref, _, _ = R.rows_ref(z, y, mode)  # the loops as well
            assert pred.tolist() == p_ref and rank.tolist() == r_ref
            for n, p in zip(names, pred.tolist()):
                assert (p == -1) == (n in ("all -inf", "NaN row", "+inf row", "padded") or
                                     (L == 1 and n == "-inf element")), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_strided_views_equal_the_contiguous_copy(dtype):
    """Column slices of wider [B, L + 24] buffers at odd element offsets, NaN around them."""
    from jumbo_mae_tpu_amd.ops import functional as Fn
    gen = torch.Generator().manual_seed(5)
    for B, L in ((5, 1000), (3, 1025), (6, 8)):
        z = (4.0 * torch.randn(B, L, generator=gen)).to(dtype)
        y = torch.randint(0, L, (B,), generator=gen).cuda()
        buf = torch.full((B, L + 24), float("nan"), dtype=dtype, device="cuda")
        buf[:, 3:3 + L] = z.cuda()
        view = buf[:, 3:3 + L]
        assert view.stride(0) == L + 24 and not view.is_contiguous() and view.storage_offset() % 2 == 1
        assert Fn._rows_ok(view)
        for mode in E.MODES:
            a = _check_rows(view, y, mode, f"view {B}x{L} {mode}")
            b = _check_rows(z.cuda(), y, mode, f"dense {B}x{L} {mode}")
            c = E.eval_rows(view, y, mode)  # the op takes the view as it is
            for u, v, w in zip(a, b, c):
                assert torch.equal(u, v) and torch.equal(u, w)
            assert (a[0] >= 0).all()


def test_rows_bad_arguments():
    ext = _ext()
    z, y = torch.randn(4, 10, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for bad in [(z.half(), y, 0), (z.cpu(), y.cpu(), 0), (z, y[:-1], 0), (z, y.int(), 0), (z[0], y, 0), (z, y, 2),
                (torch.randn(10, 4, device="cuda").t(), y, 0)]:
        with pytest.raises((RuntimeError, TypeError)):
            ext.eval_rows(*bad)
    st = torch.zeros(E.layout(10, 15)["words"], dtype=torch.int64, device="cuda")
    p, r, c = ext.eval_rows(z, y, 0)
    for bad in [(y, p, r, c, 10, 0, st), (y, p, r, c, 10, 65, st), (y, p, r, c, 11, 15, st),
                (y, p.long(), r, c, 10, 15, st), (y, p, r, c[:-1], 10, 15, st), (y, p, r, c, 10, 15, st.int())]:
        with pytest.raises((RuntimeError, TypeError)):
            ext.eval_accumulate(*bad)
    assert not st.any().item()


# ------------------------------------------------------------------------------------ accumulation
def _hand_rows(B, L, gen, kind="random", n_bins=15):
    """(labels int64, pred int32, rank int32, conf fp32) built by hand, on the CPU."""
    if kind == "random":
        y = torch.randint(-1, L + 1, (B,), generator=gen)  # -1 padded, L clamped
        pred = torch.randint(-1, L, (B,), generator=gen)  # -1 non-finite
        rank = torch.randint(0, min(L, 8), (B,), generator=gen)
        conf = torch.rand(B, generator=gen)
    elif kind == "one cell":
        y, pred = torch.full((B,), L - 1), torch.full((B,), L // 2)
        rank, conf = torch.ones(B, dtype=torch.int64), torch.rand(B, generator=gen)
    elif kind == "padding":
        y, pred = torch.full((B,), -1), torch.randint(-1, L, (B,), generator=gen)
        rank, conf = torch.zeros(B, dtype=torch.int64), torch.rand(B, generator=gen)
    else:  # bin edges: k / n_bins rounded to fp32, its two neighbours, conf = 1.0
        e = torch.tensor([k / n_bins for k in range(n_bins + 1)], dtype=torch.float64).float()
        conf = torch.cat([torch.nextafter(e, torch.tensor(-1.0)), e, torch.nextafter(e, torch.tensor(2.0))])
        conf = conf[(conf >= 0) & (conf <= 1)]
        conf = conf[torch.arange(B) % conf.numel()]
        y, pred = torch.randint(0, L, (B,), generator=gen), torch.randint(0, L, (B,), generator=gen)
        rank = (y != pred).long()
    return y.long(), pred.int(), rank.int(), conf.float()


def _check_accumulate(batches, L, n_bins, what):
    """The batches into one zeroed state, twice; every word against the loops."""
    ext = _ext()
    words = E.layout(L, n_bins)["words"]
    assert words == R.words(L, n_bins)
    got = []
    for _ in range(2):
        st = torch.zeros(words, dtype=torch.int64, device="cuda")
        for y, p, r, c in batches:
            ext.eval_accumulate(y.cuda(), p.cuda(), r.cuda(), c.cuda(), L, n_bins, st)
        torch.cuda.synchronize()
        got.append(st.cpu())
    assert torch.equal(got[0], got[1]), what
    ref = R.zero_state(L, n_bins)
    for y, p, r, c in batches:
        R.accumulate_ref(ref, y.tolist(), p.tolist(), r.tolist(), c.numpy(), L, n_bins)
    bad = np.flatnonzero(got[0].numpy() != ref)
    assert bad.size == 0, (what, bad[:8], got[0].numpy()[bad[:8]], ref[bad[:8]])
    return got[0]


@pytest.mark.parametrize("L", [1, 3, 8, 1000, 1025])
def test_accumulate_random(L):
    gen = torch.Generator().manual_seed(L)
    for B in (1, 5, 130, 700):
        for n_bins in ((15,) if B != 130 else (1, 15, 64)):
            # two consecutive batches into one state
            batches = [_hand_rows(B, L, gen), _hand_rows(max(1, B // 2), L, gen)]
            st = _check_accumulate(batches, L, n_bins, f"random B={B} L={L} bins={n_bins}")
            assert int(st[:3].sum()) == B + max(1, B // 2)


@pytest.mark.parametrize("kind", ["one cell", "padding", "bin edges"])
def test_accumulate_special(kind):
    gen = torch.Generator().manual_seed(11)
    for B, L in ((700, 8), (300, 1000), (130, 1025), (5, 3)):
        st = _check_accumulate([_hand_rows(B, L, gen, kind), _hand_rows(B, L, gen, kind)], L, 15, f"{kind} B={B} L={L}")
        v = E.views(st, L, 15)
        if kind == "one cell":
            assert int(v["confusion"][L - 1, L // 2]) == 2 * B == int(v["rows"]) == int(v["confusion"].sum())
        if kind == "padding":
            assert int(v["padded"]) == 2 * B == int(st.sum())
        if kind == "bin edges":
            assert int(v["bins"][:, 0].sum()) == 2 * B
            if B >= 100:  # every edge value is in, conf = 1.0 among them (47 values at 15 bins)
                assert int(v["bins"][-1, 0]) > 0 and bool((v["bins"][:, 0] > 0).all())


@pytest.mark.parametrize("L", [4096, 4097])
def test_accumulate_matrix_cap(L):
    """The matrix kept (4096 classes) and not kept (4097)."""
    y = torch.tensor([L - 1, 7]).long()
    rows = (y, torch.tensor([L - 1, 300], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32),
            torch.tensor([1.0, 0.26]))
    st = _check_accumulate([rows, rows], L, 15, f"cap L={L}")
    v = E.views(st, L, 15)
    assert ("confusion" in v) == (L == 4096) and st.numel() == 3 + 45 + 4 * L + (L * L if L == 4096 else 0)
    assert int(v["predicted"][300]) == 2 and int(v["hit5"].sum()) == 4
    if L == 4096:
        assert int(v["confusion"][L - 1, L - 1]) == 2 and int(v["confusion"][7, 300]) == 2


# ------------------------------------------------------------------------------------ model level
@pytest.fixture(autouse=True)
def own_step_feeder(monkeypatch):
    """As in tests/test_distill_gpu.py: the step feeder's static buffers are per process and sized by their
    first use."""
    from jumbo_mae_tpu_amd.runtime import feeder
    monkeypatch.setattr(feeder, "_FEEDERS", {})


class _Capture(E.EvalReport):
    def update(self, logits, labels):
        self.seen = (logits.detach().clone(), labels.clone())
        super().update(logits, labels)


def test_model_evaluate_fills_the_report(monkeypatch):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.ops import prims as P
    L, B = 8, 16
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (B, 3, 32, 32), dtype=torch.uint8, generator=g).cuda()
    labels = torch.randint(0, L, (B,), generator=g)
    labels[3] = labels[9] = -1
    labels = labels.cuda()
    model = FinetuneModel(ViTConfig(layers=2, dim=64, heads=2, labels=L, image_size=32, patch_size=16,
                                    posemb="learnable")).to("cuda", torch.bfloat16, seed=0)
    plain = model.evaluate(imgs, labels)
    reps = {}
    for on in (True, False):
        monkeypatch.setattr(P, "_EVAL_REPORT_OURS", on)
        rep = _Capture(L, 15, "ce", "cuda")
        out = model.evaluate(imgs, labels, None, report=rep)
        torch.cuda.synchronize()
        assert {k: v.item() for k, v in out.items()} == {k: v.item() for k, v in plain.items()}
        reps[on] = (rep, out)
    rep, out = reps[True]
    z, y = rep.seen
    assert z.dtype == torch.bfloat16 and z.shape == (B, L) and torch.equal(y, labels)
    assert torch.equal(z.view(torch.int16), reps[False][0].seen[0].view(torch.int16))
    pred, rank, conf = _check_rows(z, y, "ce", "model logits")  # the kernel's own rows, within the row bounds
    want = torch.zeros_like(rep.state, device="cpu")
    E.eval_accumulate_torch(y.cpu(), pred.cpu(), rank.cpu(), conf.cpu(), L, 15, want)
    assert torch.equal(rep.state.cpu(), want)
    v = rep.v
    assert int(v["padded"]) == 2 and int(v["rows"]) == B - 2 and int(v["nonfinite"]) == 0
    assert float(v["hit1"].sum()) == out["acc1"].item() and float(v["hit5"].sum()) == out["acc5"].item()
    off = reps[False][0].v
    for k in ("rows", "nonfinite", "padded", "count", "hit1", "hit5", "predicted", "confusion"):
        assert torch.equal(v[k], off[k]), k
    assert torch.equal(v["bins"][:, :2].sum(0), off["bins"][:, :2].sum(0))


# ------------------------------------------------------------------------------------ driver
def test_driver_on_the_gpu(tmp_path):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.train import finetune as FT
    from jumbo_mae_tpu_amd.train.cli import finetune_parser

    d = str(tmp_path)
    train = write_shards(d, shards=1, per_shard=16, classes=4, seed=0, prefix="train")
    valid = write_shards(d, shards=1, per_shard=11, classes=4, seed=1, prefix="valid")
    base = ["--train-loader-workers", "0", "--valid-loader-workers", "0", "--random-erasing", "0", "--image-size", "32",
            "--patch-size", "16", "--layers", "2", "--dim", "64", "--heads", "2", "--init-seed", "0", "--mixup-seed", "0",
            "--dropout-seed", "0", "--noise-seed", "0", "--shuffle-seed", "0", "--log-file-only", "--device", "cuda",
            "--train-batch-size", "8", "--valid-batch-size", "8", "--augment-repeats", "1", "--learning-rate", "5e-3",
            "--training-steps", "4", "--warmup-steps", "1", "--log-interval", "2", "--eval-interval", "2",
            "--droppath", "0", "--mixup", "0", "--cutmix", "0", "--labels", "4", "--name", "f",
            "--train-dataset-shards", train, "--valid-dataset-shards", valid]
    blobs, evals = {}, {}
    for name, extra in (("plain", []), ("report", ["--eval-report"])):
        out = os.path.join(d, name)
        FT.main(finetune_parser().parse_args(base + ["--output-dir", out] + extra))
        with open(os.path.join(out, "f-last.msgpack"), "rb") as f:
            blobs[name] = f.read()
        rows = [json.loads(line) for line in open(os.path.join(out, "f-metrics.jsonl"))]
        evals[name] = [r for r in rows if "val/loss" in r]
    assert blobs["plain"] == blobs["report"]
    old = ("val/loss", "val/acc1", "val/acc5")
    assert [[r[k] for k in old] for r in evals["plain"]] == [[r[k] for k in old] for r in evals["report"]]
    assert [r["step"] for r in evals["report"]] == [0, 2, 4]
    for r in evals["report"]:
        j = json.load(open(os.path.join(d, "report", f"f-report-{r['step']:07d}.json")))
        cm = np.load(os.path.join(d, "report", f"f-confusion-{r['step']:07d}.npy"))
        assert j["rows"] == 11 == int(cm.sum()) and j["nonfinite"] == 0 and cm.shape == (4, 4)
        assert int(np.trace(cm)) / 11 == r["val/acc1"]
        assert j["metrics"]["val/ece"] == r["val/ece"] and 0.0 <= r["val/ece"] <= r["val/mce"] <= 1.0
    assert "val/ece" not in evals["plain"][0]
    assert not any("report" in f or "confusion" in f for f in os.listdir(os.path.join(d, "plain")))
