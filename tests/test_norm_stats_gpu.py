"""The norm monitor's kernels (csrc/optim.hip ``seg_stats_kernel`` / ``seg_stats_finish_kernel``, binding
``opt_seg_stats``) and ``optim/monitor.py`` on the GPU.

The raw binding runs on the hand-built chunk tables of tests/optim_ref.py (``runs64``, ``partial``,
``prod``: ~70 k floats, rows of 7 and 1 elements for the scalar tail, gaps, a tail, rows removed as under
ZeRO-1) against the exact reference of tests/norm_stats_ref.py (``math.fsum`` of the float64 terms, integer
counts, the exact maximum).  Bounds, derived there and not measured: columns 3..6 equal; G2 and P2 within
n 2^-53 S*, D2 within (n + 4) 2^-53 S*, n the segment's term count; on exactly summable inputs bit for bit.
"""

import os
import subprocess
import sys
import textwrap

import pytest
import torch

import norm_stats_ref as NR
import optim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TABLES = ("runs64", "partial", "prod")


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


@pytest.fixture(scope="module")
def tables():
    from jumbo_mae_tpu_amd.optim import flat
    return NR.tables(flat.CHUNK)


def frozen_of(tab) -> tuple:
    return (3, 4) if tab.nseg == 7 else (1,)  # runs64: one chunk of 7 elements, and a run of 256 chunks


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b) -> bool:
    return bool(torch.equal(bits(a), bits(b)))


def run(ext, tab, meta, p, g, old, out=None):
    """The binding on device copies of the CPU inputs; asserts that it only reads them."""
    dp, dg = p.to(DEV), g.to(DEV)
    do = old.to(DEV) if old is not None else None
    got = ext.opt_seg_stats(dp, dg, do, tab.rows.to(DEV), meta.to(DEV), out)
    torch.cuda.synchronize()
    assert same_bits(dp, p) and same_bits(dg, g) and (old is None or same_bits(do, old))
    assert got.dtype == torch.float64 and tuple(got.shape) == (tab.nseg, 7) and got.is_cuda
    return got


def random_inputs(tab, seed):
    spec = R.spec_for(tab)  # a different power of ten per segment
    p, g = R.make_inputs(tab, spec, seed)
    noise, _ = R.make_inputs(tab, spec, seed + 1)
    return spec, p, g, p + 1e-2 * noise  # p_old = p + fp32 noise, rounded to fp32


@pytest.mark.parametrize("name", TABLES)
def test_random_inputs_against_fsum(ext, tables, name):
    tab = tables[name]
    spec, p, g, old = random_inputs(tab, 31)
    meta = R.make_meta("adamw", spec)
    ref, terms = NR.ref_stats(tab, meta, p, g, old)
    out = torch.full((tab.nseg, 7), float("nan"), dtype=torch.float64, device=DEV)
    got = run(ext, tab, meta, p, g, old, out)
    assert got.data_ptr() == out.data_ptr()
    print(name, got.cpu().tolist())
    NR.assert_stats(got, ref, terms, name)
    assert bool((ref[:, 2] > 0).any()) and bool((ref[:, 0] > 0).any())
    # a rerun gives the same bits; so does a call that allocates its own out
    assert same_bits(run(ext, tab, meta, p, g, old), got)
    # optional snapshot: column 2 is 0, the other columns keep their bits
    no_old = run(ext, tab, meta, p, g, None)
    assert not bool(no_old[:, 2].any())
    keep = [0, 1, 3, 4, 5, 6]
    assert same_bits(no_old[:, keep], got[:, keep])
    if name == "partial":  # the sums are over the covered rows only
        full_ref, _ = NR.ref_stats(tables["runs64"], meta, p, g, old)
        assert bool((ref[:, 6] < full_ref[:, 6]).any()) and bool((ref[:, 1] < full_ref[:, 1]).any())


@pytest.mark.parametrize("name", TABLES)
def test_exactly_summable_inputs_bit_for_bit(ext, tables, name):
    tab = tables[name]
    spec = R.spec_for(tab)
    meta = R.make_meta("adamw", spec)
    g, c = R.exact_norm_grad(tab, spec, 7)
    gen = torch.Generator().manual_seed(9)
    p = torch.randint(-6, 7, (tab.n,), generator=gen).to(torch.float32) * 0.5
    old = p - torch.randint(-3, 4, (tab.n,), generator=gen).to(torch.float32) * 0.5
    ref, terms = NR.ref_stats(tab, meta, p, g, old)
    got = run(ext, tab, meta, p, g, old)
    NR.assert_stats(got, ref, terms, name, exact_sums=True)
    quarter = got[:, :3].cpu() * 4
    assert torch.equal(quarter, quarter.round())  # integers / quarter units
    assert float(got[:, 0].cpu().sum()) == c * c


def test_range(ext, tables):
    tab = tables["runs64"]
    spec = R.spec_for(tab)
    meta = R.make_meta("adamw", spec)
    p, g = R.make_inputs(tab, spec, 41)
    sign = torch.where(torch.arange(tab.n) % 3 == 0, -1.0, 1.0)
    g[tab.seg_of == 1] = (2.0 ** 100 * sign)[tab.seg_of == 1]   # an fp32 square would overflow
    g[tab.seg_of == 2] = 2.0 ** -149                             # the smallest subnormal: its fp32 square is 0
    g[tab.seg_of == 0] = -0.0
    p[tab.seg_of == 0] = -0.0
    assert float(g[tab.seg_of == 2][0]) == 2.0 ** -149
    got = run(ext, tab, meta, p, g, None).cpu()
    n = [int((tab.seg_of == k).sum()) for k in range(tab.nseg)]
    assert float(got[1, 0]) == n[1] * 2.0 ** 200 and float(got[1, 3]) == 2.0 ** 100
    assert float(got[2, 0]) == n[2] * 2.0 ** -298 and float(got[2, 3]) == 2.0 ** -149
    assert got[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, float(n[0])]  # -0.0 is finite and adds 0
    ref, terms = NR.ref_stats(tab, meta, p, g, None)
    NR.assert_stats(got, ref, terms, "range")


SPECIALS = (0x7FC12345, 0xFFC54321, 0x7F800000, 0xFF800000, 0x7F812345)  # NaNs with payloads, +-inf, a signalling NaN


def plant(tab, t, shift, every):
    """``t`` with special words at covered positions of every segment: its first elements (the vector body,
    or the scalar loop of the 7- and 1-element chunks), every ``every``-th element, and its last (the
    scalar tail where the last chunk's length is no multiple of 4).  Returns the number planted per segment."""
    w = t.view(torch.int32).clone()
    sp = torch.tensor(SPECIALS, dtype=torch.int64)
    sp = torch.where(sp >= 2 ** 31, sp - 2 ** 32, sp).to(torch.int32)
    count = []
    for k in range(tab.nseg):
        idx = torch.nonzero(tab.seg_of == k).flatten()
        pos = torch.unique(torch.cat([idx[:2], idx[shift::every], idx[-1:]]))
        w[pos] = sp[(torch.arange(pos.numel()) + shift + k) % len(SPECIALS)]
        count.append(int(pos.numel()))
    return w.view(torch.float32), count


@pytest.mark.parametrize("name", TABLES)
def test_nonfinite_values_are_counted_and_left_out(ext, tables, name):
    tab = tables[name]
    spec, p, g, old = random_inputs(tab, 51)
    meta = R.make_meta("adamw", spec)
    g, ng = plant(tab, g, 0, 61)
    p, np_ = plant(tab, p, 1, 89)
    old, _ = plant(tab, old, 2, 97)
    ref, terms = NR.ref_stats(tab, meta, p, g, old)
    assert ref[:, 4].tolist() == [float(x) for x in ng] and ref[:, 5].tolist() == [float(x) for x in np_]
    if tab.nseg == 7:  # the 7-element chunk's scalar tail and the 1-element chunk hold one
        assert not torch.isfinite(g[tab.seg_of == 3][-1]) and not torch.isfinite(g[tab.seg_of == 5][0])
        assert ref[5].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    else:  # prod: the row of 5 elements ends segment 0
        assert not torch.isfinite(g[tab.seg_of == 0][-1]) and int((tab.seg_of == 0).sum()) % 4 == 1
    got = run(ext, tab, meta, p, g, old)
    NR.assert_stats(got, ref, terms, name)
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("name", TABLES)
def test_frozen_segments_report_the_weights_only(ext, tables, name):
    tab = tables[name]
    spec, p, g, old = random_inputs(tab, 61)
    frozen = frozen_of(tab)
    meta = R.make_meta("adamw", spec, frozen)
    for k in frozen:  # the model never writes a frozen gradient: its content means nothing
        g[tab.seg_of == k] = float("nan")
        old[tab.seg_of == k] = float("nan")
        p[torch.nonzero(tab.seg_of == k).flatten()[-1]] = float("inf")
    ref, terms = NR.ref_stats(tab, meta, p, g, old)
    got = run(ext, tab, meta, p, g, old)
    NR.assert_stats(got, ref, terms, name)
    for k in frozen:
        row = got[k].cpu().tolist()
        assert [row[0], row[2], row[3], row[4]] == [0.0, 0.0, 0.0, 0.0]
        assert row[1] > 0 and row[5] == 1.0 and row[6] == float((tab.seg_of == k).sum())


def test_segment_without_rows_gets_zeros(ext, tables):
    tab = tables["runs64"]
    rows = tab.rows[(tab.rows[:, 2] != 2) & (tab.rows[:, 2] != 5) & (tab.rows[:, 2] != 6)]  # the last segment too
    cut = R.table_from_rows("cut", rows, tab.n, tab.nseg)
    spec, p, g, old = random_inputs(tab, 71)
    meta = R.make_meta("adamw", spec)
    ref, terms = NR.ref_stats(cut, meta, p, g, old)
    out = torch.full((tab.nseg, 7), float("nan"), dtype=torch.float64, device=DEV)
    got = run(ext, cut, meta, p, g, old, out)
    NR.assert_stats(got, ref, terms, "cut")
    for k in (2, 5, 6):
        assert got[k].cpu().tolist() == [0.0] * 7
    # no rows at all: every row of out defined
    out.fill_(float("nan"))
    none = ext.opt_seg_stats(p.to(DEV), g.to(DEV), None, tab.rows[:0].to(DEV), meta.to(DEV), out)
    assert none.cpu().tolist() == [[0.0] * 7] * tab.nseg


def test_bad_arguments_raise(ext, tables):
    tab = tables["runs64"]
    n = tab.n
    rows = tab.rows.to(DEV)
    meta = R.make_meta("adamw", R.spec_for(tab)).to(DEV)
    p, g, o = (torch.ones(n, device=DEV) for _ in range(3))
    out = torch.zeros(tab.nseg, 7, dtype=torch.float64, device=DEV)
    ext.opt_seg_stats(p, g, o, rows, meta, out)
    assert out[:, 6].cpu().tolist() == [float((tab.seg_of == k).sum()) for k in range(tab.nseg)]
    old = out.clone()
    bad = [
        lambda: ext.opt_seg_stats(p, g.double(), o, rows, meta, out),       # wrong dtype
        lambda: ext.opt_seg_stats(p.half(), g, o, rows, meta, out),
        lambda: ext.opt_seg_stats(p, g, o.double(), rows, meta, out),
        lambda: ext.opt_seg_stats(p, g, o, rows.long(), meta, out),
        lambda: ext.opt_seg_stats(p, g, o, rows, meta, out.float()),
        lambda: ext.opt_seg_stats(p, g.cpu(), o, rows, meta, out),          # a CPU tensor
        lambda: ext.opt_seg_stats(p, g, o.cpu(), rows, meta, out),
        lambda: ext.opt_seg_stats(p, g, o, rows.cpu(), meta, out),
        lambda: ext.opt_seg_stats(p, g, o, rows, meta.cpu(), out),
        lambda: ext.opt_seg_stats(p, g, o, rows, meta, out.cpu()),
        lambda: ext.opt_seg_stats(p, g[:n - 4], o, rows, meta, out),        # shorter than the rows reach
        lambda: ext.opt_seg_stats(p, g, o[:n - 4], rows, meta, out),
        lambda: ext.opt_seg_stats(p, g[::2], o, rows, meta, out),           # not contiguous
        lambda: ext.opt_seg_stats(p, g, o, rows, meta.reshape(-1), out),    # meta not [segments, 4]
        lambda: ext.opt_seg_stats(p, g, o, rows, meta[:, :3].contiguous(), out),
        lambda: ext.opt_seg_stats(p, g, o, rows[:, :2].contiguous(), meta, out),
        lambda: ext.opt_seg_stats(p, g, o, rows, meta, out[:-1]),           # out not [segments, 7]
        lambda: ext.opt_seg_stats(p, g, o, rows, meta, out[:, :6].contiguous()),
    ]
    for i, call in enumerate(bad):
        with pytest.raises((RuntimeError, TypeError)):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert same_bits(out, old)  # the refused calls ran nothing


DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.debug_build and ext.debug_lines() == {}
    n = 256
    p, g = torch.full((n,), 2.0, device="cuda"), torch.full((n,), 3.0, device="cuda")
    meta = torch.tensor([[0.0, 1.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.0]], device="cuda")
    rows = torch.tensor([[0, 64, 0], [64, 64, 1]], dtype=torch.int32, device="cuda")
    out = ext.opt_seg_stats(p, g, None, rows, meta)
    torch.cuda.synchronize()
    assert ext.debug_lines() == {} and out.cpu().tolist() == [[576.0, 256.0, 0.0, 3.0, 0.0, 0.0, 64.0]] * 2
    past = torch.tensor([[128, 64, 0], [224, 64, 1]], dtype=torch.int32, device="cuda")  # the second ends at 288
    out = ext.opt_seg_stats(p, g, None, past, meta)
    torch.cuda.synchronize()
    lines = ext.debug_lines()
    assert set(lines) == {"optim"} and lines["optim"] > 0, lines
    assert out.cpu().tolist() == [[576.0, 256.0, 0.0, 3.0, 0.0, 0.0, 64.0], [0.0] * 7], out  # recorded, and skipped
    noseg = torch.tensor([[0, 64, 0], [192, 64, 2]], dtype=torch.int32, device="cuda")  # a segment past meta
    out = ext.opt_seg_stats(p, g, p, noseg, meta)
    torch.cuda.synchronize()
    assert set(ext.debug_lines()) == {"optim"} and ext.debug_lines() == {}
    assert out.cpu().tolist() == [[576.0, 256.0, 0.0, 3.0, 0.0, 0.0, 64.0], [0.0] * 7], out
    print("NORM_DEBUG_OK")
""")


def test_debug_build_records_a_row_past_the_buffer():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "NORM_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------ integration
LR = {"adamw": 1e-3, "lamb": 1e-2, "lars": 1.0, "sgd": 0.1}


def _model(seed=0):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=10, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.0)
    return FinetuneModel(vc).to(DEV, torch.bfloat16, seed=seed)


def _trainer(kind, with_monitor, level="layer", clip=1.0):
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.optim.monitor import NormMonitor
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams
    m = _model()
    opt = FlatOptimizer(m.store, kind, lambda c: LR[kind], weight_decay=0.05, num_layers=2, clip_grad=clip)
    mon = NormMonitor(opt, level) if with_monitor else None
    return m, opt, mon, Trainer(m, opt, None, RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, DEV))


def _batches(n=3):
    g = torch.Generator().manual_seed(0)
    return [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=g).to(DEV),
             torch.randint(0, 10, (8,), generator=g).to(DEV)) for _ in range(n)]


def _assert_close(got, want, tag):
    """Against the float64 torch composition on the same buffers: the bounds of the module docstring, n
    the segment's elements."""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(got[:, 3:], want[:, 3:]), tag
    n = want[:, 6]
    for c in range(3):
        bound = (n + (4 if c == 2 else 0)) * NR.U53 * want[:, c]
        err = (got[:, c] - want[:, c]).abs()
        assert bool((err <= bound).all()), (tag, NR.COLS[c], float((err - bound).max()))


@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars", "sgd"])
def test_three_trainer_steps(kind, monkeypatch):
    from jumbo_mae_tpu_amd.ops import prims as P
    from jumbo_mae_tpu_amd.optim import monitor as M
    data = _batches(3)
    out = {}
    for with_monitor in (True, False):
        m, opt, mon, tr = _trainer(kind, with_monitor)
        for b in data[:2]:
            tr.train_step([b])
        before = m.store.master.clone()
        if mon is not None:
            mon.begin()
        tr.train_step([data[2]])
        torch.cuda.synchronize()
        out[with_monitor] = (m, opt, mon, before)
    m, opt, mon, before = out[True]
    s = m.store
    stats = mon.collect()
    want = M.seg_stats_torch(s.master.cpu(), s.grad.cpu(), before.cpu(), opt.chunks.cpu(), opt.meta.cpu(), opt.nseg)
    _assert_close(stats, want, kind)
    assert float(want[:, 2].sum()) > 0 and float(want[:, 0].sum()) > 0
    d = mon.summary(stats)
    assert d["train/update_norm"] > 0 and d["train/clip_scale"] == min(1.0, 1.0 / d["train/grad_norm"])
    # the switch: the torch composition on the GPU gives the same table within the same bounds
    monkeypatch.setattr(P, "_NORMS_OURS", False)
    mon._armed = True
    _assert_close(mon.collect(), want, kind + " torch")
    monkeypatch.setattr(P, "_NORMS_OURS", True)
    # weights, shadow and optimizer state: bit-identical to the run without the monitor
    m0, opt0, _, _ = out[False]
    assert same_bits(s.master, m0.store.master) and same_bits(s.shadow.float(), m0.store.shadow.float())
    for k in ("mu", "nu", "trace"):
        if getattr(opt, k) is not None:
            assert same_bits(getattr(opt, k), getattr(opt0, k)), k


def test_hip_graph_steps_give_the_eager_stats():
    from jumbo_mae_tpu_amd.runtime.graph import StepRunner
    data = _batches(3)
    m1, _, mon1, tr1 = _trainer("adamw", True, clip=0.0)
    m2, _, mon2, tr2 = _trainer("adamw", True, clip=0.0)
    run2 = StepRunner(tr2, hip_graph=True)
    for i, b in enumerate(data):
        if i == 2:
            mon1.begin()
            mon2.begin()
        tr1.train_step([b])
        run2([b])
    a, b = mon1.collect(), mon2.collect()
    torch.cuda.synchronize()
    assert run2.graphed is not None and run2.graphed.replays == 3
    assert same_bits(m2.store.master, m1.store.master)
    assert same_bits(a, b) and float(a[:, 2].sum()) > 0
