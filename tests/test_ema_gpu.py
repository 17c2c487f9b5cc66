"""The weight-EMA kernels of csrc/optim.hip (``opt_ema``, ``ema_swap``) and ``optim/ema.py`` on the GPU.

Raw bindings run on the hand-built chunk tables of tests/optim_ref.py (``runs64``, ``partial``, ``prod``:
~70 k floats, chunks of 7 and 1 elements for the scalar tail, gaps, a tail, rows removed; every
segment's values carry a different power of ten), against the float64 recurrence of tests/ema_ref.py.

opt_ema   per element |err| <= 3 u (|omd (p - e)| + |e|) + 2^-126, u = 2^-24: the subtraction, the
          product and the sum round once each (a contracted FMA only removes one); two consecutive
          updates, so a non-trivial e carries over and the bounds add.  omd == 0 and p == e keep the
          bits of e.  Two frozen segments (meta[3] = 0; one single-chunk, one multi-chunk; in ``prod``,
          which has two segments, the second) and everything outside the rows (pre-filled with a
          sentinel) keep their bits, master keeps its bits everywhere, a rerun gives the same bits.
ema_swap  moves: on covered elements master and ema exchange their bits (NaNs with payloads, +-inf,
          -0.0, subnormals among them), the shadow is bit-equal to ``new_master.to(bfloat16)`` as torch
          casts it on the same device, uncovered elements of all three buffers keep their bits, a second
          swap restores everything, and a call without a shadow moves the same bits.
"""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import ema_ref as ER
import optim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SENTINEL = -77.0  # exact in bf16
OMDS = (float(np.float32(1 - 0.1)), 0.5, float(np.float32(1 - 0.9999)), 2.0 ** -20, 0.0)
TABLES = ("runs64", "partial", "prod")


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


@pytest.fixture(scope="module")
def tables():
    from jumbo_mae_tpu_amd.optim import flat
    full = R.runs64()
    return {"runs64": full, "partial": R.partial(full), "prod": R.prod(flat.CHUNK)}


def frozen_of(tab) -> tuple:
    return (3, 4) if tab.nseg == 7 else (1,)  # runs64: one chunk of 7 elements, and a run of 256 chunks


def same_bits(a, b, mask=None) -> bool:
    a, b = ER.bits(a), ER.bits(b)
    return bool(torch.equal(a, b) if mask is None else torch.equal(a[mask], b[mask]))


def setup(tab, seed):
    """(meta, live mask, p1, p2, e0): two masters and a start average, e0's uncovered elements the sentinel."""
    spec = R.spec_for(tab)
    frozen = frozen_of(tab)
    meta = R.make_meta("adamw", spec, frozen)
    p1, e0 = R.make_inputs(tab, spec, seed)
    p2, _ = R.make_inputs(tab, spec, seed + 1)
    e0 = torch.where(tab.covered, e0, torch.full_like(e0, SENTINEL))
    live = tab.covered & (meta[tab.seg_of.clamp(min=0), 3] != 0)
    return meta, live, p1, p2, e0


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("omd", OMDS)
def test_opt_ema_against_fp64(ext, tables, name, omd):
    tab = tables[name]
    meta, live, p1, p2, e0 = setup(tab, 11)
    rows, meta_d = tab.rows.to(DEV), meta.to(DEV)
    hyper = torch.tensor([omd, 123.0], dtype=torch.float32, device=DEV)  # only hyper[0] is read
    e = e0.to(DEV)
    ref, bound = ER._d(e0), torch.zeros(tab.n, dtype=torch.float64)
    for p in (p1, p2):
        p_d = p.to(DEV)
        ext.opt_ema(p_d, e, rows, meta_d, hyper)
        assert same_bits(p_d, p)  # master is only read
        ref, b = ER.step(ref, p, omd, live)
        bound = bound + b
        err = (ER._d(e) - ref).abs()
        bad = err > bound
        assert not bool(bad.any()), (int(bad.sum()), int(torch.nonzero(bad)[0]), float(err[bad].max()))
    got = e.cpu()
    # frozen segments, gaps, tail, removed rows: untouched
    assert same_bits(got, e0, ~live) and bool((got[~tab.covered] == SENTINEL).all())
    assert all(bool((tab.seg_of == k).any()) for k in frozen_of(tab))  # every table covers part of each
    if omd == 0.0:
        assert same_bits(got, e0)
    else:
        assert bool((got[live] != e0[live]).float().mean() > 0.5)  # and the live elements did move
    # a rerun of both updates gives the same bits
    e2 = e0.to(DEV)
    for p in (p1, p2):
        ext.opt_ema(p.to(DEV), e2, rows, meta_d, hyper)
    assert same_bits(e2, got)


@pytest.mark.parametrize("name", TABLES)
def test_opt_ema_equal_inputs_keep_the_bits(ext, tables, name):
    tab = tables[name]
    meta, live, p1, _, _ = setup(tab, 5)
    with_zeros = p1.clone()
    idx = torch.nonzero(live).flatten()
    with_zeros[idx[::7]] = -0.0  # -0.0 + 0.0 would be +0.0
    with_zeros[idx[3::7]] = 0.0
    e = with_zeros.to(DEV)
    hyper = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    ext.opt_ema(with_zeros.to(DEV), e, tab.rows.to(DEV), meta.to(DEV), hyper)
    assert same_bits(e, with_zeros)
    # omd == 0 with p != e, -0.0 included
    p2 = p1 + 1.0
    hyper.zero_()
    ext.opt_ema(p2.to(DEV), e, tab.rows.to(DEV), meta.to(DEV), hyper)
    assert same_bits(e, with_zeros)


SPECIALS = (0x7FC12345, 0xFFC54321, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F812345,
            0x3F808000, 0x3F818000)  # NaNs with payloads, +-inf, -0.0, subnormals, a signalling NaN, two bf16 ties


def _with_specials(tab, t, shift):
    """``t`` with the special words written, by their bits, at covered positions of every segment: the
    first elements of the segment (vector body, or the scalar loop of the 7- and 1-element chunks) and
    its last (the scalar tail where the last chunk's length is no multiple of 4)."""
    w = ER.bits(t).clone()
    sp = torch.tensor(SPECIALS, dtype=torch.int64)
    sp = torch.where(sp >= 2 ** 31, sp - 2 ** 32, sp).to(torch.int32)
    for k in range(tab.nseg):
        idx = torch.nonzero(tab.seg_of == k).flatten()
        n = min(len(SPECIALS), idx.numel())
        w[idx[:n]] = sp.roll(shift + k)[:n]
        w[idx[-1]] = sp[(shift + k) % len(SPECIALS)]
    return w.view(torch.float32)


@pytest.mark.parametrize("name", TABLES)
def test_ema_swap_moves_bits(ext, tables, name):
    tab = tables[name]
    spec = R.spec_for(tab)
    p0, e0 = R.make_inputs(tab, spec, 21)
    p0, e0 = _with_specials(tab, p0, 0), _with_specials(tab, e0, 3)
    cov = tab.covered
    assert bool(torch.isnan(p0[cov]).any()) and bool(torch.isinf(e0[cov]).any())
    s0 = torch.full((tab.n,), SENTINEL, dtype=torch.bfloat16)
    rows = tab.rows.to(DEV)
    p, e, s = p0.to(DEV), e0.to(DEV), s0.to(DEV)
    ext.ema_swap(p, e, s, rows)
    assert same_bits(p, e0, cov) and same_bits(e, p0, cov)
    assert same_bits(s, p.to(torch.bfloat16), cov)  # torch's cast of the new master, on this device
    for now, was in ((p, p0), (e, e0), (s, s0)):
        assert same_bits(now, was, ~cov)
    # without a shadow: the same master / ema bits
    p_n, e_n = p0.to(DEV), e0.to(DEV)
    ext.ema_swap(p_n, e_n, None, rows)
    assert same_bits(p_n, p) and same_bits(e_n, e)
    # a second swap restores everything; the shadow is the cast of the restored master
    ext.ema_swap(p, e, s, rows)
    assert same_bits(p, p0) and same_bits(e, e0)
    assert same_bits(s, p.to(torch.bfloat16), cov) and same_bits(s, s0, ~cov)


def test_bad_arguments_raise(ext, tables):
    tab = tables["runs64"]
    n = tab.n
    rows = tab.rows.to(DEV)
    meta = R.make_meta("adamw", R.spec_for(tab)).to(DEV)
    hyper = torch.tensor([0.5], device=DEV)
    p, e = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    ext.opt_ema(p, e, rows, meta, hyper)
    ext.ema_swap(p, e, sh, rows)
    cov = tab.covered.to(DEV)
    assert bool((p[cov] == 0.5).all()) and bool((e[cov] == 0).all()) and bool((sh[cov] == 0.5).all())
    old = [t.clone() for t in (p, e, sh)]
    bad = [
        lambda: ext.opt_ema(p, e.double(), rows, meta, hyper),            # wrong dtype
        lambda: ext.opt_ema(p.half(), e, rows, meta, hyper),
        lambda: ext.opt_ema(p, e, rows.long(), meta, hyper),
        lambda: ext.opt_ema(p, e.cpu(), rows, meta, hyper),               # a CPU tensor
        lambda: ext.opt_ema(p, e, rows.cpu(), meta, hyper),
        lambda: ext.opt_ema(p, e, rows, meta, hyper.cpu()),
        lambda: ext.opt_ema(p, e[:n - 4], rows, meta, hyper),             # ema shorter than the rows reach
        lambda: ext.opt_ema(p, e, rows, meta.reshape(-1), hyper),
        lambda: ext.ema_swap(p, e.double(), sh, rows),
        lambda: ext.ema_swap(p.cpu(), e, sh, rows),
        lambda: ext.ema_swap(p, e[:n - 4], sh, rows),
        lambda: ext.ema_swap(p, e, sh[:n - 4], rows),                     # a shadow of the wrong length
        lambda: ext.ema_swap(p, e, sh.float(), rows),
        lambda: ext.ema_swap(p, e, sh.cpu(), rows),
    ]
    for i, call in enumerate(bad):
        with pytest.raises((RuntimeError, TypeError)):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert all(same_bits(now, was) for now, was in zip((p, e, sh), old))  # the refused calls ran nothing


DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.debug_build and ext.debug_lines() == {}
    n = 256
    p, e = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    sh = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
    meta = torch.tensor([[0.0, 1.0, 0.0, 1.0]], device="cuda")
    hyper = torch.tensor([0.5], device="cuda")
    rows = torch.tensor([[0, 64, 0], [64, 64, 0]], dtype=torch.int32, device="cuda")
    ext.opt_ema(p, e, rows, meta, hyper)
    ext.ema_swap(p, e, sh, rows)
    torch.cuda.synchronize()
    assert ext.debug_lines() == {} and bool((p[:128] == 0.5).all()) and bool((e[:128] == 0).all())
    past = torch.tensor([[128, 64, 0], [224, 64, 0]], dtype=torch.int32, device="cuda")  # the second ends at 288
    ext.opt_ema(p, e, past, meta, hyper)
    torch.cuda.synchronize()
    lines = ext.debug_lines()
    assert set(lines) == {"optim"} and lines["optim"] > 0, lines
    assert bool((e[128:192] == 0.5).all()) and bool((e[192:] == 1).all())  # recorded, and skipped
    ext.ema_swap(p, e, sh, past)
    torch.cuda.synchronize()
    lines2 = ext.debug_lines()
    assert set(lines2) == {"optim"} and lines2["optim"] != lines["optim"], (lines, lines2)
    assert bool((p[128:192] == 0.5).all()) and bool((p[192:] == 0).all()) and bool((sh[192:] == 3).all())
    noseg = torch.tensor([[192, 64, 1]], dtype=torch.int32, device="cuda")  # a segment past meta
    ext.opt_ema(p, e, noseg, meta, hyper)
    torch.cuda.synchronize()
    assert set(ext.debug_lines()) == {"optim"} and ext.debug_lines() == {}
    print("EMA_DEBUG_OK")
""")


def test_debug_build_records_a_row_past_the_buffer():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "EMA_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------ integration
LR = {"adamw": 1e-3, "lamb": 1e-2, "lars": 1.0, "sgd": 0.1}


def _model(seed=0):
    from jumbo_mae_tpu_amd.config import ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    vc = ViTConfig(layers=2, dim=64, heads=2, labels=10, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.0)
    return FinetuneModel(vc).to(DEV, torch.bfloat16, seed=seed)


def _trainer(kind, with_ema):
    from jumbo_mae_tpu_amd.optim.ema import WeightEma
    from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer
    from jumbo_mae_tpu_amd.train.engine import Trainer
    from jumbo_mae_tpu_amd.utils.rng import RngStreams
    m = _model()
    opt = FlatOptimizer(m.store, kind, lambda c: LR[kind], weight_decay=0.05, num_layers=2)
    ema = None
    if with_ema:
        ema = WeightEma(m.store, 0.99)
        opt.attach_ema(ema)
    return m, opt, ema, Trainer(m, opt, None, RngStreams({"mixup": 1, "dropout": 1, "noise": 1}, 0, DEV))


def _batches(n=4):
    g = torch.Generator().manual_seed(0)
    return [(torch.randint(0, 256, (8, 3, 32, 32), dtype=torch.uint8, generator=g).to(DEV),
             torch.randint(0, 10, (8,), generator=g).to(DEV)) for _ in range(n)]


def _live(store):
    live = torch.zeros(store.total, dtype=torch.bool)
    for s in store.segments:
        if s.trainable:
            live[s.offset:s.offset + s.numel] = True
    return live


@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars", "sgd"])
def test_three_steps_follow_the_recurrence(kind):
    data = _batches(3)
    out = {}
    for with_ema in (True, False):
        m, opt, ema, tr = _trainer(kind, with_ema)
        e0 = m.store.master.clone()
        snaps, losses = [], []
        for b in data:
            losses.append(tr.train_step([b])["loss"].clone())
            snaps.append(m.store.master.clone())
        torch.cuda.synchronize()
        out[with_ema] = (m, opt, ema, e0, snaps, [float(x) for x in losses])
    m, opt, ema, e0, snaps, losses = out[True]
    live = _live(m.store)
    assert ema.updates == 3 and not torch.equal(snaps[2].cpu()[live], e0.cpu()[live])
    ref, bound = ER.run(e0, snaps, 0.99, live)
    err = (ER._d(ema.ema) - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()))
    assert same_bits(ema.ema, e0, ~live) and not same_bits(ema.ema, e0, live)
    m0, opt0, _, _, snaps0, losses0 = out[False]
    assert losses == losses0 and same_bits(snaps[2], snaps0[2]) and same_bits(m.store.shadow, m0.store.shadow)
    for k in ("mu", "nu", "trace"):
        if getattr(opt, k) is not None:
            assert same_bits(getattr(opt, k), getattr(opt0, k)), k


def test_hip_graph_steps_give_the_eager_bits():
    from jumbo_mae_tpu_amd.runtime.graph import StepRunner
    data = _batches(3)
    m1, _, ema1, tr1 = _trainer("adamw", True)
    m2, _, ema2, tr2 = _trainer("adamw", True)
    run = StepRunner(tr2, hip_graph=True)
    for b in data:
        tr1.train_step([b])
        run([b])
    torch.cuda.synchronize()
    assert run.graphed is not None and run.graphed.replays == 3
    assert ema1.updates == ema2.updates == 3  # the warm-up steps of the capture are undone
    assert same_bits(m2.store.master, m1.store.master)
    assert same_bits(ema2.ema, ema1.ema) and not same_bits(ema1.ema, m1.store.master)


def test_swapped_evaluation_equals_a_model_with_the_average():
    data = _batches(4)
    m, opt, ema, tr = _trainer("adamw", True)
    for b in data[:3]:
        tr.train_step([b])
    s = m.store
    old = (s.master.clone(), s.shadow.clone(), ema.ema.clone(), s.version)
    live_eval = m.evaluate(*data[3])
    with ema.swapped():
        v_in = s.version
        got = m.evaluate(*data[3])
        tree = m.flax_params()
    assert v_in > old[3] and s.version > v_in
    for now, was in zip((s.master, s.shadow, ema.ema), old):
        assert same_bits(now, was)
    # a second model that loads the average as a params tree
    m2 = _model(seed=5)
    m2.store.master.copy_(old[2])
    want_tree = m2.store.to_flax_tree()
    m2 = _model(seed=5)
    m2.store.load_flax_tree(want_tree, strict=True)
    want = m2.evaluate(*data[3])
    assert set(got) == set(want)
    for k in want:
        assert same_bits(got[k].float(), want[k].float()), k
    assert float(got["loss"]) != float(live_eval["loss"])
    from jumbo_mae_tpu_amd.ckpt.msgpack_flax import flatten_tree
    a, b = flatten_tree(tree), flatten_tree(want_tree)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    again = m.evaluate(*data[3])  # and the live weights are back for the next evaluation
    assert all(same_bits(again[k].float(), live_eval[k].float()) for k in again)
