"""Optimizer / schedule semantics vs per-leaf re-statements of the optax transformations."""

import math

import numpy as np
import pytest
import torch

from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
from jumbo_mae_tpu_amd.models.mae import PretrainModel
from jumbo_mae_tpu_amd.optim.flat import FlatOptimizer, layer_index
from jumbo_mae_tpu_amd.optim.schedule import warmup_cosine_decay_schedule

import optim_ref as R


def test_schedule_boundaries():
    s = warmup_cosine_decay_schedule(1e-6, 1e-3, 10, 110, 1e-5)
    assert s(0) == pytest.approx(1e-6)
    assert s(5) == pytest.approx(1e-6 + 0.5 * (1e-3 - 1e-6))
    assert s(10) == pytest.approx(1e-3)
    alpha = 1e-5 / 1e-3
    # cosine over decay_steps - warmup = 100 steps (Q17)
    assert s(60) == pytest.approx(1e-3 * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * 0.5)) + alpha))
    assert s(110) == pytest.approx(1e-5)
    assert s(10_000) == pytest.approx(1e-5)
    z = warmup_cosine_decay_schedule(1e-6, 3.0, 0, 100, 1e-6)
    assert z(0) == pytest.approx(3.0)


def test_layer_index_labels():
    assert layer_index(("model", "layer_3", "attn", "wq", "kernel"), 12) == 4
    assert layer_index(("model", "embed", "wte", "kernel"), 12) == 0
    assert layer_index(("model", "cls_tokens"), 12) == 12
    assert layer_index(("model", "jumbo_mlp", "w1", "kernel"), 12) == 12
    assert layer_index(("decoder_model", "dec_layer_0", "ff"), 12) == 12


def _model():
    vc = ViTConfig(layers=2, dim=16, heads=2, labels=0, image_size=16, patch_size=8, posemb="learnable")
    dc = DecoderConfig(dec_layers=1, dec_dim=8, dec_heads=2, image_size=16, patch_size=8)
    return PretrainModel(vc, dc).to("cpu", seed=0)


def _leaves(store, flat):
    return {s.key: flat[s.offset:s.offset + s.numel].clone().double().view(s.shape) for s in store.segments}


def _ref_step(kind, p, g, st, count, lr, s, b1=0.9, b2=0.95, eps=1e-8, wd=0.05, clip=0.0, llrd=None,
              mom=0.9, tc=1e-3):
    """One optax update on dicts of leaves (float64)."""
    if clip > 0:
        gn = math.sqrt(sum(float((v ** 2).sum()) for v in g.values()))
        if gn >= clip:
            g = {k: v / gn * clip for k, v in g.items()}
    t = count + 1
    new = {}
    for k in p:
        kernel = k.endswith("/kernel")
        scale = llrd[k] if llrd else 1.0
        if kind in ("adamw", "lamb"):
            st["mu"][k] = b1 * st["mu"][k] + (1 - b1) * g[k]
            st["nu"][k] = b2 * st["nu"][k] + (1 - b2) * g[k] ** 2
            u = (st["mu"][k] / (1 - b1 ** t)) / (torch.sqrt(st["nu"][k] / (1 - b2 ** t)) + eps)
            if kernel:
                u = u + wd * p[k]
            if kind == "lamb" and kernel:
                pn, un = p[k].norm(), u.norm()
                if pn > 0 and un > 0:
                    u = u * (pn / un)
            new[k] = p[k] - lr * u * scale
        elif kind == "lars":
            u = g[k]
            pn, un = p[k].norm(), u.norm()
            tr = tc * pn / un if (pn > 0 and un > 0) else 1.0
            u = -lr * (u * tr)
            st["tr"][k] = u + mom * st["tr"][k]
            new[k] = p[k] + st["tr"][k] * scale
        else:
            st["tr"][k] = g[k] + mom * st["tr"][k]
            new[k] = p[k] - lr * st["tr"][k] * scale
    return new


@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars", "sgd"])
@pytest.mark.parametrize("clip,lr_decay", [(0.0, 1.0), (0.3, 0.75)])
def test_flat_optimizer_matches_optax_semantics(kind, clip, lr_decay):
    m = _model()
    sched = warmup_cosine_decay_schedule(1e-6, 1e-2, 2, 8, 1e-5)
    opt = FlatOptimizer(m.store, kind, sched, b1=0.9, b2=0.95, eps=1e-8, weight_decay=0.05, lr_decay=lr_decay,
                        num_layers=2, clip_grad=clip)
    p = _leaves(m.store, m.store.master)
    st = {"mu": {k: torch.zeros_like(v) for k, v in p.items()}, "nu": {k: torch.zeros_like(v) for k, v in p.items()},
          "tr": {k: torch.zeros_like(v) for k, v in p.items()}}
    llrd = {s.key: (lr_decay ** (2 - layer_index(s.path, 2)) if lr_decay < 1 else 1.0) for s in m.store.segments}
    gen = torch.Generator().manual_seed(0)
    for c in range(4):
        m.store.grad.copy_(torch.randn(m.store.total, generator=gen) * 0.1)
        g = _leaves(m.store, m.store.grad)
        lr = opt.step()
        assert lr == pytest.approx(sched(c))
        wd = 0.05 if kind in ("adamw", "lamb") else 0.0
        p = _ref_step(kind, p, g, st, c, lr, None, wd=wd, clip=clip, llrd=llrd)
        ours = _leaves(m.store, m.store.master)
        for k in p:
            np.testing.assert_allclose(ours[k].numpy(), p[k].numpy(), rtol=2e-5, atol=3e-6, err_msg=k)


def test_optimizer_state_roundtrip():
    m = _model()
    opt = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 2, 8, 1e-5))
    m.store.grad.normal_()
    opt.step()
    sd = opt.state_dict()
    opt2 = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 2, 8, 1e-5))
    opt2.load_state_dict(sd)
    assert opt2.count == 1
    assert torch.equal(opt2.mu, opt.mu) and torch.equal(opt2.nu, opt.nu)


def test_optimizer_state_from_older_padding():
    """A sidecar written when the flat total was padded to 64 elements (round <= 3) resumes into
    today's TOTAL_ALIGN-padded buffers: the common prefix is copied, the padding tail zeroed."""
    m = _model()
    opt = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 2, 8, 1e-5))
    m.store.grad.normal_()
    m.store.grad[m.store.used_numel():] = 0
    opt.step()
    sd = opt.state_dict()
    old_total = -(-m.store.used_numel() // 64) * 64
    assert old_total < m.store.total
    old = {k: (v[:old_total].clone() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}
    opt2 = FlatOptimizer(m.store, "adamw", warmup_cosine_decay_schedule(1e-6, 1e-3, 2, 8, 1e-5))
    opt2.mu.fill_(7.0)
    opt2.load_state_dict(old)
    assert torch.equal(opt2.mu, opt.mu) and torch.equal(opt2.nu, opt.nu)
    # a larger saved buffer (a store padded for more ranks) loads too while its tail is zero
    big = {k: (torch.cat([v, torch.zeros(128)]) if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}
    opt2.load_state_dict(big)
    assert torch.equal(opt2.nu, opt.nu)
    bad = dict(big, mu=torch.cat([sd["mu"], torch.ones(128)]))
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)
    with pytest.raises(ValueError):
        opt2.load_state_dict(dict(sd, mu=sd["mu"][:m.store.used_numel() - 1]))


# ---------------------------------------------------------------------- fp64 reference, chunk tables
def test_chunk_tables_have_the_runs_the_kernel_tests_rely_on():
    """tests/optim_ref.py: ``runs64`` has runs of 1, 257, 600, 1, 256, 1 and 3 chunks (the 256-strided
    walk of chunk_sums_kernel wraps, starts at rows > 0, ends at the last row), chunks of 7 and 1
    elements, gaps and a tail nobody covers; ``partial`` drops every third row and keeps every segment;
    ``prod`` is three rows of ``flat.CHUNK`` and one of 5, then one of 64."""
    from jumbo_mae_tpu_amd.optim import flat
    full = R.runs64()
    assert full.runs() == [(0, 1), (1, 257), (2, 600), (3, 1), (4, 256), (5, 1), (6, 3)]
    lens = full.rows[:, 1].tolist()
    assert lens[858] == 7 and lens[1115] == 1 and all(n == 64 for i, n in enumerate(lens) if i not in (858, 1115))
    assert int(full.rows[-1, 0] + full.rows[-1, 1]) == full.n - 12
    assert int((~full.covered).sum()) > 12 and bool((full.rows[:, 0] % 4 == 0).all())
    part = R.partial(full)
    assert part.rows.shape[0] == full.rows.shape[0] - len(range(1, full.rows.shape[0], 3))
    assert [s for s, _ in part.runs()] == list(range(7)) and torch.equal(part.rows[-1], full.rows[-1])
    assert bool((part.covered <= full.covered).all()) and int(part.covered.sum()) < int(full.covered.sum())
    pr = R.prod(flat.CHUNK)
    assert pr.rows[:, 1].tolist() == [flat.CHUNK] * 3 + [5, 64] and pr.runs() == [(0, 4), (1, 1)]


def test_exact_norm_gradient_is_a_perfect_square_in_fp32():
    tab = R.runs64()
    g, c = R.exact_norm_grad(tab, R.spec_for(tab), 0)
    v = g[tab.covered]
    for order in (v, v.flip(0), v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(0))]):
        s = torch.zeros((), dtype=torch.float32)
        for blk in order.split(4096):  # fp32 partial sums in several orders: all exact
            s = s + (blk * blk).sum()
        assert float(s) == c * c
    assert float(torch.tensor(c, dtype=torch.float32)) == c and float(torch.tensor(c * c).sqrt()) == c


_RUNS64_PATHS = [("model", "embed", "bias"), ("model", "layer_0", "ff", "kernel"), ("model", "layer_1", "ff", "kernel"),
                 ("model", "layer_2", "norm", "scale"), ("model", "layer_3", "ff", "kernel"),
                 ("model", "layer_4", "ff", "kernel"), ("head", "bias")]


def _runs64_store(frozen):
    """A hand-made ParamStore laid out like ``runs64`` (same offsets, gaps included)."""
    from jumbo_mae_tpu_amd.models.params import ParamStore, zeros_
    tab = R.runs64()
    store = ParamStore()
    for k, (path, (chunks, ln)) in enumerate(zip(_RUNS64_PATHS, R.RUNS64_CHUNKS)):
        store.total = int(tab.rows[tab.rows[:, 2] == k][0, 0])
        store.add(path, (chunks * ln,), zeros_, trainable=k not in frozen)
    store.total = tab.n
    store.finalize("cpu")
    return store, tab


@pytest.mark.parametrize("kind", ["adamw", "lamb", "lars", "sgd"])
def test_fp64_reference_matches_step_torch(kind, monkeypatch):
    """The float64 reference of tests/optim_ref.py (what the HIP kernels are held to) against
    ``FlatOptimizer._step_torch`` on the ``runs64`` layout: segments scaled by different powers of ten,
    a segment with p == 0, one with g == 0, a frozen 600-chunk segment, a clip below the gradient norm,
    layer-wise LR scales, two steps at the kernel tests' learning rates; tolerance of
    ``test_flat_optimizer_matches_optax_semantics``."""
    from jumbo_mae_tpu_amd.optim import flat
    monkeypatch.setattr(flat, "CHUNK", 64)
    store, tab64 = _runs64_store(frozen=(2,))
    lr = R.LR[kind]
    opt = FlatOptimizer(store, kind, lambda count: lr, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.1, lr_decay=0.75,
                        num_layers=6, clip_grad=50.0)
    assert torch.equal(opt.chunks, tab64.rows)
    tab = R.table_from_rows("store", opt.chunks, store.total, opt.nseg)
    spec = R.spec_for(tab)
    assert opt.meta[:, 3].tolist() == [1, 1, 0, 1, 1, 1, 1] and opt.meta[:, 1].unique().numel() == 7
    p0, _ = R.make_inputs(tab, spec, 10)
    p0[~tab.covered] = 0
    store.master.copy_(p0)
    st = {k: torch.zeros(store.total) for k in ("mu", "nu", "trace")}
    wd = 0.1 if kind in ("adamw", "lamb") else 0.0
    g = None
    for step in range(2):
        t = step + 1
        _, g = R.make_inputs(tab, spec, 20 + step, g)
        p_old = store.master.clone()
        store.grad.copy_(g)
        opt.step()
        hyper = torch.tensor([lr, 1 - 0.9 ** t, 1 - 0.999 ** t, 50.0, 0.9, 0.999, 1e-8, wd], dtype=torch.float32)
        ref = R.ref_step(kind, tab, opt.meta, hyper, p_old, g, st["mu"], st["nu"], st["trace"], clip_on=True)
        assert ref["f"] < 0.6  # the clip is active
        np.testing.assert_allclose(store.master.numpy(), ref["p"].numpy(), rtol=2e-5, atol=3e-6)
        frozen = tab.seg_of == 2
        assert torch.equal(store.master[frozen], p_old[frozen]) and torch.equal(ref["p"][frozen], p_old[frozen].double())
        # the step is not a no-op: the floor the kernel tests assert holds here too
        moved = (ref["p"] - p_old.double())[tab.seg_of == 1].norm() / p_old[tab.seg_of == 1].double().norm()
        assert float(moved) >= 1e-2
        st = {k: (getattr(opt, k).clone() if getattr(opt, k) is not None else st[k]) for k in st}


def _shard_piece_bounds(store, world):
    """Every boundary of every rank's piece, the way GradReducer cuts them in ZeRO-1 mode."""
    from jumbo_mae_tpu_amd.models.params import ALIGN
    from jumbo_mae_tpu_amd.parallel.ddp import plan_buckets, shard_ranges, split_oversized, unit_key
    segs = [s for s in store.segments if s.trainable]
    limit = int(64.0 * 1024 * 1024 / 4)
    buckets = []
    for idxs in plan_buckets([s.numel for s in segs], [unit_key(s.path) for s in segs], limit):
        buckets.append((min(segs[i].offset for i in idxs), max(segs[i].offset + segs[i].numel for i in idxs)))
    q = world * ALIGN
    ranges = split_oversized(shard_ranges(buckets, q), [(s.offset, s.numel) for s in segs if s.numel > limit], q)
    out = []
    for lo, hi in ranges:
        assert (hi - lo) % world == 0
        n = (hi - lo) // world
        out += [lo + r * n for r in range(world + 1)]
    return out


@pytest.mark.parametrize("name", ["vit_base_patch16", "vit_large_patch16", "vit_huge_patch14"])
def test_chunk_starts_are_16_byte_aligned(name):
    """What adamw_kernel's 16-byte accesses (float4 on p / g / mu / nu, 8 bytes on the bf16 shadow)
    rely on: every chunk start is a multiple of 4 elements.  Chunk starts are segment offsets plus
    multiples of CHUNK, or ZeRO-1 piece boundaries plus multiples of CHUNK; so every segment offset and
    CHUNK are multiples of 4 and every piece boundary is a multiple of ALIGN, for the encoders with
    their decoder and for the 1000-label classifier.  (Offsets are NOT all multiples of 64: fused
    handles keep their segments adjacent.)  Offsets are assigned at construction: nothing is allocated."""
    from jumbo_mae_tpu_amd.config import decoder_config, vit_config
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.models.params import ALIGN
    from jumbo_mae_tpu_amd.optim import flat
    patch = vit_config(name).patch_size
    stores = [PretrainModel(vit_config(name, labels=0), decoder_config(patch_size=patch)).store,
              FinetuneModel(vit_config(name, labels=1000)).store]
    assert flat.CHUNK % 4 == 0 and ALIGN % 4 == 0
    for store in stores:
        assert store.master is None  # not finalized
        assert [s.key for s in store.segments if s.offset % 4] == []
        for world in (2, 3, 8):
            assert [b for b in _shard_piece_bounds(store, world) if b % ALIGN] == []
