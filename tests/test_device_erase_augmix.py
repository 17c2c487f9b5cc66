"""Device random erasing and AugMix, CPU side: the describing twins (RandomErasing.describe,
AugMix.describe) make the PIL path's draws -- both RNG streams end in the same state -- the NumPy
mirrors (data/augment_ref.py augmix_mix / erase_paste) reproduce the PIL transform bit for bit, alone,
as the whole train transform and through the loader (repeats, workers, resume), collate rejects
malformed tables, and ``--device-augment all`` routes as documented while auto / on / off keep
their behaviour."""

import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from jumbo_mae_tpu_amd.data import autoaugment as A
from jumbo_mae_tpu_amd.data import augment_ref as R

AUGMIX_SPECS = ["augmix-m3-w3-d-1", "augmix-m5-w1-d2", "augmix-m3-w3-d2-b1", "augmix-m9-w5-d1"]


def _chw(im):
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _states():
    return random.getstate(), np.random.get_state()


def _same_states(a, b):
    assert a[0] == b[0]  # random
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]  # np.random


# ---- erasing
@pytest.mark.parametrize("size", [33, 64])
def test_erasing_describe_makes_the_same_draws_and_pixels(size):
    from jumbo_mae_tpu_amd.data.transforms import RandomErasing
    t = RandomErasing(0.75)
    img = np.random.default_rng(size).integers(0, 256, (3, size, size), dtype=np.uint8)
    erased = 0
    for s in range(64):
        _seed(s)
        want = t(img)
        after = _states()
        _seed(s)
        box, fill = t.describe(size)
        _same_states(after, _states())
        assert box.dtype == np.int64 and box.shape == (4,) and fill.dtype == np.uint8
        assert fill.shape == (3, box[2], box[3])
        got = R.erase_paste(img[None], np.array([[*box, 0]], np.int64), fill.reshape(-1))[0]
        assert np.array_equal(got, want), s
        assert (box[2] > 0) == (not np.array_equal(want, img))
        erased += int(box[2] > 0)
    assert 0 < erased < 64, erased  # erased and non-erased samples both occur


# ---- AugMix
def _augmix(spec, size):
    from jumbo_mae_tpu_amd.data.transforms import auto_augment_factory
    t = auto_augment_factory(spec, size)
    assert isinstance(t, A.AugMix)
    return t


def test_augmix_slots():
    assert [(_augmix(s, 32).width, _augmix(s, 32).chain_slots, _augmix(s, 32).slots, _augmix(s, 32).blended)
            for s in AUGMIX_SPECS] == [(3, 3, 9, False), (1, 2, 2, False), (3, 2, 6, True), (5, 1, 5, False)]


@pytest.mark.parametrize("size", [48, 33])
@pytest.mark.parametrize("spec", AUGMIX_SPECS)
def test_augmix_describe_makes_the_same_draws_and_pixels(spec, size):
    t = _augmix(spec, size)
    W, D = t.width, t.chain_slots
    im = Image.fromarray(np.random.default_rng(size).integers(0, 256, (size, size, 3), dtype=np.uint8))
    a = _chw(im)
    kinds = set()
    for s in range(32):
        _seed(s)
        want = _chw(t(im))
        after = _states()
        _seed(s)
        recs, mix = t.describe(size)
        _same_states(after, _states())
        assert len(recs) == W * D == t.slots and mix.shape == (W + 1,) and mix.dtype == np.float32
        chain = np.stack(recs).reshape(W, D, A.AUG_P)
        kinds.update(int(k) for k in chain[:, :, 0].reshape(-1))
        chains = R.apply_chain(np.repeat(a[None], W, axis=0), chain)
        got = R.augmix_mix(a[None], chains, mix[None], t.blended)[0]
        assert np.array_equal(got, want), (s, np.abs(got.astype(int) - want.astype(int)).max())
    assert len(kinds) >= 4, kinds


def test_mix_mirror_on_hand_built_tables():
    rs = np.random.default_rng(1)
    S, W = 9, 3
    orig = rs.integers(0, 256, (4, 3, S, S), dtype=np.uint8)
    chains = rs.integers(0, 256, (4 * W, 3, S, S), dtype=np.uint8)
    chains[3 * W:] = 255
    third = np.float32(1) / np.float32(3)
    over = np.array([0.5, 0.3, 0.2000001], np.float32)  # float32 sum above 1: 255-valued pixels exceed 255
    assert np.float32(np.float32(np.float32(0) + over[0] * np.float32(255)) + over[1] * np.float32(255)) \
        + over[2] * np.float32(255) > np.float32(255)
    table = np.array([[third, third, third, 0.0],  # m = 0: the original
                      [third, third, third, 1.0],  # m = 1: the mixed image
                      [0.0, 1.0, 0.0, 1.0],  # one weight 1: that chain
                      [*over, 1.0]], np.float32)  # the clip
    got = R.augmix_mix(orig, chains, table, False)
    assert np.array_equal(got[0], orig[0])
    mixed = np.zeros((3, S, S), np.float32)
    for k in range(W):
        mixed += third * chains[W + k].astype(np.float32)
    assert np.array_equal(got[1], mixed.astype(np.uint8))
    assert np.array_equal(got[2], chains[2 * W + 1])
    assert (got[3] == 255).all()
    # blended: alpha 1 takes the chain, alpha 0 keeps the running image
    tb = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.25, 1.0, 0.0, 0.0], [0.5, 0.5, 1.0, 0.0]], np.float32)
    got = R.augmix_mix(orig, chains, tb, True)
    assert np.array_equal(got[0], chains[0]) and np.array_equal(got[1], orig[1])
    assert np.array_equal(got[2], chains[2 * W + 1]) and (got[3] == 255).all()
    w = A.AugMix.blended_weights(np.array([0.2, 0.3, 0.5], np.float32), 0.8)
    rest = np.cumprod((1 - w.astype(np.float64))[::-1])[::-1]  # weight left on chain k by the later steps
    assert np.allclose(w * np.append(rest[1:], 1.0), 0.8 * np.array([0.2, 0.3, 0.5]), atol=1e-6)


# ---- the whole train transform
def _describing(size, aa, cj, re):
    from jumbo_mae_tpu_amd.data.loader import DeviceTrainParams
    from jumbo_mae_tpu_amd.data.transforms import ColorJitter, RandomErasing, auto_augment_factory
    return DeviceTrainParams(size, auto_augment_factory(aa, size), ColorJitter(cj, cj, cj) if cj > 0 else None,
                             RandomErasing(re) if re > 0 else None)


COMBOS = [(aa, cj) for aa in ("rand-m9-mstd0.5-inc1", "augmix-m3-w3-d-1") for cj in (0.0, 0.4)]


@pytest.mark.parametrize("aa,cj", COMBOS)
def test_whole_transform_equals_pil(aa, cj):
    from jumbo_mae_tpu_amd.data.loader import PackedImages, collate_packed
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    from jumbo_mae_tpu_amd.data.transforms import create_transforms
    size = 64
    pil_t = create_transforms("rrc", size, aa, cj, 0.75)[0]
    dev_t = _describing(size, aa, cj, 0.75)
    rs = np.random.default_rng(7)
    want, items = [], []
    for k in range(32):
        im = Image.fromarray(rs.integers(0, 256, (80, 96, 3), dtype=np.uint8))
        _seed(k)
        want.append(pil_t(im))
        after = _states()
        _seed(k)
        items.append(dev_t(im))
        _same_states(after, _states())
    p = collate_packed(items, size=size)
    assert isinstance(p, PackedImages)
    augmix = aa.startswith("augmix")
    tail = 3 if cj else 0
    assert p.chain.shape == (32, (9 if augmix else 2) + tail, A.AUG_P)
    assert (p.mix_wdb, None if p.mix is None else (p.mix.shape, p.mix.dtype)) == \
        (((3, 3, 0), ((32, 4), torch.float32)) if augmix else (None, None))
    assert p.erase.shape == (32, 5) and p.erase.dtype == torch.int64 and p.fill.dtype == torch.uint8
    n = (p.erase[:, 2] > 0).sum()
    assert 0 < n < 32 and p.fill.numel() == int((3 * p.erase[:, 2] * p.erase[:, 3]).sum())
    assert np.array_equal(unpack_packed(p), np.stack(want))


def test_old_items_and_constructors_keep_working():
    from jumbo_mae_tpu_amd.data.loader import PackedImages, collate_packed
    t = _describing(32, "rand-m9-mstd0.5-inc1", 0.4, 0.0)
    _seed(0)
    item = t(Image.fromarray(np.zeros((40, 40, 3), np.uint8)))
    assert len(item) == 3 and t.mix_wdb is None
    p = collate_packed([item], size=32)
    assert p.mix is None and p.mix_wdb is None and p.erase is None and p.fill is None
    q = PackedImages(p.src, p.tab, p.tmp_bytes, p.rows_max, p.size, p.chain)
    assert q.mix is None and q.erase is None
    assert PackedImages._fields[:6] == ("src", "tab", "tmp_bytes", "rows_max", "size", "chain")
    # erasing alone: no chain slots, no mix
    t = _describing(32, "none", 0.0, 0.75)
    item = t(Image.fromarray(np.zeros((40, 40, 3), np.uint8)))
    assert len(item) == 6 and item[2].shape == (0, A.AUG_P) and item[3] is None
    with pytest.raises(ValueError, match="chains"):
        _describing(32, "augmix-m3-w9", 0.0, 0.0)


# ---- through the loader
def _args(spec, aa="augmix-m3-w3-d-1", cj=0.4, re=0.75, size=48, batch=8, **kw):
    d = dict(random_crop="rrc", image_size=size, auto_augment=aa, color_jitter=cj, random_erasing=re,
             test_crop_ratio=0.875, train_dataset_shards=spec, valid_dataset_shards=None, mode="finetune",
             train_batch_size=batch, grad_accum=1, augment_repeats=2, shuffle_seed=1, train_loader_workers=2,
             valid_batch_size=batch, valid_loader_workers=0)
    d.update(kw)
    return SimpleNamespace(**d)


def _take(dl, n):
    out = []
    for b in dl:
        out.append(b)
        if len(out) == n:
            break
    assert len(out) == n
    return out


@pytest.mark.parametrize("workers", [0, 2])
def test_device_batches_equal_pil_batches_through_the_loader(workers):
    from jumbo_mae_tpu_amd.data.loader import PackedImages, create_dataloaders
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    a = _args("synthetic:64:5", train_loader_workers=workers)
    cpu = _take(create_dataloaders(a)[0], 4)
    dev = _take(create_dataloaders(a, device_augment=True)[0], 4)
    erased = []
    for (x, lx), (p, lp) in zip(cpu, dev):
        assert isinstance(p, PackedImages) and p.mix_wdb == (3, 3, 0) and p.chain.shape == (8, 12, A.AUG_P)
        assert torch.equal(lx, lp)
        assert np.array_equal(unpack_packed(p), x.numpy())
        erased += (p.erase[:, 2] > 0).tolist()
    assert any(erased) and not all(erased)
    # a resumed loader continues the same stream
    res = _take(create_dataloaders(a, start_batches=2, device_augment=True)[0], 2)
    for (p, lp), (q, lq) in zip(res, dev[2:]):
        assert torch.equal(lp, lq)
        for f in ("src", "tab", "chain", "mix", "erase", "fill"):
            assert torch.equal(getattr(p, f), getattr(q, f)), f
    for (p, _), (x, _) in zip(res, cpu[2:]):
        assert np.array_equal(unpack_packed(p), x.numpy())


# ---- collate validation
def test_collate_rejects_bad_tables():
    from jumbo_mae_tpu_amd.data.loader import check_erase, check_mix, collate_packed
    S = 32
    t = _describing(S, "augmix-m3-w3-d-1", 0.0, 1.0)
    _seed(2)
    win, desc, chain, mix, box, fill = t(Image.fromarray(np.zeros((40, 40, 3), np.uint8)))
    assert box[2] > 0
    p = collate_packed([(win, desc, chain, mix, box, fill)] * 2, size=S)
    assert p.erase[:, 4].tolist() == [0, fill.size] and p.fill.numel() == 2 * fill.size

    def boxed(i, j, eh, ew):
        b = np.array([i, j, eh, ew], np.int64)
        return (win, desc, chain, mix, b, np.zeros((3, max(eh, 0), max(ew, 0)), np.uint8))

    for bad in ((S - 3, 0, 4, 4), (0, S - 3, 4, 4), (-1, 0, 4, 4), (0, -1, 4, 4)):  # leaves [0, S)
        with pytest.raises(ValueError, match="leaves"):
            collate_packed([boxed(*bad)], size=S)
    for bad in ((0, 0, S, 4), (0, 0, 4, S), (0, 0, S + 1, 1)):  # eh >= S or ew >= S
        with pytest.raises(ValueError, match="rows and columns"):
            collate_packed([boxed(*bad)], size=S)
    for bad in ((0, 0, -2, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        with pytest.raises(ValueError, match="erase"):
            collate_packed([boxed(*bad)], size=S)
    collate_packed([boxed(0, 0, S - 1, S - 1), boxed(S - 1, S - 1, 1, 1), boxed(0, 0, 0, 0)], size=S)  # the extremes pass
    # a fill of the wrong length or dtype, a box of the wrong shape
    with pytest.raises(ValueError, match="fill"):
        collate_packed([(win, desc, chain, mix, box, fill[:, 1:])], size=S)
    with pytest.raises(ValueError, match="fill"):
        collate_packed([(win, desc, chain, mix, box, fill.astype(np.int16))], size=S)
    with pytest.raises(ValueError, match="box"):
        collate_packed([(win, desc, chain, mix, box.astype(np.int32), fill)], size=S)
    # offsets and lengths against the fill buffer
    ok = np.array([[1, 2, 3, 4, 10]], np.int64)
    check_erase(ok, 10 + 36, S)
    for tab, n in ((ok, 10 + 35), (np.array([[1, 2, 3, 4, -1]], np.int64), 100), (ok, 0)):
        with pytest.raises(ValueError, match="fill buffer"):
            check_erase(tab, n, S)
    with pytest.raises(ValueError, match=r"int64 \[B, 5\]"):
        check_erase(ok[:, :4], 100, S)
    with pytest.raises(ValueError, match=r"int64 \[B, 5\]"):
        check_erase(ok.astype(np.int32), 100, S)
    # mix tables: shape, dtype, non-finite values
    vals, wdb = mix
    assert wdb == (3, 3, 0) and vals.shape == (4,)
    for bad in (vals[:3], vals.astype(np.float64), np.append(vals, np.float32(0))):
        with pytest.raises(ValueError, match=r"float32 \[B, 4\]"):
            collate_packed([(win, desc, chain, (bad, wdb), box, fill)], size=S)
    for v in (np.nan, np.inf, -np.inf):
        bad = vals.copy()
        bad[1] = v
        with pytest.raises(ValueError, match="non-finite"):
            collate_packed([(win, desc, chain, (bad, wdb), box, fill)], size=S)
    with pytest.raises(ValueError, match="disagree"):
        collate_packed([(win, desc, chain, mix, box, fill), (win, desc, chain, (vals, (3, 3, 1)), box, fill)], size=S)
    with pytest.raises(ValueError, match="slots"):
        check_mix(np.zeros((2, 4), np.float32), (3, 4, 0), 9)  # more chain slots than the op chain has
    with pytest.raises(ValueError, match="chains"):
        check_mix(np.zeros((2, 10), np.float32), (9, 1, 0), 9)


# ---- gating
def test_gating_all(monkeypatch):
    from jumbo_mae_tpu_amd.data.loader import device_augment_all_ok, device_augment_ok
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.train import common as C

    def args(**kw):
        d = dict(aa="rand-m9-mstd0.5-inc1", cj=0.0, re=0.0)
        d.update(kw)
        return _args("x-{0..1}.tar", **d)

    for aa in ("none", "rand-m9-mstd0.5-inc1", "v0r", "original-mstd0.5", "augmix-m3-w3-d-1", "augmix-m3-w3-d2-b1"):
        for cj in (0.0, 0.4):
            for re in (0.0, 0.25):
                assert device_augment_all_ok(args(aa=aa, cj=cj, re=re)), (aa, cj, re)
                assert device_augment_ok(args(aa=aa, cj=cj, re=re)) == (not aa.startswith("augmix") and re == 0.0)
    for crop in ("src", "none"):
        assert not device_augment_all_ok(args(random_crop=crop))
        assert not device_augment_all_ok(args(random_crop=crop, re=0.25))

    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    monkeypatch.setattr(_ext, "available", lambda: True)
    new = (dict(re=0.25), dict(aa="augmix-m3-w3-d-1"), dict(aa="augmix-m3-w3-d-1", re=0.25, cj=0.4))
    for kw in new + (dict(), dict(aa="none")):
        assert C.use_device_augment(args(device_augment="all", **kw), cuda) is True
        assert C.use_device_augment(args(device_augment="all", **kw), cpu) is False
        assert C.use_device_augment(args(device_augment="all", train_dataset_shards=None, **kw), cuda) is False
    for crop in ("src", "none"):
        with pytest.raises(SystemExit, match="host"):
            C.use_device_augment(args(device_augment="all", random_crop=crop), cuda)
    assert C.use_device_valid(args(device_augment="all", valid_dataset_shards="v-{0..1}.tar", re=0.25), cuda) is True
    assert C.use_device_valid(args(device_augment="all", valid_dataset_shards="v-{0..1}.tar"), cpu) is False

    # auto / on / off: unchanged for every case tests/test_device_randaug.py::test_gating lists
    assert C.use_device_augment(args(device_augment="auto"), cuda) is False
    assert C.use_device_augment(args(device_augment="auto", aa="none", cj=0.4), cuda) is False
    assert C.use_device_augment(args(device_augment="auto", aa="none"), cuda) is True
    assert C.use_device_augment(args(device_augment="on"), cuda) is True
    assert C.use_device_augment(args(device_augment="off"), cuda) is False
    for kw in (dict(aa="augmix-m3-w3-d-1"), dict(re=0.25), dict(random_crop="src"), dict(random_crop="none")):
        with pytest.raises(SystemExit, match="host"):
            C.use_device_augment(args(device_augment="on", **kw), cuda)
        assert C.use_device_augment(args(device_augment="auto", **kw), cuda) is False
        assert C.use_device_augment(args(device_augment="off", **kw), cuda) is False

    monkeypatch.setattr(_ext, "available", lambda: False)
    for kw in new:
        with pytest.raises(SystemExit, match="extension"):
            C.use_device_augment(args(device_augment="all", **kw), cuda)
    with pytest.raises(SystemExit, match="extension"):
        C.use_device_augment(args(device_augment="on"), cuda)
    assert C.use_device_augment(args(device_augment="auto", aa="none"), cuda) is False


def test_cli_parses_device_augment_all():
    from jumbo_mae_tpu_amd.train.cli import finetune_parser, pretrain_parser
    f = finetune_parser().parse_args(["--device-augment", "all"])
    assert f.device_augment == "all" and f.random_erasing == 0.25  # the default finetune flags need 'all'
    assert pretrain_parser().parse_args(["--device-augment", "all"]).device_augment == "all"
    assert finetune_parser().parse_args([]).device_augment == "auto"
    with pytest.raises(SystemExit):
        finetune_parser().parse_args(["--device-augment", "everything"])


def test_create_dataloaders_routes_by_the_args():
    """device_augment=True builds the extended params only when the args need them."""
    from jumbo_mae_tpu_amd.data.loader import DeviceRRCParams, DeviceTrainParams, create_dataloaders
    plain = create_dataloaders(_args("synthetic:16:5", aa="none", cj=0.0, re=0.0), device_augment=True)[0].dataset.transform
    assert type(plain) is DeviceRRCParams
    old = create_dataloaders(_args("synthetic:16:5", aa="v0", cj=0.0, re=0.0), device_augment=True)[0].dataset.transform
    assert type(old) is DeviceTrainParams and old.erase is None and old.mix_wdb is None
    new = create_dataloaders(_args("synthetic:16:5"), device_augment=True)[0].dataset.transform
    assert new.erase is not None and new.erase.p == 0.75 and new.mix_wdb == (3, 3, 0) and new.slots == 12
    with pytest.raises(AssertionError, match="host"):
        create_dataloaders(_args("synthetic:16:5", random_crop="src"), device_augment=True)
