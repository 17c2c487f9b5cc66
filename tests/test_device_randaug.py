"""Device RandAugment, CPU side: the NumPy mirror of the op chain (data/augment_ref.py) is bit-exact
to the PIL ops it stands for, the describing train transform (data/loader.py DeviceTrainParams)
makes the PIL transform's draws -- no more, no fewer -- and the switches route as documented."""

import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

from jumbo_mae_tpu_amd.data import autoaugment as A
from jumbo_mae_tpu_amd.data import augment_ref as R

FILL = (124, 116, 104)


def _chw(im):
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def _images():
    rs = np.random.default_rng(0)
    ims = {f"random{s}": Image.fromarray(rs.integers(0, 256, (s, s, 3), dtype=np.uint8)) for s in (64, 70)}
    a = rs.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    a[..., 1] = 77  # one bin: autocontrast and equalize leave the band unchanged
    ims["constant_channel"] = Image.fromarray(a)
    ims["tiny8"] = Image.fromarray(rs.integers(0, 256, (8, 8, 3), dtype=np.uint8))  # equalize step == 0
    ims["step1"] = Image.fromarray(rs.integers(0, 256, (17, 16, 3), dtype=np.uint8))  # equalize step == 1
    g = np.zeros((70, 70, 3), np.uint8)  # narrow ranges: autocontrast stretches, equalize has empty bins
    g[..., 0] = np.arange(70)[:, None] * 2 + 40
    g[..., 1] = rs.integers(100, 130, (70, 70))
    g[..., 2] = rs.integers(0, 256, (70, 70))
    ims["narrow"] = Image.fromarray(g)
    return ims


IMAGES = _images()


def _same(im, pil_out, rec):
    got, want = R.apply_op(_chw(im), rec), _chw(pil_out)
    assert np.array_equal(got, want), (np.abs(got.astype(int) - want.astype(int)).max(), (got != want).mean())


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_mirror_lut_ops_equal_pil(name):
    im = IMAGES[name]
    _same(im, ImageOps.equalize(im), A.op_record(A.K_EQUALIZE))
    _same(im, ImageOps.autocontrast(im), A.op_record(A.K_AUTOCONTRAST))
    _same(im, ImageOps.invert(im), A.op_record(A.K_INVERT))
    for bits in range(8):
        _same(im, ImageOps.posterize(im, bits), A.op_record(A.K_POSTERIZE, bits))
    for t in (0, 1, 100, 255, 256):
        _same(im, ImageOps.solarize(im, t), A.op_record(A.K_SOLARIZE, t))
    for lvl in (0.0, 3.0, 10.0):
        _same(im, A.solarize_add(im, lvl, {}), A.op_record(A.K_SOLARIZE_ADD, int(lvl / 10 * 110)))


def test_mirror_edge_cases_leave_bands_unchanged():
    a = _chw(IMAGES["constant_channel"])
    for k in (A.K_EQUALIZE, A.K_AUTOCONTRAST):
        assert np.array_equal(R.apply_op(a, A.op_record(k))[1], a[1])
    t = _chw(IMAGES["tiny8"])
    assert np.array_equal(R.apply_op(t, A.op_record(A.K_EQUALIZE)), t)  # 64 pixels: step == 0


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_mirror_blends_equal_pil(name):
    im = IMAGES[name]
    for f in (0.0, 0.1, 0.37, 1.0, 1.3, 1.9):  # truncating branch (0 <= f <= 1) and clipping branch
        _same(im, ImageEnhance.Color(im).enhance(f), A.op_record(A.K_COLOR, f))
        _same(im, ImageEnhance.Brightness(im).enhance(f), A.op_record(A.K_BRIGHTNESS, f))
        _same(im, ImageEnhance.Contrast(im).enhance(f), A.op_record(A.K_CONTRAST, f))
        _same(im, ImageEnhance.Sharpness(im).enhance(f), A.op_record(A.K_SHARPNESS, f))


@pytest.mark.parametrize("resample", [Image.BILINEAR, Image.BICUBIC])
@pytest.mark.parametrize("name", ["random64", "random70", "tiny8"])
def test_mirror_affine_equals_pil(name, resample):
    im = IMAGES[name]
    W, H = im.size
    mats = [(1, 0.3, 0, 0, 1, 0), (1, -0.3, 0, 0, 1, 0), (1, 0, 0, 0.3, 1, 0), (1, 0, 0, -0.3, 1, 0),  # max shear
            (1, 0, 0.45 * W, 0, 1, 0), (1, 0, -0.45 * W, 0, 1, 0), (1, 0, 0, 0, 1, 0.45 * H),  # max translate
            (1, 0, 0, 0, 1, -0.45 * H), (1, 0.1234, 3.7, -0.2, 1, 1.1), (1, 0, 0.5, 0, 1, 0.25)]
    for m in mats:
        want = im.transform(im.size, Image.AFFINE, m, resample=resample, fillcolor=FILL)
        if m[2] or m[5] or m[1] or m[3]:
            assert (np.asarray(want) == np.array(FILL, np.uint8)).all(-1).any()  # fill pixels present
        _same(im, want, A.op_record(A.K_AFFINE, 0, m, resample, FILL))


@pytest.mark.parametrize("resample", [Image.BILINEAR, Image.BICUBIC])
def test_rotate_matrix_equals_pil_rotate(resample):
    """rotate_matrix reproduces the matrix Image.rotate builds (its rounding included); a level-0
    rotate is an identity record because PIL returns a copy."""
    for name in ("random64", "random70"):
        im = IMAGES[name]
        for deg in (0.0, 360.0, 30.0, -30.0, 12.34, -7.7, 1e-4, 90.0, 180.0, 270.0):
            m = A.rotate_matrix(deg, *im.size)
            assert (m is None) == (deg % 360.0 == 0)
            rec = A.op_record() if m is None else A.op_record(A.K_AFFINE, 0, m, resample, FILL)
            _same(im, im.rotate(deg, resample=resample, fillcolor=FILL), rec)
    random.seed(3)
    assert int(A._d_rotate(0.0, {}, 64)[0]) == A.K_IDENTITY


# ---- same draws
SPECS = [("rand-m9-mstd0.5-inc1", 0.0), ("rand-m15-n3-p0.7", 0.0), ("v0", 0.0), ("originalr-mstd0.5", 0.0),
         ("none", 0.4), ("rand-m9-mstd0.5-inc1", 0.4)]


def _describing(size, aa, cj):
    from jumbo_mae_tpu_amd.data.loader import DeviceTrainParams
    from jumbo_mae_tpu_amd.data.transforms import ColorJitter, auto_augment_factory
    return DeviceTrainParams(size, auto_augment_factory(aa, size), ColorJitter(cj, cj, cj) if cj > 0 else None)


@pytest.mark.parametrize("aa,cj", SPECS)
def test_describing_transform_makes_the_same_draws(aa, cj):
    from jumbo_mae_tpu_amd.data.loader import collate_packed
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    from jumbo_mae_tpu_amd.data.transforms import create_transforms
    size = 32
    rs = np.random.default_rng(5)
    im = Image.fromarray(rs.integers(0, 256, (48, 56, 3), dtype=np.uint8))
    pil_t, _ = create_transforms("rrc", size, aa, cj, 0.0, 0.875)
    dev_t = _describing(size, aa, cj)
    kinds = set()
    for k in range(200):
        random.seed(k)
        want = pil_t(im)
        after_pil = random.random()
        random.seed(k)
        item = dev_t(im)
        after_dev = random.random()
        assert after_pil == after_dev, k  # no draw missing or extra
        assert item[2].shape == (dev_t.slots, A.AUG_P) and item[2].dtype == np.float64
        kinds.update(int(v) for v in item[2][:, 0])
        got = unpack_packed(collate_packed([item], size=size))[0]
        assert np.array_equal(got, want), (k, item[2][:, 0])
    assert len(kinds) >= 3, kinds  # the seeds exercise several ops (colour jitter alone has three)


def test_chain_slot_counts():
    assert _describing(32, "rand-m9-mstd0.5-inc1", 0.4).slots == 2 + 3
    assert _describing(32, "rand-m15-n3-p0.7", 0.0).slots == 3
    assert _describing(32, "v0", 0.0).slots == 2
    assert _describing(32, "none", 0.4).slots == 3


def test_collate_rejects_unknown_kinds():
    from jumbo_mae_tpu_amd.data.loader import PackedImages, collate_packed
    random.seed(0)
    im = IMAGES["random64"]
    win, desc, chain = _describing(32, "rand-m9-mstd0.5-inc1", 0.0)(im)
    p = collate_packed([(win, desc, chain)], size=32)
    assert isinstance(p, PackedImages) and p.chain.shape == (1, 2, A.AUG_P) and p.chain.dtype == torch.float64
    assert PackedImages(p.src, p.tab, p.tmp_bytes, p.rows_max, p.size).chain is None  # old constructors keep working
    for bad in (float(A.AUG_KINDS), -1.0, 2.5):
        c = chain.copy()
        c[1, 0] = bad
        with pytest.raises(ValueError, match="kind"):
            collate_packed([(win, desc, c)], size=32)
    c = chain.copy()
    c[0] = A.op_record(A.K_AFFINE, 0, (1, 0, 0, 0, 1, 0), 0, FILL)  # nearest is not a RandAugment resample mode
    with pytest.raises(ValueError, match="resample"):
        collate_packed([(win, desc, c)], size=32)


# ---- through the loader
def _args(spec, aa="rand-m9-mstd0.5-inc1", cj=0.0, size=64, batch=8, **kw):
    d = dict(random_crop="rrc", image_size=size, auto_augment=aa, color_jitter=cj, random_erasing=0.0,
             test_crop_ratio=0.875, train_dataset_shards=spec, valid_dataset_shards=None, mode="finetune",
             train_batch_size=batch, grad_accum=1, augment_repeats=1, shuffle_seed=1, train_loader_workers=2,
             valid_batch_size=batch, valid_loader_workers=0)
    d.update(kw)
    return SimpleNamespace(**d)


def test_device_batches_equal_pil_batches_through_the_loader(tmp_path):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.data.loader import PackedImages, create_dataloaders
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    spec = write_shards(str(tmp_path), shards=2, per_shard=16, classes=5, seed=9)
    cpu, _ = create_dataloaders(_args(spec, cj=0.4))
    dev, _ = create_dataloaders(_args(spec, cj=0.4), device_augment=True)
    n = 0
    for (a, la), (p, lb) in zip(cpu, dev):
        assert isinstance(p, PackedImages) and p.chain.shape == (8, 5, A.AUG_P)
        assert torch.equal(la, lb)
        assert np.array_equal(unpack_packed(p), a.numpy())
        n += 1
        if n == 3:
            break
    assert n == 3


# ---- gating
def test_gating(monkeypatch):
    from jumbo_mae_tpu_amd.data.loader import device_augment_ok
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.train import common as C
    assert device_augment_ok(_args("x"))
    assert device_augment_ok(_args("x", aa="v0r", cj=0.4))
    assert device_augment_ok(_args("x", aa="none"))
    assert not device_augment_ok(_args("x", aa="augmix-m3-w3-d-1"))
    assert not device_augment_ok(_args("x", random_erasing=0.25))
    assert not device_augment_ok(_args("x", random_crop="src"))
    assert not device_augment_ok(_args("x", random_crop="none"))

    cuda = torch.device("cuda")
    monkeypatch.setattr(_ext, "available", lambda: True)
    ra = _args("x-{0..1}.tar", device_augment="auto")
    assert C.use_device_augment(ra, cuda) is False  # auto keeps its meaning: the pretraining transform only
    assert C.use_device_augment(_args("x-{0..1}.tar", aa="none", cj=0.4, device_augment="auto"), cuda) is False
    assert C.use_device_augment(_args("x-{0..1}.tar", aa="none", device_augment="auto"), cuda) is True
    ra.device_augment = "on"
    assert C.use_device_augment(ra, cuda) is True
    ra.device_augment = "off"
    assert C.use_device_augment(ra, cuda) is False
    for kw in (dict(aa="augmix-m3-w3-d-1"), dict(random_erasing=0.25), dict(random_crop="src")):
        with pytest.raises(SystemExit, match="host"):
            C.use_device_augment(_args("x-{0..1}.tar", device_augment="on", **kw), cuda)
        assert C.use_device_augment(_args("x-{0..1}.tar", device_augment="auto", **kw), cuda) is False
