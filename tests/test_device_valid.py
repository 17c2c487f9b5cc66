"""Device validation transform, CPU side: the worker-side descriptors (data/loader.py
DeviceValidParams), the padded packed collate and the NumPy mirror (data/resample_ref.py) reproduce
the PIL transform Resize(int(size / ratio), bicubic) -> CenterCrop(size) -> PILToTensor bit for bit,
pad rows included, and the switches route as documented."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

# (W, H) at S = 32, ratio 0.875 (Resize(36)): see the comments
SIZES = [(36, 36),  # Resize returns the image unchanged: both passes are the identity
         (36, 50), (50, 36),  # one pass is the identity
         (20, 31),  # upscale
         (97, 61), (61, 97),  # odd sizes; 36 * 97 / 61 -> 57, so the crop origin (57 - 32) / 2 lands on 12.5
         (64, 200), (333, 40),  # extreme aspect: the long axis is downscaled
         (400, 300)]  # 300 / 36 -> 35 taps, over the 24-tap budget: the worker resizes with PIL


def images(sizes, seed=0):
    rs = np.random.default_rng(seed)
    return [Image.fromarray(rs.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]


def pil_valid(size, ratio=0.875):
    from jumbo_mae_tpu_amd.data.transforms import create_transforms
    return create_transforms("rrc", size, "none", 0.0, 0.0, ratio)[1]


def _packed(ims, size, batch_size=None, ratio=0.875):
    from jumbo_mae_tpu_amd.data.loader import DeviceValidParams, collate_valid_packed
    t = DeviceValidParams(size, ratio)
    return collate_valid_packed([(t(im), k) for k, im in enumerate(ims)], batch_size=batch_size or len(ims), size=size)


@pytest.mark.parametrize("wh", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mirror_equals_pil_small(wh):
    from jumbo_mae_tpu_amd.data.loader import RRC_KMAX, WIN_TAB, _taps
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    im = images([wh], seed=wh[0] * 1000 + wh[1])[0]
    p, labels = _packed([im], 32)
    assert p.tab.shape == (1, WIN_TAB) and p.tab.dtype == torch.int64
    d = p.tab[0].tolist()
    H, W, oh, ow = d[5], d[6], d[13], d[14]
    assert max(_taps(H, oh), _taps(W, ow)) <= RRC_KMAX  # what is shipped fits the kernel's tap budget
    if wh == (400, 300):
        assert (W, H) == (48, 36) == (ow, oh)  # resized in the worker, shipped as an identity window
    else:
        assert (W, H) == wh
    if wh == (97, 61):
        assert (ow, oh, d[16], d[15]) == (57, 36, 12, 2)  # round(12.5) = 12: Python's rounding, as CenterCrop
    got = unpack_packed(p)
    assert np.array_equal(got[0], pil_valid(32)(im))
    assert labels.tolist() == [0]


def test_mirror_equals_pil_224():
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    ims = images([(500, 375), (375, 500), (224, 256)], seed=7)
    p, _ = _packed(ims, 224)
    want = np.stack([pil_valid(224)(im) for im in ims])
    assert np.array_equal(unpack_packed(p), want)


def test_shipped_window_is_what_the_passes_read():
    """Only the source pixels behind the 32 x 32 window travel, not the image."""
    p, _ = _packed(images([(64, 200)]), 32)
    d = p.tab[0].tolist()
    # Resize -> 36 x 112, crop rows 40 .. 71 of 112: about (32 + 2 * support) / 112 of the 200 rows
    assert d[1] < 80 and d[2] <= 64 and d[3] > 50 and p.src.numel() == d[1] * d[2] * 3


def test_padding_equals_collate_and_pad():
    from jumbo_mae_tpu_amd.data.loader import collate_and_pad
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    ims = images(SIZES[:5], seed=3)
    p, labels = _packed(ims, 32, batch_size=8)
    want_x, want_l = collate_and_pad([(pil_valid(32)(im), k) for k, im in enumerate(ims)], batch_size=8)
    got = unpack_packed(p)
    assert got.shape == tuple(want_x.shape) == (8, 3, 32, 32) and got.dtype == np.uint8
    assert (got[5:] == 255).all()
    assert labels.tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and labels.dtype == want_l.dtype
    assert torch.equal(labels, want_l)
    assert np.array_equal(got, want_x.numpy())
    assert p.tab[5:, 17].tolist() == [1, 1, 1] and (p.tab[5:, 1:3] == 0).all()  # fill flag, zero-size window


def _args(spec, workers=0, batch=5, size=32, **kw):
    d = dict(random_crop="rrc", image_size=size, auto_augment="none", color_jitter=0.0, random_erasing=0.0,
             test_crop_ratio=0.875, train_dataset_shards=None, valid_dataset_shards=spec, mode="finetune",
             train_batch_size=batch, grad_accum=1, augment_repeats=1, shuffle_seed=1, train_loader_workers=0,
             valid_batch_size=batch, valid_loader_workers=workers)
    d.update(kw)
    return SimpleNamespace(**d)


def test_through_the_loader(tmp_path):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.data.loader import PackedImages, create_dataloaders
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    spec = write_shards(str(tmp_path), shards=2, per_shard=6, classes=5, seed=4, prefix="valid")
    _, cpu = create_dataloaders(_args(spec), device_valid=False)
    _, dev = create_dataloaders(_args(spec), device_valid=True)
    n = 0
    for (a, la), (p, lb) in zip(cpu, dev, strict=True):
        assert isinstance(p, PackedImages) and p.size == 32
        assert torch.equal(la, lb)
        assert np.array_equal(unpack_packed(p), a.numpy())
        n += 1
    assert n == 3 and la.tolist()[2:] == [-1, -1, -1]  # 12 images in batches of 5: the last one is padded


def test_gating(monkeypatch, tmp_path):
    from jumbo_mae_tpu_amd.data.loader import PackedImages, create_dataloaders, device_valid_ok
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.train import common as C
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    monkeypatch.setattr(_ext, "available", lambda: True)
    for mode in ("auto", "on"):
        assert C.use_device_valid(_args("v-{0..1}.tar", device_augment=mode), cuda) is True
        assert C.use_device_valid(_args("v-{0..1}.tar", device_augment=mode), cpu) is False
        assert C.use_device_valid(_args(None, device_augment=mode), cuda) is False
        assert C.use_device_valid(_args("v-{0..1}.tar", device_augment=mode, test_crop_ratio=1.25), cuda) is False
        # the train transform's host-only parts do not concern the validation transform
        assert C.use_device_valid(_args("v-{0..1}.tar", device_augment=mode, random_erasing=0.25), cuda) is True
    assert C.use_device_valid(_args("v-{0..1}.tar", device_augment="off"), cuda) is False
    assert C.use_device_valid(_args("v-{0..1}.tar", device_augment="auto", test_crop_ratio=1.0), cuda) is True
    monkeypatch.setattr(_ext, "available", lambda: False)
    for mode in ("auto", "on"):  # no extension: the PIL path, and no new error
        assert C.use_device_valid(_args("v-{0..1}.tar", device_augment=mode), cuda) is False
    assert device_valid_ok(_args("x")) and not device_valid_ok(_args("x", test_crop_ratio=1.25))

    # device_augment=True alone leaves the validation loader on the PIL path
    a = _args("synthetic:6:3", train_dataset_shards="synthetic:6:3")
    _, valid = create_dataloaders(a, device_augment=True)
    x, _ = next(iter(valid))
    assert isinstance(x, torch.Tensor) and x.shape == (5, 3, 32, 32)
    _, valid = create_dataloaders(a, device_augment=True, device_valid=True)
    assert isinstance(next(iter(valid))[0], PackedImages)
    with pytest.raises(AssertionError, match="host"):
        create_dataloaders(_args("synthetic:6:3", test_crop_ratio=1.25), device_valid=True)


def test_collate_rejects_bad_descriptors():
    from jumbo_mae_tpu_amd.data.loader import DeviceRRCParams, DeviceValidParams, collate_valid_packed
    im = images([(50, 36)])[0]
    win, desc = DeviceValidParams(32)(im)
    collate_valid_packed([((win, desc), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="descriptor"):  # the 13-column train descriptor
        collate_valid_packed([(DeviceRRCParams(32)(im), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="descriptor"):
        collate_valid_packed([((win, desc[:17]), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="descriptor"):
        collate_valid_packed([((win, desc.astype(np.int32)), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="window"):
        collate_valid_packed([((win.astype(np.int16), desc), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="window"):
        collate_valid_packed([((win[1:], desc), 1)], batch_size=2, size=32)
    with pytest.raises(ValueError, match="smaller"):
        DeviceValidParams(32, 1.25)
