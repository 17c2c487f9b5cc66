"""Device random erasing and AugMix kernels (csrc/augment_chain.hip erase_paste_kernel /
augmix_mix_kernel): equal to their NumPy mirrors (data/augment_ref.py, pinned to PIL in
tests/test_device_erase_augmix.py) bit for bit -- per kernel on hand-built tables, as the whole
``unpack_on_device`` path, and through the real loader + DevicePrefetcher against the PIL loader.
Only well-formed tables reach the kernels; malformed arguments stop at the bindings' host checks."""

import functools
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


# ---- erase_paste
@functools.lru_cache(maxsize=None)
def _erase_case(S):
    """(images, table, fill, mirror result): the listed boxes, fill chunks in shuffled order."""
    from jumbo_mae_tpu_amd.data.augment_ref import erase_paste
    from jumbo_mae_tpu_amd.data.loader import check_erase
    rs = np.random.default_rng(S)
    imgs = rs.integers(0, 256, (B, 3, S, S), dtype=np.uint8)
    boxes = [(0, 0, 0, 0), (0, 0, 1, 1), (S - 1, S - 1, 1, 1), (0, 0, S - 1, S - 1), (1, 1, S - 1, S - 1),
             (5, 7, 6, 9), (2, (S - 12) | 1, 11, 11),  # odd column with an odd width
             (S - 4, 1, 3, S - 1), (3, 0, 2, S - 1)]  # strips of the full width minus one
    while len(boxes) < B:
        eh, ew = (int(v) for v in rs.integers(1, S, 2))
        boxes.append((int(rs.integers(0, S - eh + 1)), int(rs.integers(0, S - ew + 1)), eh, ew))
    boxes[11] = (0, 0, 0, 0)
    sizes = np.array([3 * eh * ew for _, _, eh, ew in boxes])
    order = rs.permutation(B)  # position of every image's chunk in the fill buffer
    offs = np.zeros(B, np.int64)
    offs[order] = np.concatenate([[0], np.cumsum(sizes[order])[:-1]])
    assert (np.diff(offs[sizes > 0]) < 0).any() and (np.diff(offs[sizes > 0]) > 0).any()  # non-monotonic
    table = np.array([[*b, o if n else 0] for b, o, n in zip(boxes, offs, sizes)], np.int64)
    fill = rs.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    check_erase(table, fill.size, S)
    ref = erase_paste(imgs, table, fill)
    assert np.array_equal(ref[0], imgs[0]) and np.array_equal(ref[11], imgs[11]) and (ref[3] != imgs[3]).any()
    return imgs, table, fill, ref


@pytest.mark.parametrize("hint", [True, False])
@pytest.mark.parametrize("S", [33, 64])
def test_erase_paste_equals_mirror(S, hint):
    imgs, table, fill, ref = _erase_case(S)
    x = torch.from_numpy(imgs).cuda()
    out = _ext().erase_paste(x, torch.from_numpy(table).cuda(), torch.from_numpy(fill).cuda(),
                             int((3 * table[:, 2] * table[:, 3]).max()) if hint else 0)
    torch.cuda.synchronize()
    assert out.data_ptr() == x.data_ptr()  # in place
    got = out.cpu().numpy()
    bad = [(b, table[b].tolist()) for b in range(B) if not np.array_equal(got[b], ref[b])]
    assert not bad, bad  # the whole image: nothing outside a box changed either


# ---- augmix_mix
@functools.lru_cache(maxsize=None)
def _mix_case(S, W, blended):
    from jumbo_mae_tpu_amd.data.augment_ref import augmix_mix
    from jumbo_mae_tpu_amd.data.loader import check_mix
    rs = np.random.default_rng(1000 * S + 10 * W + blended)
    orig = rs.integers(0, 256, (B, 3, S, S), dtype=np.uint8)
    chains = rs.integers(0, 256, (B * W, 3, S, S), dtype=np.uint8)
    chains[rs.integers(0, W)] = 255  # one all-255 and one all-0 chain image (images 0 and 1)
    chains[W + rs.integers(0, W)] = 0
    chains[2 * W:3 * W] = 255  # image 2: every chain 255, for the clip
    if blended:
        table = np.concatenate([rs.random((B, W)), np.zeros((B, 1))], axis=1).astype(np.float32)
        table[3, :W] = 0.0  # the original
        table[4, :W] = 1.0  # the last chain
        table[5, rs.integers(0, W)] = 1.0
    else:
        table = np.concatenate([rs.dirichlet([1.0] * W, B), rs.beta(1.0, 1.0, (B, 1))], axis=1).astype(np.float32)
        table[2, :W] = table[2, :W] * np.float32(1.0001) + np.float32(1e-6)  # float32 sum > 1 on 255-valued pixels
        table[2, W] = 1.0
        acc = np.float32(0)
        for w in table[2, :W]:
            acc = acc + w * np.float32(255)
        assert acc > np.float32(255)
        table[3, W] = 0.0  # m = 0: the original
        table[4, W] = 1.0  # m = 1: the mixed image
        table[5, :W] = 0.0  # one weight 1, the others 0
        table[5, rs.integers(0, W)] = 1.0
        table[6, W] = 1.0
    check_mix(table, (W, 1, blended), W)
    ref = augmix_mix(orig, chains, table, bool(blended))
    if not blended:
        assert (ref[2] == 255).all() and np.array_equal(ref[3], orig[3])
    return orig, chains, table, ref


@pytest.mark.parametrize("blended", [0, 1])
@pytest.mark.parametrize("W", [1, 3, 5])
@pytest.mark.parametrize("S", [33, 64, 70])  # 3 S S odd (byte path), a multiple of 16, a multiple of 4 only
def test_augmix_mix_equals_mirror(S, W, blended):
    orig, chains, table, ref = _mix_case(S, W, blended)
    o, c = torch.from_numpy(orig).cuda(), torch.from_numpy(chains).cuda()
    out = _ext().augmix_mix(o, c, torch.from_numpy(table).cuda(), bool(blended))
    torch.cuda.synchronize()
    assert out.data_ptr() not in (o.data_ptr(), c.data_ptr()) and torch.equal(o.cpu(), torch.from_numpy(orig))
    got = out.cpu().numpy()
    bad = [(b, table[b].tolist(), int(np.abs(got[b].astype(int) - ref[b]).max()))
           for b in range(B) if not np.array_equal(got[b], ref[b])]
    assert not bad, bad


def test_augmix_mix_unaligned_base_takes_the_byte_path():
    """A base pointer that is no multiple of 4 must not be read with vector loads."""
    orig, chains, table, ref = _mix_case(64, 3, 0)
    buf = torch.empty(chains.size + 1, dtype=torch.uint8, device="cuda")
    c = buf[1:].view(chains.shape)
    c.copy_(torch.from_numpy(chains))
    assert c.data_ptr() % 4 == 1 and c.is_contiguous()
    out = _ext().augmix_mix(torch.from_numpy(orig).cuda(), c, torch.from_numpy(table).cuda(), False)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- the whole path
COMBOS = [(aa, cj) for aa in ("rand-m9-mstd0.5-inc1", "augmix-m3-w3-d-1") for cj in (0.0, 0.4)]


@functools.lru_cache(maxsize=None)
def _packed(aa, cj, size=70, n=32, re=0.75):
    import random

    from PIL import Image

    from jumbo_mae_tpu_amd.data.loader import DeviceTrainParams, collate_packed
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    from jumbo_mae_tpu_amd.data.transforms import ColorJitter, RandomErasing, auto_augment_factory
    t = DeviceTrainParams(size, auto_augment_factory(aa, size), ColorJitter(cj, cj, cj) if cj > 0 else None,
                          RandomErasing(re))
    rs = np.random.default_rng(0)
    items = []
    for k in range(n):
        random.seed(k)
        np.random.seed(k)
        items.append(t(Image.fromarray(rs.integers(0, 256, (90, 120, 3), dtype=np.uint8))))
    p = collate_packed(items, size=size)
    erased = (p.erase[:, 2] > 0).sum()
    assert 0 < erased < n
    return p, unpack_packed(p)


@pytest.mark.parametrize("aa,cj", COMBOS)
def test_unpack_on_device_equals_mirror(aa, cj):
    from jumbo_mae_tpu_amd.data.loader import unpack_on_device
    p, ref = _packed(aa, cj)
    runs = []
    for _ in range(2):
        out = unpack_on_device(p, torch.device("cuda"))
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    bad = [b for b in range(len(ref)) if not np.array_equal(runs[0][b], ref[b])]
    assert not bad, (bad, p.erase[bad].tolist())
    assert np.array_equal(runs[0], runs[1])  # two runs are bit-identical


# ---- through the real loader
def _args(spec, aa, cj, batch=16):
    return SimpleNamespace(random_crop="rrc", image_size=96, auto_augment=aa, color_jitter=cj, random_erasing=0.75,
                           test_crop_ratio=0.875, train_dataset_shards=spec, valid_dataset_shards=None,
                           mode="finetune", train_batch_size=batch, grad_accum=1, augment_repeats=1, shuffle_seed=1,
                           train_loader_workers=2, valid_batch_size=batch, valid_loader_workers=0)


@pytest.mark.parametrize("aa,cj", [("rand-m9-mstd0.5-inc1", 0.0), ("augmix-m3-w3-d-1", 0.4)])
def test_matches_pil_through_the_loader(tmp_path, aa, cj):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.train.common import DevicePrefetcher
    spec = write_shards(str(tmp_path), shards=2, per_shard=24, classes=5, seed=9)
    cpu, _ = create_dataloaders(_args(spec, aa, cj))
    dev, _ = create_dataloaders(_args(spec, aa, cj), device_augment=True)
    erased = []

    def tap(dl):  # the erase tables of the batches on their way to the device
        for p, lb in dl:
            erased.extend((p.erase[:, 2] > 0).tolist())
            yield p, lb

    pf = DevicePrefetcher(tap(dev), torch.device("cuda"))
    n = 0
    for (a, la), (b, lb) in zip(cpu, pf):
        torch.cuda.synchronize()
        assert b.is_cuda and b.dtype == torch.uint8 and b.shape == a.shape
        assert torch.equal(lb.cpu(), la)
        assert torch.equal(b.cpu(), a), (b.cpu().int() - a.int()).abs().max()
        n += 1
        if n == 3:
            break
    assert n == 3
    assert any(erased[:48]) and not all(erased[:48])  # erased and non-erased images in those batches


# ---- debug build
SCRIPT = textwrap.dedent("""
    import numpy as np
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.__name__.endswith("_C_debug") and ext.debug_build
    import test_erase_augmix_gpu as T  # the same batch as the release-build test
    from jumbo_mae_tpu_amd.data.loader import unpack_on_device
    p, ref = T._packed("augmix-m3-w3-d-1", 0.4)
    assert p.mix is not None and p.chain.shape[1] == 12 and p.fill.numel() > 0
    out = unpack_on_device(p, torch.device("cuda"))
    torch.cuda.synchronize()
    _ext.debug_check()
    assert np.array_equal(out.cpu().numpy(), ref)
    print("DEBUG_ERASE_AUGMIX_OK")
""")


def test_debug_build_checks_clean_on_an_augmix_erasing_batch():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")])
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=path)
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0 and "DEBUG_ERASE_AUGMIX_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- bad arguments: stopped by the bindings' host checks, nothing is launched
def test_bindings_reject_bad_arguments():
    ext = _ext()
    S = 16
    img = torch.zeros(2, 3, S, S, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(2, 5, dtype=torch.int64, device="cuda")
    fill = torch.zeros(8, dtype=torch.uint8, device="cuda")
    for bad in (lambda: ext.erase_paste(img.float(), tab, fill), lambda: ext.erase_paste(img, tab.int(), fill),
                lambda: ext.erase_paste(img, tab, fill.float()), lambda: ext.erase_paste(img, tab[:, :4].contiguous(), fill),
                lambda: ext.erase_paste(img, tab[:1], fill), lambda: ext.erase_paste(img[:, :, :, :8].contiguous(), tab, fill),
                lambda: ext.erase_paste(img[:, :, :, ::2], tab, fill), lambda: ext.erase_paste(img, tab, fill.view(2, 4)),
                lambda: ext.erase_paste(img.cpu(), tab, fill), lambda: ext.erase_paste(img, tab, fill, -1),
                lambda: ext.erase_paste(img[:0], tab[:0], fill)):
        with pytest.raises(RuntimeError):
            bad()
    W = 3
    ch = torch.zeros(2 * W, 3, S, S, dtype=torch.uint8, device="cuda")
    mix = torch.zeros(2, W + 1, dtype=torch.float32, device="cuda")
    for bad in (lambda: ext.augmix_mix(img.float(), ch, mix, False), lambda: ext.augmix_mix(img, ch.float(), mix, False),
                lambda: ext.augmix_mix(img, ch, mix.double(), False), lambda: ext.augmix_mix(img, ch[:4], mix, False),
                lambda: ext.augmix_mix(img, ch, mix[:1], False), lambda: ext.augmix_mix(img, ch, mix[:, :1].contiguous(), False),
                lambda: ext.augmix_mix(img, torch.zeros(18, 3, S, S, dtype=torch.uint8, device="cuda"),
                                       torch.zeros(2, 10, device="cuda"), False),  # W = 9
                lambda: ext.augmix_mix(img, ch[:, :, :8].contiguous(), mix, False),
                lambda: ext.augmix_mix(img, ch, mix.t().contiguous().t(), False),
                lambda: ext.augmix_mix(img.cpu(), ch, mix, False), lambda: ext.augmix_mix(img[:0], ch[:0], mix[:0], False)):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()
    assert not img.any()
