"""Device validation transform on the GPU (csrc/augment.hip jm_window_resize): the window-resize
kernels must equal PIL's Resize(int(size / ratio), bicubic) -> CenterCrop(size) -> PILToTensor and
the NumPy mirror (data/resample_ref.py) bit for bit, write 255 for pad rows, read nothing outside the
shipped windows, and pass the debug build's bounds checks; then the same through the real loader and
the DevicePrefetcher against the PIL loader."""

import functools
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (W, H) at S = 32, Resize(36): unchanged, one identity pass, upscale, odd sizes (crop origin on x.5),
# extreme aspects, and one over the tap budget (resized in the worker) -- tests/test_device_valid.py
SIZES = [(36, 36), (36, 50), (50, 36), (20, 31), (97, 61), (61, 97), (64, 200), (333, 40), (400, 300)]
PADS = 3


def _images(sizes, seed):
    rs = np.random.default_rng(seed)
    return [Image.fromarray(rs.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in sizes]


@functools.lru_cache(maxsize=None)
def _batch(size):
    """(packed batch with PADS pad rows, labels, PIL reference) -- computed once, never modified."""
    from jumbo_mae_tpu_amd.data.loader import DeviceValidParams, collate_and_pad, collate_valid_packed
    from jumbo_mae_tpu_amd.data.transforms import create_transforms
    ims = _images(SIZES if size == 32 else [(500, 375), (375, 500), (224, 256)], seed=size)
    dev_t, pil_t = DeviceValidParams(size, 0.875), create_transforms("rrc", size, "none", 0.0, 0.0, 0.875)[1]
    n = len(ims) + PADS
    p, labels = collate_valid_packed([(dev_t(im), k) for k, im in enumerate(ims)], batch_size=n, size=size)
    want, want_labels = collate_and_pad([(pil_t(im), k) for k, im in enumerate(ims)], batch_size=n)
    assert torch.equal(labels, want_labels)
    return p, labels, want


def _run(p):
    from jumbo_mae_tpu_amd.data.loader import unpack_on_device
    out = unpack_on_device(p, torch.device("cuda"))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("size", [32, 224])
def test_kernel_equals_pil_and_mirror(size):
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    p, _, want = _batch(size)
    out = _run(p)
    assert out.dtype == torch.uint8 and out.shape == want.shape
    assert torch.equal(out, want), (out.int() - want.int()).abs().amax((1, 2, 3))
    assert torch.equal(out, torch.from_numpy(unpack_packed(p)))
    assert (out[-PADS:] == 255).all()
    assert torch.equal(_run(p), out)  # deterministic


def test_nothing_outside_the_windows_is_read():
    """The same windows with 0xAA bytes before, between and after them give the same batch."""
    from jumbo_mae_tpu_amd.data.loader import PackedImages
    p, _, want = _batch(32)
    src, tab = p.src.numpy(), p.tab.numpy().copy()
    gap, parts, off = 257, [], 0
    for d in tab:
        n = int(d[1] * d[2] * 3)
        parts += [np.full(gap, 0xAA, np.uint8), src[int(d[0]):int(d[0]) + n]]
        d[0] = off + gap  # pad rows too: their offset points into the poison, and must never be used
        off += gap + n
    parts.append(np.full(gap, 0xAA, np.uint8))
    q = PackedImages(torch.from_numpy(np.concatenate(parts)), torch.from_numpy(tab), p.tmp_bytes, p.rows_max, p.size)
    assert torch.equal(_run(q), want)


def test_pad_rows_need_no_source():
    """A batch of pad rows only, with a single byte of src: 255 everywhere."""
    from jumbo_mae_tpu_amd.data.loader import WIN_TAB, PackedImages
    tab = torch.zeros(4, WIN_TAB, dtype=torch.int64)
    tab[:, 17] = 1
    for size in (32, 37):  # 37: the last 16-row block is partial
        out = _run(PackedImages(torch.full((1,), 7, dtype=torch.uint8), tab, 0, 0, size))
        assert out.shape == (4, 3, size, size) and (out == 255).all()


def test_binding_rejects_bad_arguments():
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    p, _, _ = _batch(32)
    dev = torch.device("cuda")
    src, tab = p.src.to(dev), p.tab.to(dev)
    assert ext.window_tab() == 18
    with pytest.raises(RuntimeError):
        ext.window_resize(p.src, tab, 32, p.tmp_bytes, p.rows_max)  # host src
    with pytest.raises(RuntimeError):
        ext.window_resize(src, tab[:, :13].contiguous(), 32, p.tmp_bytes, p.rows_max)  # the train table
    with pytest.raises(RuntimeError):
        ext.window_resize(src, tab.int(), 32, p.tmp_bytes, p.rows_max)
    with pytest.raises(RuntimeError):
        ext.window_resize(src, tab.t().contiguous().t(), 32, p.tmp_bytes, p.rows_max)  # not contiguous
    with pytest.raises(RuntimeError):
        ext.window_resize(src, tab, 0, p.tmp_bytes, p.rows_max)
    with pytest.raises(RuntimeError):
        ext.window_resize(src, tab, 32, 0, p.rows_max)  # rows without scratch
    with pytest.raises(RuntimeError):
        ext.rrc_resize(src, tab, 32, p.tmp_bytes, p.rows_max)  # the 13-column entry keeps its contract


SCRIPT = textwrap.dedent("""
    import sys
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.__name__.endswith("_C_debug") and ext.debug_build
    sys.path.insert(0, "tests")
    import test_device_valid_gpu as T  # the same batches as the release-build tests
    from jumbo_mae_tpu_amd.data.loader import unpack_on_device
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    for size in (32, 224):
        p, _, want = T._batch(size)
        out = unpack_on_device(p, torch.device("cuda"))
        torch.cuda.synchronize()
        lines = ext.debug_lines()
        assert not lines, dict(lines)
        assert torch.equal(out.cpu(), want)
    print("DEBUG_VALID_OK")
""")


def test_debug_build_checks_clean():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0 and "DEBUG_VALID_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_through_the_loader_and_prefetcher(tmp_path):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.train.common import DevicePrefetcher

    def args(spec):
        return SimpleNamespace(random_crop="rrc", image_size=224, auto_augment="none", color_jitter=0.0,
                               random_erasing=0.0, test_crop_ratio=0.875, train_dataset_shards=None,
                               valid_dataset_shards=spec, mode="finetune", train_batch_size=8, grad_accum=1,
                               augment_repeats=1, shuffle_seed=1, train_loader_workers=0, valid_batch_size=8,
                               valid_loader_workers=2)

    spec = write_shards(str(tmp_path), shards=2, per_shard=10, classes=5, seed=11, prefix="valid")
    _, cpu = create_dataloaders(args(spec))
    _, dev = create_dataloaders(args(spec), device_valid=True)
    n = pads = 0
    for (a, la), (b, lb) in zip(cpu, DevicePrefetcher(dev, torch.device("cuda")), strict=True):
        torch.cuda.synchronize()
        assert b.is_cuda and b.dtype == torch.uint8 and lb.is_cuda
        assert torch.equal(lb.cpu(), la)
        assert torch.equal(b.cpu(), a), (b.cpu().int() - a.int()).abs().max()
        assert (b.cpu()[la == -1] == 255).all()
        n += 1
        pads += int((la == -1).sum())
    assert n >= 3 and pads == n * 8 - 20 and pads > 0  # 20 images in batches of 8: padded final batches
