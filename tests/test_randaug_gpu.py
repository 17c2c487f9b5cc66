"""Device RandAugment kernels (csrc/augment_chain.hip): the op chain on the GPU must equal the NumPy
mirror (data/augment_ref.py, itself pinned to PIL in tests/test_device_randaug.py) bit for bit, per
op kind and through the real loader + DevicePrefetcher against the PIL loader."""

import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (124, 116, 104)
B, SLOTS = 32, 4


def _records(S):
    """Every kind, both resample modes and the documented edge cases."""
    from jumbo_mae_tpu_amd.data import autoaugment as A
    recs = [A.op_record(A.K_INVERT), A.op_record(A.K_AUTOCONTRAST), A.op_record(A.K_EQUALIZE)]
    recs += [A.op_record(A.K_POSTERIZE, b) for b in (0, 4, 7)]
    recs += [A.op_record(A.K_SOLARIZE, t) for t in (0, 100, 256)]
    recs += [A.op_record(A.K_SOLARIZE_ADD, a) for a in (0, 33, 110)]
    for k in (A.K_COLOR, A.K_BRIGHTNESS, A.K_CONTRAST, A.K_SHARPNESS):
        recs += [A.op_record(k, f) for f in (0.1, 1.0, 1.9)]  # truncating and clipping blend branches
    mats = [(1, 0.3, 0, 0, 1, 0), (1, 0, 0, -0.3, 1, 0), (1, 0, 0.45 * S, 0, 1, 0), (1, 0, 0, 0, 1, -0.45 * S),
            A.rotate_matrix(30.0, S, S), A.rotate_matrix(-12.34, S, S)]  # maximum shear / translate / rotate
    for rs in (2, 3):
        recs += [A.op_record(A.K_AFFINE, 0, m, rs, FILL) for m in mats]
    assert A.rotate_matrix(0.0, S, S) is None  # a level-0 rotate is the identity record
    recs.append(A.op_record())
    assert {int(r[0]) for r in recs} == set(range(A.AUG_KINDS))
    return recs


@functools.lru_cache(maxsize=None)
def _case(S):
    """(images uint8 [B, 3, S, S], chain float64 [B, SLOTS, P], mirror result), computed once."""
    from jumbo_mae_tpu_amd.data import autoaugment as A
    from jumbo_mae_tpu_amd.data.augment_ref import apply_chain
    from jumbo_mae_tpu_amd.data.loader import check_chain
    rs = np.random.default_rng(S)
    imgs = rs.integers(0, 256, (B, 3, S, S), dtype=np.uint8)
    imgs[5, 1] = 77  # a constant channel: autocontrast and equalize leave the band unchanged
    near = np.full(S * S, 250, np.uint8)  # equalize step == 0: all but a few pixels in the last nonzero bin
    near[rs.choice(S * S, 90, replace=False)] = rs.integers(0, 250, 90)
    imgs[6, 2] = near.reshape(S, S)
    imgs[7] = rs.integers(90, 140, (3, S, S))  # narrow range: autocontrast stretches, equalize has empty bins
    chain = np.tile(A.op_record(), (B, SLOTS, 1))
    recs = _records(S)
    assert len(recs) <= 2 * B
    for j, r in enumerate(recs):  # different slot positions, identity records between the ops
        chain[j % B, (j % 4 + 2 * (j // B)) % 4] = r
    for b in (5, 6, 7):
        chain[b] = A.op_record()
    chain[5, 0], chain[5, 2] = A.op_record(A.K_AUTOCONTRAST), A.op_record(A.K_EQUALIZE)
    chain[6, 1], chain[6, 3] = A.op_record(A.K_EQUALIZE), A.op_record(A.K_AUTOCONTRAST)
    chain[7, 0], chain[7, 3] = A.op_record(A.K_AUTOCONTRAST), A.op_record(A.K_EQUALIZE)
    check_chain(chain)
    ref = apply_chain(imgs, chain)
    assert np.array_equal(ref[5, 1], imgs[5, 1])
    assert np.array_equal(apply_chain(imgs[6:7], chain[6:7, :2])[0, 2], imgs[6, 2])  # the step == 0 equalize
    assert (ref != imgs).reshape(B, -1).any(1).sum() >= B // 2  # the chains do something (f = 1 and such do not)
    return imgs, chain, ref


def _run(imgs, chain):
    from jumbo_mae_tpu_amd.ops import _ext
    x = torch.from_numpy(imgs).cuda()
    out = _ext.load(True).aug_chain(x, torch.from_numpy(chain).cuda(), torch.empty_like(x))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("S", [64, 70, 96])
def test_aug_chain_equals_mirror_per_kind(S):
    imgs, chain, ref = _case(S)
    got = _run(imgs, chain)
    bad = [(b, chain[b, :, 0].astype(int).tolist(), chain[b, :, 8].astype(int).tolist())
           for b in range(B) if not np.array_equal(got[b], ref[b])]
    assert not bad, bad


def test_aug_chain_single_slot_and_unknown_kind_is_a_copy():
    """An odd slot count ends in the scratch buffer; a kind the device does not know (the host
    rejects those in collate) is an identity copy."""
    imgs, chain, _ = _case(64)
    from jumbo_mae_tpu_amd.data.augment_ref import apply_chain
    one = np.ascontiguousarray(chain[:, 1:2])
    assert np.array_equal(_run(imgs, one), apply_chain(imgs, one))
    bad = one.copy()
    bad[:, 0, 0] = [99.0, -3.0, 2.5, float("nan")] * (B // 4)
    assert np.array_equal(_run(imgs, bad), imgs)


def test_aug_chain_two_runs_bit_identical():
    imgs, chain, _ = _case(96)
    assert np.array_equal(_run(imgs, chain), _run(imgs, chain))


def _args(spec, batch=16):
    from types import SimpleNamespace
    return SimpleNamespace(random_crop="rrc", image_size=96, auto_augment="rand-m9-mstd0.5-inc1", color_jitter=0.0,
                           random_erasing=0.0, test_crop_ratio=0.875, train_dataset_shards=spec,
                           valid_dataset_shards=None, mode="pretrain", train_batch_size=batch, grad_accum=1,
                           augment_repeats=1, shuffle_seed=1, train_loader_workers=2, valid_batch_size=batch,
                           valid_loader_workers=0)


def test_randaugment_matches_pil_through_the_loader(tmp_path):
    from jumbo_mae_tpu_amd.data.jpeg_shards import write_shards
    from jumbo_mae_tpu_amd.data.loader import create_dataloaders
    from jumbo_mae_tpu_amd.train.common import DevicePrefetcher
    spec = write_shards(str(tmp_path), shards=2, per_shard=24, classes=5, seed=9)
    cpu, _ = create_dataloaders(_args(spec))
    dev, _ = create_dataloaders(_args(spec), device_augment=True)
    pf = DevicePrefetcher(dev, torch.device("cuda"))
    n = 0
    for a, b in zip(cpu, pf):
        torch.cuda.synchronize()
        assert b.is_cuda and b.dtype == torch.uint8 and b.shape == a.shape
        assert torch.equal(b.cpu(), a), (b.cpu().int() - a.int()).abs().max()
        n += 1
        if n == 3:
            break
    assert n == 3


SCRIPT = textwrap.dedent("""
    import random
    import numpy as np
    import torch
    from PIL import Image
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.__name__.endswith("_C_debug") and ext.debug_build
    from jumbo_mae_tpu_amd.data.loader import DeviceTrainParams, collate_packed, unpack_on_device
    from jumbo_mae_tpu_amd.data.resample_ref import unpack_packed
    from jumbo_mae_tpu_amd.data.transforms import ColorJitter, auto_augment_factory
    t = DeviceTrainParams(70, auto_augment_factory("rand-m9-n3-mstd0.5-inc1", 70), ColorJitter(0.4, 0.4, 0.4))
    rs = np.random.default_rng(0)
    items = []
    for k in range(32):
        random.seed(k)
        items.append(t(Image.fromarray(rs.integers(0, 256, (90, 120, 3), dtype=np.uint8))))
    p = collate_packed(items, size=70)
    assert len(set(p.chain[:, :, 0].flatten().tolist())) >= 10
    out = unpack_on_device(p, torch.device("cuda"))
    torch.cuda.synchronize()
    _ext.debug_check()
    assert np.array_equal(out.cpu().numpy(), unpack_packed(p))
    print("DEBUG_CHAIN_OK")
""")


def test_debug_build_checks_clean_on_a_chain_batch():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0 and "DEBUG_CHAIN_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
