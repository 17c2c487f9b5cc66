"""Training / validation data loaders.

Reference ``create_dataloaders`` (/root/reference/src/dataset.py:100-161) with helpers
``repeat_samples`` / ``collate_and_shuffle`` / ``collate_and_pad`` (:85-97).
* train: infinite cycle over deterministically shuffled shards, split by rank then by worker,
  sample shuffle buffer, decode, repeated augmentation (``augment_repeats`` deep copies, and the
  collate re-orders the batch as batch[0::r] + batch[1::r] + ... so the copies of one image land
  far apart), per-rank batch = train_batch_size // world_size // grad_accum, drop_last.
* valid: one pass, rank split, last batch padded with ``-1`` (uint8 images become 255, labels -1).
* ``synthetic:N[:C]`` shard spec: N random images with C classes (plumbing tests / benchmarks;
  no dataset is reachable offline).
* Device augment (``--device-augment``, on by default on a GPU when the train transform is the
  pretraining one -- RandomResizedCrop + flip, nothing else): the workers decode, draw the crop /
  flip parameters from the same per-sample RNG as the PIL path and ship only the crop window plus
  a descriptor (``DeviceRRCParams``, packed per batch by ``collate_packed``); the resize and flip
  run on the GPU (csrc/augment.hip), bit-exact to PIL's bicubic, when ``DevicePrefetcher`` lands
  the batch.  A worker then spends its time on the JPEG decode only (profiles/r5_data_rate.txt).
  ``--device-augment on`` also covers the finetune transform -- RandAugment / AutoAugment and
  ColorJitter after the crop (``DeviceTrainParams``): the worker makes their draws too and ships a
  chain of op records per image, which csrc/augment_chain.hip applies after the resize, bit-exact
  to PIL (data/augment_ref.py is the NumPy mirror).  ``--device-augment all`` adds AugMix (its
  ``width`` chains run as one op chain over the replicated batch and are composited by
  ``augmix_mix``) and random erasing (the worker draws the box and the noise bytes and ships them;
  ``erase_paste`` writes them into the final batch).  The ``src`` / ``none`` crops stay on the host.
* Device validation (``create_dataloaders(device_valid=True)``; the drivers: ``--device-augment
  auto|on|all`` on a GPU, ``train/common.py use_device_valid``): the validation transform Resize ->
  CenterCrop is an S x S window of a larger resize, which the same kernels compute from an
  18-column descriptor (``DeviceValidParams``); ``collate_valid_packed`` pads the last batch with
  fill entries that the kernel writes as 255 (labels -1), like ``collate_and_pad``.  Bit-exact to
  PIL; only offered while ``int(size / test_crop_ratio) >= size`` (``device_valid_ok``).
Per-rank split replaces the reference's per-host split (one process per GPU here).
"""

from __future__ import annotations

import copy
import itertools
import math
import random
from functools import partial
from typing import NamedTuple

import numpy as np
import torch
from torch.utils.data import DataLoader, IterableDataset, get_worker_info

from . import shards as S
from .transforms import RandomResizedCrop, create_transforms

RRC_TAB = 13  # csrc/augment.hip descriptor width
WIN_TAB = 18  # ... of the window resize (validation): + full output rows / cols, window origin, pad flag
RRC_KMAX = 24  # csrc/augment.hip taps per output pixel


class PackedImages(NamedTuple):
    """A batch for the device augment: concatenated HWC uint8 crop windows + [B, 13] descriptors
    (csrc/augment.hip; [B, 18] for a validation batch, whose pad rows have no window), the scratch
    size of the horizontal pass and the output size; ``chain``:
    float64 [B, slots, AUG_P] op records applied after the resize (csrc/augment_chain.hip), or None.
    AugMix: ``mix`` float32 [B, W + 1] mixing values and the static ``mix_wdb`` = (W chains, D slots
    each, blended); the first W * D slots of ``chain`` are the chains, the rest runs on the mixed
    image.  Random erasing: ``erase`` int64 [B, 5] = box i, j, eh, ew (eh 0: not erased) and the
    offset of the box's [3, eh, ew] bytes in ``fill``, one flat uint8 buffer."""
    src: torch.Tensor
    tab: torch.Tensor
    tmp_bytes: int
    rows_max: int
    size: int
    chain: torch.Tensor | None = None
    mix: torch.Tensor | None = None
    mix_wdb: tuple | None = None
    erase: torch.Tensor | None = None
    fill: torch.Tensor | None = None


def _span(n: int, a: int, c: int, out: int) -> tuple[int, int]:
    """Input index range a superset of what Pillow's bicubic resample of [a, a + c) -> ``out`` reads."""
    support = 2.0 * max(c / out, 1.0)
    return max(0, math.floor(a - support) - 1), min(n, math.ceil(a + c + support) + 1)


def _taps(c: int, out: int) -> int:
    return math.ceil(2.0 * max(c / out, 1.0)) * 2 + 1  # Pillow's ksize


class DeviceRRCParams:
    """Worker side of the device augment, in place of RandomResizedCrop(scale 0.2-1, bicubic) +
    RandomHorizontalFlip + PILToArray: the same RNG draws in the same order; returns the crop
    window (HWC uint8) and its descriptor.  A crop too large for the kernel's tap budget is resized
    here with PIL and shipped as an identity window."""

    def __init__(self, size: int):
        self.size = size
        self.rrc = RandomResizedCrop(size, scale=(0.2, 1.0))

    def __call__(self, img):
        from PIL import Image
        if img.mode != "RGB":
            img = img.convert("RGB")
        W, H = img.size
        i, j, ch, cw = self.rrc.get_params(W, H)
        flip = int(random.random() < 0.5)
        S = self.size
        if max(_taps(ch, S), _taps(cw, S)) > RRC_KMAX:
            arr = np.asarray(img.resize((S, S), Image.BICUBIC, box=(j, i, j + cw, i + ch)))
            H = W = S
            i = j = 0
            ch = cw = S
        else:
            arr = np.asarray(img)
        y0, y1 = _span(H, i, ch, S)
        x0, x1 = _span(W, j, cw, S)
        win = np.ascontiguousarray(arr[y0:y1, x0:x1])
        return win, np.array([0, y1 - y0, x1 - x0, y0, x0, H, W, i, j, ch, cw, flip, 0], dtype=np.int64)


class DeviceTrainParams(DeviceRRCParams):
    """Worker side of the device augment for the finetune transform: ``DeviceRRCParams``, then the
    draws of RandAugment / AutoAugment / AugMix (``aa``), ColorJitter (``cj``) and RandomErasing
    (``erase``) in the PIL path's order.  Returns (window, descriptor, chain): chain = float64
    [slots, AUG_P] op records (data/autoaugment.py), identity-padded to the transform's fixed slot
    count.  With AugMix or erasing the item is (window, descriptor, chain, mix, box, fill): mix =
    (float32 [W + 1] mixing values, (W, D, blended)) or None -- the chain then starts with the W
    chains of D slots each; box int64 [4] and fill uint8 [3, eh, ew] (``RandomErasing.describe``)
    or None."""

    def __init__(self, size: int, aa=None, cj=None, erase=None):
        from .autoaugment import AugMix
        super().__init__(size)
        self.stages = [t for t in (aa, cj) if t is not None]
        self.slots = sum(t.slots for t in self.stages)
        self.mix_wdb = (aa.width, aa.chain_slots, int(aa.blended)) if isinstance(aa, AugMix) else None
        if self.mix_wdb is not None and not 1 <= aa.width <= 8:
            raise ValueError(f"device augment: AugMix with {aa.width} chains (the mix kernel takes 1 .. 8)")
        self.erase = erase

    def __call__(self, img):
        from .autoaugment import op_record
        win, desc = super().__call__(img)
        recs, mix = [], None
        for t in self.stages:
            d = t.describe(self.size)
            if self.mix_wdb is not None and t is self.stages[0]:
                d, mix = d[0], (d[1], self.mix_wdb)
            recs += d
        recs += [op_record()] * (self.slots - len(recs))
        chain = np.stack(recs) if recs else np.zeros((0, len(op_record())), np.float64)
        if mix is None and self.erase is None:
            return win, desc, chain
        box, fill = self.erase.describe(self.size) if self.erase is not None else (None, None)
        return win, desc, chain, mix, box, fill


def device_valid_ok(args) -> bool:
    """The device path covers the validation transform: the centre crop lies inside the resized
    image (a crop that reaches outside it, which PIL pads with black, stays on the host)."""
    return int(args.image_size / args.test_crop_ratio) >= args.image_size


class DeviceValidParams:
    """Worker side of the device validation transform, in place of Resize(int(size / ratio),
    bicubic) + CenterCrop(size) + PILToArray (no random draws): ``Resize``'s output size and
    ``CenterCrop``'s origin, the window of source pixels that the two passes read for that S x S
    window of the full resize, and its 18-column descriptor (csrc/augment.hip).  An image too large
    for the kernel's tap budget is resized here with PIL and shipped as an identity window."""

    def __init__(self, size: int, test_crop_ratio: float = 0.875):
        self.size = size
        self.resize = int(size / test_crop_ratio)
        if self.resize < size:
            raise ValueError(f"device validation transform: Resize({self.resize}) is smaller than the crop ({size})")

    def __call__(self, img):
        from PIL import Image

        from .resample_ref import read_range
        if img.mode != "RGB":
            img = img.convert("RGB")
        W, H = img.size
        S, R = self.size, self.resize
        if W <= H:  # transforms.Resize
            nw, nh = R, int(R * H / W)
        else:
            nh, nw = R, int(R * W / H)
        i0 = int(round((nh - S) / 2.0))  # transforms.CenterCrop
        j0 = int(round((nw - S) / 2.0))
        if max(_taps(H, nh), _taps(W, nw)) > RRC_KMAX:
            arr = np.asarray(img.resize((nw, nh), Image.BICUBIC))
            H, W = nh, nw
        else:
            arr = np.asarray(img)
        y0, y1 = read_range(H, 0, H, nh, i0, S)
        x0, x1 = read_range(W, 0, W, nw, j0, S)
        win = np.ascontiguousarray(arr[y0:y1, x0:x1])
        return win, np.array([0, y1 - y0, x1 - x0, y0, x0, H, W, 0, 0, H, W, 0, 0, nh, nw, i0, j0, 0], dtype=np.int64)


def collate_valid_packed(batch, batch_size: int = 1, size: int = 224):
    """Device-validation collate, ``collate_and_pad`` for ``DeviceValidParams`` items ((window,
    descriptor), label): windows concatenated with their offsets written into the descriptors, then
    pad entries (no window, fill flag: the kernel writes 255) and labels -1 up to ``batch_size``.
    Returns (PackedImages, labels)."""
    descs = [np.asarray(d) for (_, d), _ in batch]
    for d in descs:
        if d.shape != (WIN_TAB,) or d.dtype != np.int64:
            raise ValueError(f"validation descriptor must be int64 [{WIN_TAB}], got {d.dtype} {d.shape}")
    wins = [np.asarray(w) for (w, _), _ in batch]
    for w, d in zip(wins, descs):
        if w.dtype != np.uint8 or w.size != d[1] * d[2] * 3:
            raise ValueError(f"validation window must be uint8 [{d[1]}, {d[2]}, 3], got {w.dtype} {w.shape}")
    pad = np.zeros(WIN_TAB, np.int64)
    pad[17] = 1
    tab = np.stack(descs + [pad] * (batch_size - len(batch)))
    sizes = np.array([w.size for w in wins] + [0] * (batch_size - len(batch)), dtype=np.int64)
    tab[:, 0] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rows = tab[:, 1]
    tab[:, 12] = np.concatenate([[0], np.cumsum(rows * size * 3)[:-1]])
    src = torch.from_numpy(np.concatenate([w.reshape(-1) for w in wins]))
    labels = torch.tensor([lb for _, lb in batch] + [-1] * (batch_size - len(batch)))
    return PackedImages(src, torch.from_numpy(tab), int((rows * size * 3).sum()), int(rows.max()), size), labels


def check_chain(chain: np.ndarray) -> np.ndarray:
    """Host-side validation of a [B, slots, AUG_P] record table: known kinds and resample modes only."""
    from .autoaugment import AUG_KINDS, AUG_P, K_AFFINE
    if chain.ndim != 3 or chain.shape[2] != AUG_P or chain.dtype != np.float64:
        raise ValueError(f"op chain must be float64 [B, slots, {AUG_P}], got {chain.dtype} {chain.shape}")
    kinds = chain[:, :, 0]
    if not np.all((kinds == np.floor(kinds)) & (kinds >= 0) & (kinds < AUG_KINDS)):
        raise ValueError(f"op chain: unknown kind(s) {sorted(set(kinds[(kinds != np.floor(kinds)) | (kinds < 0) | (kinds >= AUG_KINDS)].tolist()))}")
    rs = chain[:, :, 8][kinds == K_AFFINE]
    if not np.all((rs == 2) | (rs == 3)):
        raise ValueError("op chain: an affine op needs resample 2 (bilinear) or 3 (bicubic)")
    return chain


def check_mix(mix: np.ndarray, wdb, slots: int) -> np.ndarray:
    """Host-side validation of an AugMix mix table against its static (W, D, blended): float32
    [B, W + 1], finite, 1 <= W <= 8, and W * D chain slots in the batch's op chain."""
    W, D, _ = wdb
    if not (1 <= W <= 8 and D >= 1 and W * D <= slots):
        raise ValueError(f"AugMix mix: {W} chains of {D} slots do not fit the device path (1..8 chains, {slots} slots)")
    if mix.ndim != 2 or mix.shape[1] != W + 1 or mix.dtype != np.float32:
        raise ValueError(f"AugMix mix table must be float32 [B, {W + 1}], got {mix.dtype} {mix.shape}")
    if not np.isfinite(mix).all():
        raise ValueError("AugMix mix table: non-finite value(s)")
    return mix


def check_erase(erase: np.ndarray, fill_len: int, size: int) -> np.ndarray:
    """Host-side validation of an erase table: int64 [B, 5]; a row is all zero up to the offset (not
    erased) or a box of 1 .. size - 1 rows and columns inside the image whose 3 * eh * ew bytes lie
    inside the fill buffer."""
    if erase.ndim != 2 or erase.shape[1] != 5 or erase.dtype != np.int64:
        raise ValueError(f"erase table must be int64 [B, 5], got {erase.dtype} {erase.shape}")
    i, j, eh, ew, off = erase.T
    on = eh != 0
    if ((eh < 0) | (~on & (ew != 0))).any():
        raise ValueError("erase table: a box with negative or half-empty extent")
    if (on & ((eh >= size) | (ew >= size) | (ew <= 0))).any():
        raise ValueError(f"erase table: a box needs 1 .. {size - 1} rows and columns")
    if (on & ((i < 0) | (j < 0) | (i + eh > size) | (j + ew > size))).any():
        raise ValueError(f"erase table: a box leaves the image [0, {size})")
    if (on & ((off < 0) | (off + 3 * eh * ew > fill_len))).any():
        raise ValueError(f"erase table: fill bytes outside the fill buffer of {fill_len}")
    return erase


def _collate_mix_erase(items, slots: int, size: int):
    """The AugMix and erasing fields of ``PackedImages`` from the (mix, box, fill) tails of the items."""
    mix = wdb = erase = fill = None
    if items[0][0] is not None:
        wdb = tuple(int(v) for v in items[0][0][1])
        if any(tuple(m[1]) != wdb for m, _, _ in items):
            raise ValueError("AugMix mix: the items of a batch disagree on (chains, slots, blended)")
        rows = [np.asarray(m[0]) for m, _, _ in items]
        if any(r.shape != rows[0].shape or r.dtype != rows[0].dtype for r in rows):
            raise ValueError(f"AugMix mix table must be float32 [B, {wdb[0] + 1}]: rows of different shape or dtype")
        mix = torch.from_numpy(check_mix(np.stack(rows), wdb, slots))
    if items[0][1] is not None:
        boxes = [np.asarray(b) for _, b, _ in items]
        fills = [np.asarray(f) for _, _, f in items]
        for b, f in zip(boxes, fills):
            if b.shape != (4,) or b.dtype != np.int64:
                raise ValueError(f"erase box must be int64 [4], got {b.dtype} {b.shape}")
            if f.dtype != np.uint8 or f.size != 3 * max(int(b[2]), 0) * max(int(b[3]), 0):
                raise ValueError(f"erase fill must be uint8 [3, {b[2]}, {b[3]}], got {f.dtype} {f.shape}")
        sizes = np.array([f.size for f in fills], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]) * (sizes > 0)
        tab = np.concatenate([np.stack(boxes), offs[:, None]], axis=1)
        erase = torch.from_numpy(check_erase(tab, int(sizes.sum()), size))
        fill = torch.from_numpy(np.concatenate([f.reshape(-1) for f in fills]))
    return mix, wdb, erase, fill


def collate_packed(batch, repeats: int = 1, size: int = 224):
    """Device-augment collate: the repeat re-ordering of ``collate_and_shuffle``, then windows
    concatenated into one flat buffer with offsets written into the descriptors; op chains
    (``DeviceTrainParams``) stacked into one validated [B, slots, AUG_P] table, AugMix mixing values
    into a [B, W + 1] table and erase boxes into a [B, 5] table over one flat fill buffer."""
    batch = sum([batch[i::repeats] for i in range(repeats)], [])
    labels = None
    if isinstance(batch[0][0], tuple):  # ((win, desc[, chain[, mix, box, fill]]), label)
        labels = torch.tensor([b[1] for b in batch])
        batch = [b[0] for b in batch]
    chain = None
    extra = (None, None, None, None)
    if len(batch[0]) >= 3:
        chain = torch.from_numpy(check_chain(np.stack([b[2] for b in batch])))
        if len(batch[0]) == 6:
            extra = _collate_mix_erase([b[3:] for b in batch], chain.shape[1], size)
        batch = [b[:2] for b in batch]
    tab = np.stack([d for _, d in batch])
    sizes = np.array([w.size for w, _ in batch], dtype=np.int64)
    tab[:, 0] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rows = tab[:, 1]
    tab[:, 12] = np.concatenate([[0], np.cumsum(rows * size * 3)[:-1]])
    src = torch.from_numpy(np.concatenate([w.reshape(-1) for w, _ in batch]))
    packed = PackedImages(src, torch.from_numpy(tab), int((rows * size * 3).sum()), int(rows.max()), size, chain,
                          *extra)
    return packed if labels is None else (packed, labels)


def unpack_on_device(p: PackedImages, device) -> torch.Tensor:
    """uint8 [B, 3, S, S] from a packed batch: H2D of the windows, then the resize / flip kernels
    (by the table's width: the random-resized-crop or the validation window resize) and, for a
    batch with an op chain, the chain kernels; for an AugMix batch the W chains on W replicas of
    the resized batch, their composite, then the rest of the chain (ColorJitter); last the erase
    boxes, in place -- all on the current stream."""
    from ..ops import _ext
    ext = _ext.load(True)
    src = p.src.to(device, non_blocking=True)
    tab = p.tab.to(device, non_blocking=True)
    resize = ext.window_resize if p.tab.shape[1] == WIN_TAB else ext.rrc_resize
    out = resize(src, tab, p.size, p.tmp_bytes, p.rows_max)
    chain = p.chain.to(device, non_blocking=True) if p.chain is not None and p.chain.shape[1] > 0 else None
    if p.mix is not None:
        W, D, blended = p.mix_wdb
        B = out.shape[0]
        rep = out.unsqueeze(1).repeat(1, W, 1, 1, 1).view(B * W, *out.shape[1:])  # always a copy: aug_chain consumes it
        recs = chain[:, :W * D].reshape(B * W, D, chain.shape[2])
        rep = ext.aug_chain(rep, recs, torch.empty_like(rep))
        orig, out = out, ext.augmix_mix(out, rep, p.mix.to(device, non_blocking=True), bool(blended))
        if chain.shape[1] > W * D:
            out = ext.aug_chain(out, chain[:, W * D:].contiguous(), orig)  # the original is the free buffer now
    elif chain is not None:
        out = ext.aug_chain(out, chain, torch.empty_like(out))
    if p.erase is not None and p.fill.numel() > 0:
        out = ext.erase_paste(out, p.erase.to(device, non_blocking=True), p.fill.to(device, non_blocking=True),
                              3 * int((p.erase[:, 2] * p.erase[:, 3]).max()))
    return out


def device_augment_rrc_only(args) -> bool:
    """The train transform is RandomResizedCrop + flip only (the pretraining presets)."""
    return (getattr(args, "random_crop", "rrc") == "rrc" and getattr(args, "auto_augment", "none") in ("none", "", None)
            and not getattr(args, "color_jitter", 0.0) and not getattr(args, "random_erasing", 0.0))


def device_augment_ok(args) -> bool:
    """The device augment covers the train transform: RandomResizedCrop + flip, optionally followed
    by RandAugment (``rand-*``) or an AutoAugment policy and ColorJitter.  Not AugMix (parallel
    chains), random erasing (np.random noise) or the ``src`` / ``none`` crops."""
    from .autoaugment import POLICIES
    aa = getattr(args, "auto_augment", "none") or "none"
    return (getattr(args, "random_crop", "rrc") == "rrc" and not getattr(args, "random_erasing", 0.0)
            and (aa == "none" or aa.startswith("rand") or aa.split("-")[0] in POLICIES))


def device_augment_all_ok(args) -> bool:
    """What ``--device-augment all`` covers: ``device_augment_ok`` plus AugMix (``augmix-*``) and
    random erasing.  The ``src`` / ``none`` crops stay on the host."""
    from .autoaugment import POLICIES
    aa = getattr(args, "auto_augment", "none") or "none"
    return (getattr(args, "random_crop", "rrc") == "rrc"
            and (aa == "none" or aa.startswith("rand") or aa.startswith("augmix") or aa.split("-")[0] in POLICIES))


def repeat_samples(samples, repeats: int = 1):
    for s in samples:
        for _ in range(repeats):
            yield copy.deepcopy(s)


def _stack(items):
    first = items[0]
    if isinstance(first, tuple):
        return tuple(_stack([it[i] for it in items]) for i in range(len(first)))
    if isinstance(first, np.ndarray):
        return torch.from_numpy(np.stack(items))
    if isinstance(first, torch.Tensor):
        return torch.stack(items)
    return torch.tensor(items)


def collate_and_shuffle(batch, repeats: int = 1):
    return _stack(sum([batch[i::repeats] for i in range(repeats)], []))


def _minus_one_like(x):
    if isinstance(x, np.ndarray):
        # torch.full_like(uint8, -1) wraps to 255 in the reference; numpy 2 refuses -1 for uint8
        return np.full_like(x, np.iinfo(x.dtype).max if x.dtype.kind == "u" else -1)
    return -1


def collate_and_pad(batch, batch_size: int = 1):
    first = batch[0]
    if isinstance(first, tuple):
        pad = tuple(_minus_one_like(x) for x in first)
    else:
        pad = _minus_one_like(first)
    return _stack(list(batch) + [pad] * (batch_size - len(batch)))


def sample_seed(seed: int, rank: int, wid: int, index: int) -> int:
    """Seed of the augmentation draws of one training sample: sample ``index`` of worker ``wid``'s
    post-repeat stream on ``rank``.  Seeding per sample (not once per worker) makes a sample's
    augmentation independent of how many samples came before it, so a resumed run that skips the
    consumed samples without decoding them reproduces the uninterrupted stream exactly."""
    h = (seed * 1_000_003 + rank * 92_821 + wid * 7_919) & 0xFFFFFFFF
    return (h * 2_654_435_761 + index * 40_503 + 0x9E3779B9) % (2 ** 32)


def worker_skip(batches: int, wid: int, nw: int) -> int:
    """Batches that worker ``wid`` of ``nw`` delivered among the first ``batches`` of a DataLoader
    (the loader takes batches from its workers round-robin)."""
    return (batches - wid + nw - 1) // nw if batches > wid else 0


class ShardDataset(IterableDataset):
    def __init__(self, spec, mode: str, transform, train: bool, repeats: int = 1, seed: int = 0,
                 rank: int = 0, world: int = 1, shuffle_buffer: int = 2000, image_size: int = 224,
                 skip_batches: int = 0, batch_size: int = 1):
        self.spec, self.mode, self.transform, self.train = spec, mode, transform, train
        self.repeats, self.seed, self.rank, self.world = repeats, seed, rank, world
        self.shuffle_buffer = shuffle_buffer
        self.image_size = image_size
        # resume: the first ``skip_batches`` DataLoader batches (of ``batch_size``) were consumed by
        # the interrupted run; each worker skips its share of them without decoding
        self.skip_batches, self.batch_size = skip_batches, batch_size
        # validation batches always carry a label so that padded rows (-1) can be masked out
        self.with_label = mode in ("finetune", "linear") or not train
        self.synthetic = isinstance(spec, str) and spec.startswith("synthetic:")
        self.urls = [] if self.synthetic else S.shard_list(spec)

    # raw (undecoded) records of this rank/worker, one epoch
    def _records(self, epoch: int, wid: int, nw: int):
        if self.synthetic:
            parts = self.spec.split(":")
            n = int(parts[1])
            idx = itertools.islice(range(n), self.rank * nw + wid, None, self.world * nw)
            for i in idx:
                yield {"synthetic": i + (epoch * 7919 if self.train else 0)}
            return
        urls = S.epoch_shards(self.urls, self.seed, epoch, shuffle=self.train)
        total = self.world * nw
        if len(urls) >= total:
            mine = S.split(S.split(urls, self.rank, self.world), wid, nw)
            sample_filter = None
        else:  # fewer shards than consumers: split samples instead of shards
            mine = urls
            sample_filter = (self.rank * nw + wid, total)
        handler = S.ignore_and_continue if self.train else None
        # validation shards are cached locally on the first pass (webdataset cached_tarfile_to_samples)
        it = S.iter_samples(mine, handler) if self.train else S.cached_samples(mine, handler)
        if sample_filter is not None:
            it = itertools.islice(it, sample_filter[0], None, sample_filter[1])
        if self.train:
            it = S.detshuffle(it, self.shuffle_buffer, self.seed * 7 + epoch * 131 + self.rank * 17 + wid)
        yield from it

    def _decode(self, rec):
        """Decoded sample dict of a record, or None (train: a corrupt record is skipped)."""
        if "synthetic" in rec:
            parts = self.spec.split(":")
            ncls = int(parts[2]) if len(parts) > 2 else 1000
            rs = np.random.default_rng(rec["synthetic"])
            arr = rs.integers(0, 256, (self.image_size + 32, self.image_size + 32, 3), dtype=np.uint8)
            from PIL import Image
            return {"jpg": Image.fromarray(arr), "cls": int(rs.integers(0, ncls))}
        try:
            out = {"jpg": S.decode_pil(rec["jpg"])}
            if self.with_label:
                out["cls"] = S.decode_cls(rec["cls"]) if "cls" in rec else 0
            return out
        except Exception:
            if not self.train:
                raise
            return None

    # kept for callers of the one-epoch decoded view
    def _raw(self, epoch: int, wid: int, nw: int):
        for rec in self._records(epoch, wid, nw):
            s = self._decode(rec)
            if s is not None:
                yield s

    def __iter__(self):
        info = get_worker_info()
        wid, nw = (info.id, info.num_workers) if info is not None else (0, 1)
        if self.train:
            # a resumed loader's batch j is batch start + j of the interrupted stream, which worker
            # (start + j) % nw produced: worker w takes over the role of worker (w + start) % nw
            wid = (wid + self.skip_batches) % nw
        random.seed(self.seed * 1000 + self.rank * 97 + wid)
        np.random.seed((self.seed * 1000 + self.rank * 97 + wid) % (2 ** 32))
        if not self.train:
            for s in self._raw(0, wid, nw):
                img = self.transform(s["jpg"])
                yield (img, s["cls"]) if self.with_label else img
            return
        r = max(self.repeats, 1)
        skip = worker_skip(self.skip_batches, wid, nw) * self.batch_size  # post-repeat samples
        index = 0  # position in this worker's post-repeat sample stream
        epoch = 0
        while True:
            for rec in self._records(epoch, wid, nw):
                if skip >= r:  # the whole record (all its repeats) was consumed before the resume
                    skip -= r
                    index += r
                    continue
                s = self._decode(rec)
                if s is None:
                    # a record that fails to decode still takes its r positions, so the per-sample
                    # augmentation seeds of everything after it match a resumed run (whose skip
                    # counts records without decoding them).  Exact resume assumes no corrupt
                    # record BEFORE the resume point: the skip (samples consumed / r records) then
                    # lands one record early per corrupt record and repeats its successor's samples.
                    index += r  # as the decoded path: skip + (r - skip) positions
                    skip = 0
                    continue
                first, skip = skip, 0
                index += first
                for k in range(first, r):
                    # repeated augmentation: deep copies of one decoded sample, own draws each
                    seed = sample_seed(self.seed, self.rank, wid, index)
                    random.seed(seed)
                    np.random.seed(seed)
                    img = self.transform(copy.deepcopy(s["jpg"]) if r > 1 else s["jpg"])
                    index += 1
                    yield (img, s["cls"]) if self.with_label else img
            epoch += 1


def create_dataloaders(args, rank: int = 0, world: int = 1, start_batches: int = 0, device_augment: bool = False,
                       device_valid: bool = False):
    """Returns (train_loader | None, valid_loader | None) like dataset.py:100-161.  ``start_batches``
    (resume): train batches already consumed on this rank -- the stream continues after them.
    ``device_augment``: train batches are ``PackedImages`` for ``unpack_on_device`` (requires
    ``device_augment_all_ok(args)``; AugMix and random erasing ride along when the args ask for them).  ``device_valid``: validation batches are (``PackedImages``,
    labels) too (requires ``device_valid_ok(args)``); ``device_augment`` alone leaves them on PIL."""
    train_t, valid_t = create_transforms(args.random_crop, args.image_size, args.auto_augment, args.color_jitter,
                                         args.random_erasing, args.test_crop_ratio)
    if device_augment:
        assert device_augment_all_ok(args), "device augment: the src / none crops stay on the host"
        if device_augment_rrc_only(args):
            train_t = DeviceRRCParams(args.image_size)
        else:
            from .transforms import ColorJitter, RandomErasing, auto_augment_factory
            cj, re = args.color_jitter, args.random_erasing
            train_t = DeviceTrainParams(args.image_size, auto_augment_factory(args.auto_augment or "none", args.image_size),
                                        ColorJitter(cj, cj, cj) if cj > 0 else None,
                                        RandomErasing(re) if re > 0 else None)
    train_dl = valid_dl = None
    pin = torch.cuda.is_available()
    if getattr(args, "train_dataset_shards", None):
        bs = args.train_batch_size // world // args.grad_accum
        ds = ShardDataset(args.train_dataset_shards, args.mode, train_t, True, args.augment_repeats,
                          args.shuffle_seed, rank, world, image_size=args.image_size,
                          skip_batches=start_batches, batch_size=bs)
        nw = args.train_loader_workers
        collate = (partial(collate_packed, repeats=args.augment_repeats, size=args.image_size) if device_augment
                   else partial(collate_and_shuffle, repeats=args.augment_repeats))
        train_dl = DataLoader(ds, batch_size=bs, num_workers=nw, collate_fn=collate,
                              drop_last=True, pin_memory=pin, prefetch_factor=4 if nw > 0 else None,
                              persistent_workers=nw > 0)
    if getattr(args, "valid_dataset_shards", None):
        if device_valid:
            assert device_valid_ok(args), "device validation: a centre crop larger than the resized image stays on the host"
            valid_t = DeviceValidParams(args.image_size, args.test_crop_ratio)
        ds = ShardDataset(args.valid_dataset_shards, args.mode, valid_t, False, 1, 0, rank, world,
                          image_size=args.image_size)
        bs = args.valid_batch_size // world
        nw = args.valid_loader_workers
        collate = (partial(collate_valid_packed, batch_size=bs, size=args.image_size) if device_valid
                   else partial(collate_and_pad, batch_size=bs))
        valid_dl = DataLoader(ds, batch_size=bs, num_workers=nw, collate_fn=collate,
                              drop_last=False, pin_memory=pin, prefetch_factor=4 if nw > 0 else None,
                              persistent_workers=nw > 0)
    return train_dl, valid_dl


class SyntheticGPUImages:
    """Infinite GPU-resident random uint8 batches (benchmarks: no host decode / H2D in the loop)."""

    def __init__(self, batch: int, image_size: int, device, labels: int = 0, seed: int = 0, pool: int = 2):
        g = torch.Generator(device=device).manual_seed(seed)
        self.imgs = [torch.randint(0, 256, (batch, 3, image_size, image_size), dtype=torch.uint8, device=device,
                                   generator=g) for _ in range(pool)]
        self.labels = [torch.randint(0, max(labels, 1), (batch,), device=device, generator=g) for _ in range(pool)]
        self.with_labels = labels > 0
        self.i = 0

    def __iter__(self):
        return self

    def __next__(self):
        k = self.i % len(self.imgs)
        self.i += 1
        return (self.imgs[k], self.labels[k]) if self.with_labels else self.imgs[k]
