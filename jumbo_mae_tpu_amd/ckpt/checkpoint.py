"""Checkpoint IO: async params writer, resume sidecar, pretrained-param loading.

Reference:
  save_checkpoint_in_background ... /root/reference/src/utils.py:55-63 (a bare thread per save,
                                    writing ``{output_dir}/{name}-{postfix}.msgpack`` via gopen:
                                    local, gs://, s3://, pipe: -- utils/gopen.py here)
  load_pretrained_params .......... /root/reference/src/utils.py:150-202
  save sites ...................... main_pretrain.py:77-90 (``last`` every eval, ``best`` on
                                    improvement)
Changes by design:
  * ONE writer thread with a FIFO queue and write-to-temp + atomic rename: two saves of the same
    file can no longer interleave, and a crash never leaves a torn checkpoint.
  * a ``{name}-{postfix}.state.pt`` sidecar with optimizer moments, step, RNG streams,
    BatchNorm running stats and data position enables ``--resume`` (the reference has none).
  * ``load_pretrained_params`` implements the intended behaviour (quirk Q6): it loads the
    pretrained ``model/*`` encoder subtree into the freshly initialised finetune tree, keeps the
    new head, and can resize a learnable position table.
"""

from __future__ import annotations

import queue
import threading

import numpy as np

from ..utils import gopen
from .msgpack_flax import msgpack_restore, msgpack_serialize


# ------------------------------------------------------------------------------ gopen
# local paths, file://, pipe:<cmd>, gs://, s3://, http(s):// (read) -- utils/gopen.py
read_bytes = gopen.read_bytes
write_bytes = gopen.write_bytes


# ------------------------------------------------------------------------------ writer
class AsyncCheckpointWriter:
    """Single background writer thread; ``submit`` returns immediately."""

    def __init__(self):
        self.q: queue.Queue = queue.Queue()
        self.errors: list[BaseException] = []
        self.t = threading.Thread(target=self._run, name="ckpt-writer", daemon=True)
        self.t.start()

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                self.q.task_done()
                return
            url, payload = item
            try:
                data = payload() if callable(payload) else payload
                write_bytes(url, data)
            except BaseException as e:  # pragma: no cover - surfaced by flush()
                self.errors.append(e)
            finally:
                self.q.task_done()

    def submit(self, url: str, payload) -> None:
        self.q.put((url, payload))

    def flush(self) -> None:
        self.q.join()
        if self.errors:
            raise self.errors.pop(0)

    def close(self) -> None:
        self.flush()
        self.q.put(None)
        self.t.join(timeout=60)


_WRITER: AsyncCheckpointWriter | None = None


def writer() -> AsyncCheckpointWriter:
    global _WRITER
    if _WRITER is None:
        _WRITER = AsyncCheckpointWriter()
    return _WRITER


def ckpt_path(output_dir: str, name: str, postfix: str, ext: str = "msgpack") -> str:
    return gopen.join(output_dir, f"{name}-{postfix}.{ext}")


def save_checkpoint_in_background(output_dir: str, name: str, params_bytes: bytes, postfix: str = "last") -> str:
    url = ckpt_path(output_dir, name, postfix)
    writer().submit(url, params_bytes)
    return url


def save_params(output_dir: str, name: str, tree: dict, postfix: str = "last") -> str:
    return save_checkpoint_in_background(output_dir, name, msgpack_serialize(tree), postfix)


def load_params(url: str) -> dict:
    return msgpack_restore(read_bytes(url))


# ------------------------------------------------------------------------------ resume
def save_resume_state(path: str, state: dict) -> None:
    import io

    import torch

    buf = io.BytesIO()
    torch.save(state, buf)
    writer().submit(path, buf.getvalue())


def load_resume_state(path: str) -> dict:
    import io

    import torch

    return torch.load(io.BytesIO(read_bytes(path)), map_location="cpu", weights_only=True)


# ------------------------------------------------------------------------------ pretrained
def _resize_posemb(arr: np.ndarray, shape) -> np.ndarray:
    """Bicubic resize of a (g, g, D) learnable table to ``shape`` (finetune at a new resolution)."""
    import torch
    import torch.nn.functional as F

    t = torch.from_numpy(np.asarray(arr, dtype=np.float32)).permute(2, 0, 1)[None]
    t = F.interpolate(t, size=tuple(shape[:2]), mode="bicubic", align_corners=False)
    return t[0].permute(1, 2, 0).numpy()


POSEMB_MISMATCH = ("the checkpoint and the model were built with different position embeddings: pass the --posemb "
                   "(and, for rope, the --rope-theta) the checkpoint was trained with")


def _posemb_kind(model_tree: dict):
    """("rope", theta) | ("learnable", None) | ("none", None) of a ``model`` subtree: a rope model's tree has the
    frozen marker ``embed/rope_theta`` and no ``embed/wpe``; a sincos2d tree has neither."""
    embed = model_tree.get("embed", {})
    if "rope_theta" in embed:
        return "rope", float(np.asarray(embed["rope_theta"]).reshape(-1)[0])
    return ("learnable" if "wpe" in embed else "none"), None


def check_posemb(src: dict, dst: dict) -> None:
    """Loading the ``model`` subtree ``src`` into a model whose fresh tree is ``dst``: a rotary model takes
    only a rotary checkpoint of the same theta, and a rotary checkpoint goes only into a rotary model.
    (A table-free sincos2d checkpoint into a learnable model stays allowed: the table keeps its init.)"""
    (sk, st), (dk, dt) = _posemb_kind(src), _posemb_kind(dst)
    if (sk == "rope") != (dk == "rope") or (sk == "rope" and abs(st - dt) > 1e-6 * abs(dt)):
        def name(k, t):
            return f"--posemb rope --rope-theta {t:g}" if k == "rope" else \
                ("--posemb learnable" if k == "learnable" else "a table-free --posemb (sincos2d)")
        raise ValueError(f"checkpoint of {name(sk, st)} into a model of {name(dk, dt)}: {POSEMB_MISMATCH}")


QKNORM_MISMATCH = ("the checkpoint and the model differ in QK-norm: pass the --qk-norm (and, for a pretrain model, the "
                   "--dec-qk-norm) the checkpoint was trained with")


def qknorm_leaves(tree: dict, path: tuple = ()) -> set:
    """The paths of the QK-norm scales (``.../attn/q_norm/scale``, ``.../attn/k_norm/scale``) in a params tree."""
    out = set()
    for k, v in tree.items():
        if isinstance(v, dict):
            out |= qknorm_leaves(v, path + (k,))
        elif k == "scale" and path[-1:] in (("q_norm",), ("k_norm",)):
            out.add(path + (k,))
    return out


def check_qknorm(src: dict, dst: dict) -> None:
    """Loading the tree ``src`` into a model whose fresh tree is ``dst`` (same root): both hold QK-norm scales
    in the same attention layers, or neither does.  A model with QK-norm never takes a checkpoint without it
    with scales left at ones -- the weights were trained against un-normalised logits -- and the other way round
    the scales would be dropped silently."""
    # (a finetune model holds no decoder: only the attention layers present on both sides are compared)
    s = {p for p in qknorm_leaves(src) if _has_path(dst, p[:-2])}
    d = {p for p in qknorm_leaves(dst) if _has_path(src, p[:-2])}
    if s != d:
        diff = sorted("/".join(p) for p in s ^ d)
        side = "the checkpoint" if s - d else "the model"
        raise ValueError(f"only {side} has the QK-norm scale {diff[0]} ({len(diff)} such leaves): {QKNORM_MISMATCH}")


FFN_MISMATCH = ("the checkpoint and the model differ in the feed-forward kind: pass the --ffn (and, for a pretrain "
                "model, the --dec-ffn; for a distillation teacher, the --teacher-ffn) the checkpoint was trained with")


def ffn_nodes(tree: dict, path: tuple = ()) -> dict:
    """{path of a feed-forward node: it is gated} of a params tree: the nodes ``.../ff`` and ``.../jumbo_mlp``
    (they hold ``w1`` and ``w2``); gated = the node has the SwiGLU up projection ``w3``."""
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            if k in ("ff", "jumbo_mlp") and "w1" in v and "w2" in v:
                out[path + (k,)] = "w3" in v
            else:
                out.update(ffn_nodes(v, path + (k,)))
    return out


def check_ffn(src: dict, dst: dict) -> None:
    """Loading the tree ``src`` into a model whose fresh tree is ``dst`` (same root): every feed-forward present
    on both sides is of the same kind.  Checked before any leaf is compared, so that a GELU checkpoint in a
    SwiGLU model (or the reverse) fails naming the flag and the ``w3`` leaves, not with the shape mismatch of
    ``w1/kernel`` (4 dim against the gated width)."""
    s, d = ffn_nodes(src), ffn_nodes(dst)
    missing = sorted("/".join(p + ("w3",)) for p in d if d[p] and p in s and not s[p])
    extra = sorted("/".join(p + ("w3",)) for p in s if s[p] and p in d and not d[p])
    if missing:
        raise ValueError(f"the model (swiglu) holds {missing[0]} ({len(missing)} such feed-forwards) and the checkpoint "
                         f"(gelu) does not: {FFN_MISMATCH}")
    if extra:
        raise ValueError(f"the checkpoint (swiglu) holds {extra[0]} ({len(extra)} such feed-forwards) and the model "
                         f"(gelu) does not: {FFN_MISMATCH}")


def _has_path(tree: dict, path: tuple) -> bool:
    for k in path:
        if not (isinstance(tree, dict) and k in tree):
            return False
        tree = tree[k]
    return True


def load_pretrained_params(url: str, params: dict, log=print) -> dict:
    """Merge the ``model`` subtree of a pretrained checkpoint into ``params`` (a Flax tree).

    Leaves that exist in both with equal shapes are taken from the checkpoint; the new head and
    any other leaf missing from the checkpoint keep their fresh initialisation; a learnable
    ``embed/wpe`` of a different grid is resized bicubically.
    """
    new = load_params(url)
    src = new.get("model", new)
    dst = params["model"]
    check_posemb(src, dst)
    check_qknorm(src, dst)
    check_ffn(src, dst)
    overlap = len(set(src).intersection(dst))
    log(f"[*] load pretrained params with overlap of {overlap}/{len(dst)}")

    loaded = [0]

    def merge(d, s, path=()):
        for k, v in d.items():
            if k not in s:
                continue
            if isinstance(v, dict):
                if isinstance(s[k], dict):
                    merge(v, s[k], path + (k,))
                continue
            sv = np.asarray(s[k])
            if sv.shape == np.shape(v):
                d[k] = sv.astype(np.float32)
                loaded[0] += 1
            elif path[-1:] == ("embed",) and k == "wpe" and sv.ndim == 3:
                d[k] = _resize_posemb(sv, np.shape(v))
                loaded[0] += 1
                log(f"[*] resized embed/wpe {sv.shape} -> {np.shape(v)}")
            else:
                log(f"[!] shape mismatch for {'/'.join(path + (k,))}: {sv.shape} vs {np.shape(v)} (kept init)")

    if "head" in dst:
        head = dst["head"]
        merge(dst, {k: v for k, v in src.items() if k != "head"})
        dst["head"] = head
    else:
        merge(dst, src)
    log(f"[*] {loaded[0]} pretrained leaves loaded")
    return params
