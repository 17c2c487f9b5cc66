"""Cases and digests of tests/test_attention_bits_gpu.py: the whole-sequence attention kernels of
csrc/attention.hip must give the bits recorded in tests/golden/attn_whole_seq_digests.json.

One shape per whole-sequence instantiation (the shapes tests/attn_ref.py uses for that purpose): every SP
bucket at both head dims, both EX values, the partial and the full batch groups of bwd2 and the shared last
key tile of the 4-wave bwd3.  Each shape runs without dropout and with dropout at ``RATE`` and the seed
``SEED``; the backward is called with a dbias tensor.  Inputs come from a CPU generator seeded by the shape,
so they do not depend on the device's random stream; their digests are recorded as well.

The golden file is written from the tree of the commit BEFORE a change to the kernels:
    python tests/attn_bits.py --tree DIR --write FILE
(``DIR``, the root of a built tree, is put first on sys.path).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import sys
import zlib
from pathlib import Path

import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "attn_whole_seq_digests.json"
RATE = 0.2
SEED = 0x5EED_1234_5678
INPUTS = ("qkv", "dO")
OUTPUTS = ("o", "lse", "dqkv", "dbias")

# (B, S, H, hd)
CASES = [(2, S, 3, 32) for S in (17, 33, 64, 72, 128, 160, 197, 209, 224)] + \
        [(9, S, 3, 64) for S in (19, 30, 52, 64)] + \
        [(16, 52, 3, 64)] + \
        [(2, S, 3, 64) for S in (80, 100, 128, 160, 199, 224)]


def case_id(shape) -> str:
    B, S, H, hd = shape
    return f"hd{hd}-S{S}-B{B}-H{H}"


def digest(t: torch.Tensor) -> str:
    """SHA-256 of the tensor's raw bytes."""
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def inputs(shape):
    """(qkv [B, S, 3 H hd], dO [B, S, H hd]) in bf16 on the CPU."""
    B, S, H, hd = shape
    gen = torch.Generator().manual_seed(zlib.crc32(repr(tuple(shape)).encode()))
    qkv = (torch.randn(B, S, 3 * H * hd, generator=gen) * 1.5).bfloat16()
    dO = (torch.randn(B, S, H * hd, generator=gen) * 1.5).bfloat16()
    return qkv, dO


def run_case(ext, shape, drop: bool) -> dict:
    """Forward and backward (with dbias) of one shape on the device; digests of inputs and outputs."""
    B, S, H, hd = shape
    qkv_c, dO_c = inputs(shape)
    qkv, dO = qkv_c.cuda(), dO_c.cuda()
    dbias = torch.zeros(3 * H * hd, device="cuda")
    if drop:
        seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
        o, lse = ext.attn_fwd(qkv, H, seed, RATE)
        dqkv = ext.attn_bwd(dO, qkv, o, lse, H, dbias, seed, RATE)
    else:
        o, lse = ext.attn_fwd(qkv, H)
        dqkv = ext.attn_bwd(dO, qkv, o, lse, H, dbias)
    torch.cuda.synchronize()
    return {"qkv": digest(qkv_c), "dO": digest(dO_c), "o": digest(o), "lse": digest(lse), "dqkv": digest(dqkv),
            "dbias": digest(dbias)}


def run_all(ext) -> dict:
    return {case_id(s): {"nodrop": run_case(ext, s, False), "drop": run_case(ext, s, True)} for s in CASES}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="root of the built tree whose kernels are recorded")
    ap.add_argument("--write", required=True, help="JSON file to write")
    a = ap.parse_args(argv)
    sys.path.insert(0, str(Path(a.tree).resolve()))
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    print("extension:", ext.__file__)
    res = run_all(ext)
    Path(a.write).parent.mkdir(parents=True, exist_ok=True)
    Path(a.write).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(f"wrote {len(res)} cases to {a.write}")


if __name__ == "__main__":
    sys.exit(main())
