"""Structured attention inputs, fp64 references and the shared assertions of the attention kernel tests.

Used by tests/test_attention_structured_gpu.py (the kernels of csrc/attention.hip) and by
tests/test_attn_ref.py, which keeps this module honest without a GPU: the construction conditions of
every shape, a bf16-emulating composition against every bound, and injected faults that the assertions
must catch.

Layout: qkv [B, S, 3, H, hd] flattened to [B, S, 3 H hd], o / dO [B, S, H hd], lse [B, H, S]; everything
in here works on [B, H, S, hd] and ``pack`` / ``unpack_*`` convert.  Every value of qkv and dO is a bf16
number, every (batch, head) draws its own data from one seeded generator.

The cases
  A  selector   k_j = c code_j, q_i = c code_pi(i) with +-1 codes whose pairwise dot products are at most
                ``CODES[hd][1]``: key pi(i) wins row i by more than 150 in the log2 domain, so every other
                probability underflows to zero in fp32 and P is exactly one-hot.  v and dO are small
                integers: o == v[pi], dv[pi(i)] == dO[i], dq == dk == 0, all exact.
  B  uniform    q = 0 (mirror: k = 0): every score is 0, like a zero-filled padded key, P = 1 / S.
                v[j, d] = [d == j mod hd].  lse, o, dv, dq (mirror: dk) per element within bounds built
                from the reference's own terms; the gradient of the zero operand's partner is exactly 0.
  C  negative   q = 2, k = -2: every real score is -4 sqrt(hd), a padded key at score 0 that escapes the
                mask takes all the mass.  Forward only.
  R  random     randn * 1.5 as in test_kernels_gpu.py::test_attention, forward per element.
"""

from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import torch

F64 = torch.float64
BF16 = torch.bfloat16
ULP32 = 2.0 ** -23

# hd -> (c, largest dot product of two different codes).  The winner's score is c^2 sqrt(hd) nats, the
# runner-up's at most c^2 T / sqrt(hd): hd 32 / 64 / 80 / 96 with c = 8 give 362 / 512 / 572 / 627 nats
# (times log2(e) < 1024) and gaps of 181 / 256 / 286 / 313 nats; hd 128 needs c = 4 (c = 8: 724 nats =
# 1045 in the log2 domain) and T = 48 for a gap of 113 nats.  Every gap is past 150 ln 2 = 104 nats, where
# exp2 of the difference is below half the smallest fp32 denormal: exactly zero in any kernel.
CODES = {32: (8, 16), 64: (8, 32), 80: (8, 40), 96: (8, 48), 128: (4, 48)}
MIN_GAP_NATS = 40.0
ZERO_GAP_NATS = 150.0 * math.log(2.0)
INT_MAX = 8  # v, dO, and the non-zero operand of B are integers in [-8, 8]


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode())


def _nan_backed(t):
    """``t`` as the leading contiguous view of a larger buffer whose remaining elements are NaN:
    a read past the last row then lands in allocated memory and poisons the result."""
    n = t.numel()
    buf = torch.full((n + 64 * t.shape[-1] + 4096,), float("nan"), dtype=t.dtype, device=t.device)
    buf[:n] = t.reshape(-1)
    return buf[:n].view(t.shape)


# ------------------------------------------------------------------ the dispatch, as csrc/attention.hip has it
MAX_SEQ = 224
SPS = (32, 64, 128, 224)


def kernels(S: int, hd: int) -> dict:
    """The instantiation a shape reaches: HD, SP, EX, forward kind, backward kind (dispatch_sp, run,
    run_bwd, jm_attn_tiled)."""
    if hd not in (32, 64) or S > MAX_SEQ:
        return dict(HD=hd, SP=None, EX=None, fwd="fwd_long", bwd="bwd_dq+bwd_dkv")
    SP = next(sp for sp in SPS if S <= sp)
    bwd = "bwd3x4" if hd == 32 else ("bwd3x8" if S > 64 else "bwd2")
    return dict(HD=hd, SP=SP, EX=S > SP - 32, fwd="fwd_ml" if SP <= 64 else "fwd", bwd=bwd)


def shape_id(shape) -> str:
    B, S, H, hd = shape
    k = kernels(S, hd)
    sp = "stream" if k["SP"] is None else f"SP{k['SP']}{'ex' if k['EX'] else ''}"
    return f"hd{hd}-S{S}-B{B}-H{H}-{sp}-{k['fwd']}-{k['bwd']}"


def _shapes():
    """(B, S, H, hd, starred): the smallest S per instantiation and the sizes where a path changes."""
    out = []
    star = lambda ss: [(int(str(s).rstrip("*")), str(s).endswith("*")) for s in ss]
    for S, st in star(["17*", 33, "64*", "72*", 97, 128, "160*", "197*", 208, 209, "224*"]):
        out.append((2, S, 3, 32, st))
    # bwd2: 9 batch elements = one full 8-element group plus a group of one; 27 (b, h) pairs leave the
    # last 4-pair forward workgroup partial
    for S, st in star([19, "30*", "52*", 64]):
        out.append((9, S, 3, 64, st))
    out.append((16, 52, 3, 64, False))  # two full bwd2 groups
    for S, st in star(["80*", 100, 128, "160*", "199*", 224]):
        out.append((2, S, 3, 64, st))
    for hd in (32, 64):
        for S, st in star(["225*", 259, 321]):  # 321: five full 64-row tiles plus one row
            out.append((2, S, 3, hd, st))
    for hd in (80, 96, 128):
        for S, st in star([1, "52*", 64, "65*", 259]):
            out.append((2, S, 3, hd, st))
    return out


_ALL = _shapes()
SHAPES = [s[:4] for s in _ALL]
SHAPES_C = [s[:4] for s in _ALL if s[4]]
# one shape per forward instantiation
SHAPES_R = [(2, 17, 3, 32), (2, 64, 3, 32), (2, 72, 3, 32), (2, 128, 3, 32), (2, 160, 3, 32), (2, 197, 3, 32),
            (9, 30, 3, 64), (9, 52, 3, 64), (2, 80, 3, 64), (2, 100, 3, 64), (2, 160, 3, 64), (2, 199, 3, 64),
            (2, 225, 3, 32), (2, 259, 3, 64), (2, 65, 3, 80), (2, 52, 3, 96), (2, 259, 3, 128)]


# ------------------------------------------------------------------ layout
def pack(q, k, v):
    """[B, H, S, hd] x 3 -> bf16 qkv [B, S, 3 H hd]; the values must be bf16 numbers already."""
    B, H, S, hd = q.shape
    x = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * H * hd)
    xb = x.to(BF16)
    assert torch.equal(xb.double(), x.double()), "qkv values must be exactly representable in bf16"
    return xb.contiguous()


def pack_o(x):
    """[B, H, S, hd] -> bf16 [B, S, H hd]."""
    B, H, S, hd = x.shape
    xb = x.permute(0, 2, 1, 3).reshape(B, S, H * hd).to(BF16)
    assert torch.equal(xb.double(), x.permute(0, 2, 1, 3).reshape(B, S, H * hd).double())
    return xb.contiguous()


def unpack_o(o, H):
    B, S, D = o.shape
    return o.view(B, S, H, D // H).permute(0, 2, 1, 3)


def unpack_qkv(x, H):
    """[B, S, 3 H hd] -> (q, k, v) views [B, H, S, hd]."""
    B, S, D3 = x.shape
    return tuple(t.permute(0, 2, 1, 3) for t in x.view(B, S, 3, H, D3 // 3 // H).unbind(2))


# ------------------------------------------------------------------ fp64 reference
@dataclass
class Ref:
    z: torch.Tensor      # scores [B, H, S, S], nats
    p: torch.Tensor      # softmax
    lse: torch.Tensor    # [B, H, S]
    o: torch.Tensor      # [B, H, S, hd]
    dP: torch.Tensor
    delta: torch.Tensor  # [B, H, S, 1]
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor


def reference(q, k, v, dO=None) -> Ref:
    """Attention forward and gradients in float64 from [B, H, S, hd] operands, no rounding anywhere."""
    q, k, v = q.double(), k.double(), v.double()
    scale = 1.0 / math.sqrt(q.shape[-1])
    z = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(z, -1)
    p = torch.exp(z - lse.unsqueeze(-1))
    o = p @ v
    if dO is None:
        return Ref(z, p, lse, o, None, None, None, None, None)
    dO = dO.double()
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * o).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    return Ref(z, p, lse, o, dP, delta, scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), p.transpose(-1, -2) @ dO)


def bf(x):
    """Round to bf16 and back to float64 (float64 -> bf16 is one correctly rounded step in torch)."""
    return x.to(BF16).double()


FAULTS = ("row_ignores_key0", "last_key_masked", "pad_counted", "swap_keys", "dv_shift")


def emulate(q, k, v, dO, fault: str | None = None):
    """The composition the kernels compute, in float64 with their roundings to bf16: the unnormalised P
    (exp of score minus row maximum) and the output in the forward; P, dS, the o inside delta and every
    result in the backward; lse in fp32.  Stands in for a kernel on the CPU, and takes the faults of
    ``FAULTS`` (last query row ignores key 0; last valid key masked; one zero-filled padded key counted;
    V rows 1 and 2 swapped against K; dv rows shifted by one).  Returns (o, lse, dq, dk, dv) as
    [B, H, S, hd] bf16 / [B, H, S] fp32."""
    q, k, v, dO = q.double(), k.double(), v.double(), dO.double()
    S, hd = q.shape[-2:]
    scale = 1.0 / math.sqrt(hd)
    if fault == "pad_counted":
        pad = torch.zeros_like(k[..., :1, :])
        k, v = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
    vv = v
    if fault == "swap_keys":
        vv = v.clone()
        vv[..., 1, :], vv[..., 2, :] = v[..., 2, :], v[..., 1, :]
    z = (q @ k.transpose(-1, -2)) * scale
    if fault == "row_ignores_key0":
        z[..., S - 1, 0] = -math.inf
    if fault == "last_key_masked":
        z[..., S - 1] = -math.inf
    m = z.max(-1, keepdim=True).values
    pu = bf(torch.exp(z - m))
    l = pu.sum(-1, keepdim=True)
    o = bf(pu @ vv / l)
    lse = (m + torch.log(l)).squeeze(-1).float()
    p = torch.exp(z - lse.double().unsqueeze(-1))
    dP = dO @ vv.transpose(-1, -2)
    delta = (dO * o).sum(-1, keepdim=True)
    dS = bf(p * (dP - delta))
    dq = bf(scale * (dS @ k))
    dk = bf(scale * (dS.transpose(-1, -2) @ q))[..., :S, :]
    dv = bf(bf(p).transpose(-1, -2) @ dO)[..., :S, :]
    if fault == "dv_shift":
        dv = torch.roll(dv, 1, -2)
    return o.to(BF16), lse, dq.to(BF16), dk.to(BF16), dv.to(BF16)


# ------------------------------------------------------------------ inputs
def _ints(gen, shape, hi=INT_MAX):
    return torch.randint(-hi, hi + 1, shape, generator=gen, dtype=torch.int64).double()


def _codes(gen, B, H, S, hd, T):
    """+-1 codes [B, H, S, hd], own set per (b, h), pairwise dot products at most T (so all distinct):
    of every pair that breaks the limit the later code is redrawn until none is left."""
    c = torch.randint(0, 2, (B, H, S, hd), generator=gen, dtype=torch.int64).double() * 2 - 1
    for _ in range(1000):
        g = c @ c.transpose(-1, -2)
        bad = (torch.triu(g, 1) > T).any(-2)  # [B, H, S]: code j clashes with an earlier one
        n = int(bad.sum())
        if n == 0:
            return c
        c[bad] = torch.randint(0, 2, (n, hd), generator=gen, dtype=torch.int64).double() * 2 - 1
    raise AssertionError("no code set found")


@dataclass
class Case:
    kind: str
    shape: tuple
    q: torch.Tensor      # [B, H, S, hd] float64, bf16 numbers
    k: torch.Tensor
    v: torch.Tensor
    dO: torch.Tensor
    ref: Ref
    pi: torch.Tensor | None = None  # A: [B, H, S], the key query i selects

    @property
    def H(self):
        return self.shape[2]

    def qkv(self):
        return pack(self.q, self.k, self.v)

    def dO_packed(self):
        return pack_o(self.dO)


@functools.lru_cache(maxsize=None)
def make_case(kind: str, shape: tuple, device: str = "cpu") -> Case:
    """Inputs (drawn on the CPU from a generator seeded by kind and shape) and their float64 reference on
    ``device``, computed once and left unchanged.  kind: A, B, Bm (mirror), C, R."""
    B, S, H, hd = shape
    gen = torch.Generator().manual_seed(seed_of(kind, shape))
    pi = None
    dO = _ints(gen, (B, H, S, hd))
    if kind == "A":
        c, T = CODES[hd]
        code = _codes(gen, B, H, S, hd, T)
        pi = torch.argsort(torch.rand(B, H, S, generator=gen), -1)
        k = c * code
        q = c * torch.gather(code, 2, pi.unsqueeze(-1).expand(B, H, S, hd))
        v = _ints(gen, (B, H, S, hd))
        pi = pi.to(device)
    elif kind in ("B", "Bm", "C"):
        d = torch.arange(hd)
        v = (d[None, :] == (torch.arange(S) % hd)[:, None]).double().expand(B, H, S, hd).clone()
        x = _ints(gen, (B, H, S, hd))
        zero = torch.zeros(B, H, S, hd, dtype=F64)
        if kind == "B":
            q, k = zero, x
        elif kind == "Bm":
            q, k = x, zero
        else:
            q, k = zero + 2.0, zero - 2.0
    elif kind == "R":
        q, k, v = ((torch.randn(B, H, S, hd, generator=gen) * 1.5).to(BF16).double() for _ in range(3))
        dO = torch.randn(B, H, S, hd, generator=gen).to(BF16).double()
    else:
        raise ValueError(kind)
    q, k, v, dO = (t.to(device) for t in (q, k, v, dO))
    return Case(kind, shape, q, k, v, dO, reference(q, k, v, dO), pi)


def selector_conditions(case: Case):
    """(smallest gap between the best and the second-best score of a row in nats, largest |score| times
    log2(e), whether bf16(softmax(z) @ v) == v[pi] exactly) of an A case, from the reference alone."""
    r = case.ref
    S = case.shape[1]
    top = torch.topk(r.z, min(2, S), -1).values
    gap = float((top[..., 0] - top[..., 1]).min()) if S > 1 else math.inf
    sel = torch.gather(case.v, 2, case.pi.unsqueeze(-1).expand_as(case.v))
    assert torch.equal(r.z.argmax(-1), case.pi)
    return gap, float(r.z.abs().max()) * math.log2(math.e), torch.equal(r.o.to(BF16).double(), sel)


# ------------------------------------------------------------------ shared assertions
def worst(out, ref, bound):
    """(max |out - ref| / bound with 0 / 0 = 0, flat index); NaN or an error at a zero bound gives inf."""
    err = (out.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    i = int(r.argmax())
    return float(r.flatten()[i]), i


def _within(what, out, ref, bound, log):
    r, i = worst(out, ref, bound)
    log(f"  {what}: worst |err| / bound = {r:.4f} at flat index {i}: out {float(out.flatten()[i])!r}, "
        f"ref {float(ref.flatten()[i])!r}")
    assert r <= 1.0, (what, r, i)
    return r


def _finite(**ts):
    for n, t in ts.items():
        assert bool(torch.isfinite(t.float()).all()), f"{n} is not finite"


def _zero(what, t):
    assert bool((t == 0).all()), (what, "not exactly zero", float(t.double().abs().max()))  # -0.0 == 0


def check_lse(what, lse, ref, log=print, floor=0.0):
    """|lse - ref| <= 4 fp32 ulps of |ref| (the scale product, the log2-to-ln product, the sum, one
    spare), plus ``floor``."""
    assert lse.dtype == torch.float32
    return _within(what, lse, ref, 4 * ULP32 * ref.abs() + floor + 1e-300, log)


def check_selector_fwd(case: Case, o, lse, log=print):
    """A: o[b, h, i] == v[b, h, pi(i)] bit for bit, lse within 4 fp32 ulps."""
    _finite(o=o, lse=lse)
    sel = torch.gather(case.v, 2, case.pi.unsqueeze(-1).expand_as(case.v))
    bad = (o.double() != sel).any(-1)
    assert not bool(bad.any()), ("o != v[pi]", int(bad.sum()), "rows, first (b, h, i) =", bad.nonzero()[0].tolist())
    check_lse("A lse", lse, case.ref.lse, log)


def check_selector_bwd(case: Case, dq, dk, dv, log=print):
    """A: dv[b, h, pi(i)] == dO[b, h, i] bit for bit, dq == dk == 0."""
    _finite(dq=dq, dk=dk, dv=dv)
    got = torch.gather(dv.double(), 2, case.pi.unsqueeze(-1).expand_as(case.v))
    bad = (got != case.dO).any(-1)
    if bool(bad.any()):
        b, h, i = bad.nonzero()[0].tolist()
        ratio = got[b, h, i] / case.dO[b, h, i]
        log(f"  A dv: {int(bad.sum())} rows differ; first (b, h, i) = {(b, h, i)}, dv / dO = "
            f"{ratio[torch.isfinite(ratio)][:4].tolist()}")
    assert not bool(bad.any()), ("dv[pi(i)] != dO[i]", int(bad.sum()), "rows")
    _zero("A dq", dq)
    _zero("A dk", dk)


def check_selector_dbias(case: Case, dbias, fill=0.5):
    """A, fused bias gradient on a dbias pre-filled with ``fill``: the v part is fill + sum(dO) exactly
    (integers below 2**24 in any order), the q and k parts stay ``fill``."""
    B, S, H, hd = case.shape
    d = dbias.double().view(3, H, hd)
    assert torch.equal(d[2], fill + case.dO.sum((0, 2))), "dbias v part"
    assert bool((d[:2] == fill).all()), "dbias q / k parts"


def _uniform_o(case: Case, o, log):
    """o against count(j == d mod hd) / S, within 2**-8 of it: the output's bf16 rounding (2**-9) and as
    much again for the reciprocal and the product."""
    B, S, H, hd = case.shape
    ref = (case.v[0, 0].sum(0) / S).expand(B, H, S, hd)
    _within(f"{case.kind} o", o, ref, 2.0 ** -8 * ref, log)


def check_uniform(case: Case, o, lse, dq, dk, dv, log=print):
    """B and its mirror: lse against ln S, o against the key counts, dv and dq (mirror: dk) per element
    against the fp64 reference; the other gradient is exactly zero."""
    B, S, H, hd = case.shape
    r = case.ref
    _finite(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    check_lse(f"{case.kind} lse", lse, torch.full_like(r.lse, math.log(S)), log, floor=2.0 ** -22)
    _uniform_o(case, o, log)
    # roundings on the path: P in bf16 and the bf16 result.  2**-7, not the 2**-8 of two roundings at
    # 2**-9 each: a bf16 rounding is within 2**-9 of the power of two below the value, which is 2**-8 of a
    # value just above that power, and every P of a row here is the SAME number, so its error does not
    # average out.  At S = 30, bf16(1 / 30) is off by 0.87 * 2**-8, and the float64 composition with only
    # these two roundings reaches 1.02 of the 2**-8 bound in a column whose dO share one sign
    # (test_attn_ref.py, hd 64, B 9); 2**-8 per rounding is the worst case of the format.
    _within(f"{case.kind} dv", dv, r.dv, 2.0 ** -7 * (r.p.transpose(-1, -2) @ case.dO.abs()) + 1e-300, log)
    scale = 1.0 / math.sqrt(hd)
    w = r.p * (r.dP.abs() + r.delta.abs())  # dS in bf16, o in bf16 inside delta: 2**-7 of the terms of dS
    if case.kind == "B":
        _zero("B dk", dk)
        if S > 1:
            _within("B dq", dq, r.dq, 2.0 ** -7 * scale * (w @ case.k.abs()) + 2.0 ** -9 * r.dq.abs() + 1e-300, log)
    else:
        _zero("Bm dq", dq)
        if S > 1:
            _within("Bm dk", dk, r.dk,
                    2.0 ** -7 * scale * (w.transpose(-1, -2) @ case.q.abs()) + 2.0 ** -9 * r.dk.abs() + 1e-300, log)


def check_negative(case: Case, o, lse, log=print):
    """C: o as in B; lse against score + ln S within 4 fp32 ulps of |score| + ln S."""
    B, S, H, hd = case.shape
    _finite(o=o, lse=lse)
    score = -4.0 * math.sqrt(hd)
    ref = torch.full_like(case.ref.lse, score + math.log(S))
    _within("C lse", lse, ref, 4 * ULP32 * (abs(score) + math.log(S)) + 1e-300, log)
    _uniform_o(case, o, log)


def check_random_fwd(case: Case, o, log=print):
    """R: |o - ref| <= 2**-8 (|ref| + sum_j p_j |v_j|) per element: bf16 rounding of P and of the result,
    2**-9 each relative to the term it rounds, doubled."""
    _finite(o=o)
    r = case.ref
    return _within("R o", o, r.o, 2.0 ** -8 * (r.o.abs() + r.p @ case.v.abs()), log)
