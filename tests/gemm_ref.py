"""Exactly summable GEMM operands, fp64 references and the shared assertions of the GEMM kernel tests.

Used by tests/test_gemm_exact_gpu.py and tests/test_gemm_tn_exact_gpu.py (the kernels of csrc/gemm.hip
and csrc/gemm_tn.hip) and by tests/test_gemm_ref.py, which keeps this module honest without a GPU.

Why exact.  ``exact_operands`` draws A as small integers and B (and the bias) as small integers times
``2**-s`` (the bias with ``BIAS_FRAC`` more fractional bits).  Every product, every partial sum of products
and the sum plus bias is then an integer multiple of the finest unit below ``2**24`` units, so it is an fp32 number: fp32 accumulation is exact
in ANY summation order, split-K / split-M plan or pipeline, the accumulator is a pure function of the
inputs, and what the epilogue stores can be compared element by element with ``torch.equal`` --

  h       = RNE_bf16(acc + bias)                       EPI_STORE, first output of EPI_GELU
  gelu    = RNE_bf16(gelu32(h)), gelu' likewise        on the ROUNDED h, which is what the backward sees
  dh      = RNE_bf16(RNE_bf16(acc) * gelu')            EPI_DGELU / EPI_DMUL
  dbias  += column sums of the rounded dh

(csrc/gemm.hip ``epilogue`` / ``epilogue_lds``, csrc/common.h).  gelu32 is one v_exp_f32 and one
v_rcp_f32 in the sigmoid form; the references here are the same form in float64 (``gelu64``,
``dgelu64``).  The tanh form 0.5 x (1 + tanh u) is never used: it cancels for x < -6.7 and is off by more
than a bf16 ulp on dozens of bf16 values in [-9.25, -6.72] even in float64.

Operands come as views into larger NaN-filled buffers (``poisoned_view``): a kernel that consumes a row
>= M, a column >= K or the padding between rows puts a NaN into an output element.
"""

from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

F64 = torch.float64
BF16 = torch.bfloat16
EXACT = 2 ** 24          # integers below this magnitude are fp32 numbers
BIAS_MAX = 8             # |bias| in units of 2**-s
BIAS_FRAC = 6            # the bias has this many more fractional bits than the products (see exact_operands)
POISON_ROWS = 256        # NaN rows before and after an operand view
POISON_COL0 = 64         # first column of the view inside its buffer (elements)

# |out - ref| <= GELU_REL |ref| + GELU_FLOOR for a bf16 GELU output against gelu64 of the same bf16 h:
# 2**-8 is the worst-case half ulp of bf16 relative to the value, 2**-12 covers the fp32 exp / reciprocal
# evaluation (test_gemm_ref.py: the fp32 emulation alone stays within it), 1e-30 the results that the
# fp32 evaluation flushes to zero (exp overflow: |gelu| < 1e-36 there).
GELU_REL = 2.0 ** -8 + 2.0 ** -12
GELU_FLOOR = 1e-30
# |gelu'32 - gelu'64| of the fp32 evaluation (common.h gelu_and_grad_f / gelu_n), absolute, over every bf16
# |x| <= 12: the fp32 emulation of test_gemm_ref.py measures 1.9e-6 (|gelu'| <= 1.13, so about 14 fp32
# unit roundoffs of a value near 1: p carries the exp argument's rounding, x p (1 - p) (..) three more
# products), hence 2e-6 and not 1e-6
DGELU_ABS = 2e-6

GELU_C = math.sqrt(2.0 / math.pi)
GELU_A = 0.044715
SAT = 16.0               # |pre-activation| at which the kernels' gelu' is exactly 1.0f / 0.0f


def seed_of(*key) -> int:
    """A seed that is a pure function of ``key``: every launch of every case gets its own, so stale
    allocator contents of an earlier launch can never equal the expected output."""
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------ operands
def poisoned_view(t: torch.Tensor, fill: float = float("nan")) -> torch.Tensor:
    """``t`` [R, C] as the view ``buf[r0:r0+R, c0:c0+C]`` of a larger buffer filled with ``fill``:
    ``POISON_ROWS`` rows before and after, ``c0`` = ``POISON_COL0`` and a row stride that is a multiple
    of 64 elements and at least C + 128."""
    R, C = t.shape
    ld = (POISON_COL0 + C + 64 + 63) // 64 * 64
    buf = torch.full((POISON_ROWS + R + POISON_ROWS, ld), fill, dtype=t.dtype, device=t.device)
    v = buf[POISON_ROWS:POISON_ROWS + R, POISON_COL0:POISON_COL0 + C]
    v.copy_(t)
    assert v.stride(0) > C and v.stride(0) % 64 == 0 and v.stride(1) == 1
    return v


def _ints(gen: torch.Generator, shape, hi: int) -> torch.Tensor:
    return torch.randint(-hi, hi + 1, shape, generator=gen, dtype=torch.int64)


def grid_scale(K: int, a_max: int, b_max: int) -> int:
    """s such that std(A . B^T) / 2**s lies in [1, 2): a uniform integer in [-m, m] has variance
    m (m + 1) / 3, the K products are independent."""
    std_units = math.sqrt(K * (a_max * (a_max + 1) / 3.0) * (b_max * (b_max + 1) / 3.0))
    return max(0, math.floor(math.log2(std_units)))


def check_exact(K: int, a_max: int, b_max: int, *, rows: int = 1, extra: int = BIAS_MAX) -> None:
    """The exactness condition, in units of 2**-s: every partial sum is an integer of magnitude at most
    K a_max b_max + extra.  ``rows`` > 1: column sums over that many bf16-ROUNDED outputs must be exact as
    well (rounding to bf16 keeps a value on the grid and raises its magnitude by at most 2**-8)."""
    assert a_max <= 256 and b_max <= 256, "operand entries must be bf16 integers"
    bound = (K * a_max * b_max + extra) * 2 ** BIAS_FRAC  # in units of the bias's finer grid
    if rows > 1:  # bias-free products and a dbias0 of up to 64, in units of 2**-s
        bound = max(bound, rows * K * a_max * b_max * (1.0 + 2.0 ** -8) + 64)
    assert bound < EXACT, f"not exactly summable in fp32: {bound} >= 2**24 units"


@dataclass
class Operands:
    A: torch.Tensor      # bf16 [M, K], integers
    B: torch.Tensor      # bf16 [N, K], integers times 2**-s
    bias: torch.Tensor   # fp32 [N], integers times 2**-s
    s: int

    @property
    def unit(self) -> float:
        return 2.0 ** -self.s

    def acc64(self) -> torch.Tensor:
        """A . B^T in float64 (exact)."""
        return self.A.double() @ self.B.double().t()

    def h64(self) -> torch.Tensor:
        return self.acc64() + self.bias.double()

    def grid(self, shape, seed: int, hi: int = 64, dtype=torch.float32) -> torch.Tensor:
        """Random values on the same 2**-s grid (addends, initial bias gradients)."""
        gen = torch.Generator().manual_seed(seed)
        return (_ints(gen, shape, hi).double() * self.unit).to(dtype).to(self.A.device)


def exact_operands(M: int, K: int, N: int, seed: int, *, a_max: int = 2, b_max: int = 2, colsum_rows: int = 1,
                   strided: bool = True, device="cpu") -> Operands:
    """bf16 A [M, K] (integers in [-a_max, a_max]), B [N, K] (integers in [-b_max, b_max] times 2**-s)
    and an fp32 bias [N] in [-8, 8] times 2**-s; ``strided``: A and B are views into NaN-filled buffers
    (``poisoned_view``), else contiguous.  ``colsum_rows`` = M for the cases that also compare column sums
    exactly (use a_max = 1 there).

    The bias is an integer times 2**-(s + BIAS_FRAC): on the products' own grid acc + bias would be a bf16
    number already (|h| < 8 on a 2**-5 grid has 8 significant bits) and RNE_bf16 a no-op, so an epilogue that
    applied GELU to the unrounded value would pass.  With 6 more fractional bits h = acc + bias is still
    exact in fp32 (``check_exact`` counts in the finer units) but almost never a bf16 number."""
    check_exact(K, a_max, b_max, rows=colsum_rows)
    s = grid_scale(K, a_max, b_max)
    gen = torch.Generator().manual_seed(seed)
    unit = 2.0 ** -s
    A = _ints(gen, (M, K), a_max).to(BF16)
    B = (_ints(gen, (N, K), b_max).double() * unit).to(BF16)
    bias = (_ints(gen, (N,), BIAS_MAX * 2 ** BIAS_FRAC).double() * unit / 2 ** BIAS_FRAC).float()
    A, B, bias = A.to(device), B.to(device), bias.to(device)
    if strided:
        A, B = poisoned_view(A), poisoned_view(B)
    return Operands(A, B, bias, s)


def saturated_pre(M: int, N: int, seed: int, device="cpu") -> torch.Tensor:
    """bf16 [M, N] of random +-16: the kernels' fp32 gelu' is exactly 1.0f at +16 (exp underflows to 0,
    rcp(1) = 1) and exactly 0.0f at -16 (exp overflows to inf, rcp(inf) = 0)."""
    gen = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (M, N), generator=gen, dtype=torch.int8).to(device)
    return ((sign.float() * 2 - 1) * SAT).to(BF16)


def saturated_codes(pre: torch.Tensor) -> torch.Tensor:
    """The uint8 gelu' codes of a ``saturated_pre``: 229 (= 195 + GD_Z, gelu' = 1) where it is positive,
    34 (GD_Z, gelu' = 0) where negative.  Code 34 decodes to exactly 0; code 229 to 195 fl(1 / 195) =
    1 + 3e-8, which cannot move an already-bf16 value across a rounding boundary."""
    return torch.where(pre > 0, 229, 34).to(torch.uint8)


# ------------------------------------------------------------------ fp64 references
def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest even to bf16 (torch's conversion), from float64 without an fp32 step in between
    that could double-round: every value given to it here is an fp32 number already."""
    return x.to(BF16)


def gelu_p64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 1.0 / (1.0 + torch.exp(-2.0 * GELU_C * (x + GELU_A * x ** 3)))


def gelu64(x: torch.Tensor) -> torch.Tensor:
    """tanh-approximated GELU in its sigmoid form x p, p = 1 / (1 + exp(-2 c (x + 0.044715 x^3)))."""
    return x.double() * gelu_p64(x)


def dgelu64(x: torch.Tensor) -> torch.Tensor:
    """Its derivative p + x p (1 - p) 2 c (1 + 3 0.044715 x^2)."""
    x = x.double()
    p = gelu_p64(x)
    return p + x * p * (1.0 - p) * 2.0 * GELU_C * (1.0 + 3.0 * GELU_A * x * x)


# ------------------------------------------------------------------ fp32 emulation of csrc/common.h
def gelu32_emul(x: torch.Tensor, form: str = "exp"):
    """(gelu, gelu') as common.h evaluates them in fp32, with correctly rounded exp and reciprocal in
    place of v_exp_f32 / v_rcp_f32 and no fused multiply-adds.  ``exp``: gelu_p_f / gelu_and_grad_f (the
    register epilogue), ``exp2``: gelu_n with log2(e) folded into the polynomial (the LDS epilogue)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    x = x.float()
    x2 = x * x
    if form == "exp":
        m = x * (f(-1.5957691216057308) - f(0.07135481627260025) * x * x)
        e = torch.exp(m)
    else:
        m = x * (x2 * f(-0.07135481627260025 * 1.4426950408889634) + f(-1.5957691216057308 * 1.4426950408889634))
        e = torch.exp2(m)
    p = 1.0 / (1.0 + e)
    g = x * p
    d = (g * (1.0 - p)) * (x2 * f(0.21406444881780076) + f(1.5957691216057308)) + p
    return g, d


def all_bf16(max_abs: float) -> torch.Tensor:
    """Every finite bf16 value with |x| <= max_abs (both zeros included)."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF16)
    return v[torch.isfinite(v.float()) & (v.float().abs() <= max_abs)]


# ------------------------------------------------------------------ shared assertions
def worst_ratio(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """(max of |out - ref| / bound, flat index of that element); a NaN anywhere gives inf."""
    err = (out.double() - ref.double()).abs() / bound
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(err.argmax())
    return float(err.flatten()[i]), i


def assert_gelu(out: torch.Tensor, h_bf: torch.Tensor, scale: float = 1.0, what: str = "gelu") -> float:
    """A bf16 GELU output against scale gelu64 of the bf16 pre-activation, per element within
    ``GELU_REL`` |ref| + ``GELU_FLOOR``.  Returns the worst error / |ref| in units of 2**-8."""
    assert out.dtype == BF16 and out.shape == h_bf.shape
    ref = gelu64(h_bf) * scale
    r, i = worst_ratio(out, ref, GELU_REL * ref.abs() + GELU_FLOOR)
    print(f"{what}: worst |err| / bound = {r:.4f} (= {r * GELU_REL * 256:.4f} x 2^-8 |ref|) at h = "
          f"{float(h_bf.flatten()[i])}, out = {float(out.flatten()[i])}, ref = {float(ref.flatten()[i])}")
    assert r <= 1.0, (what, r, float(h_bf.flatten()[i]))
    return r


def assert_dmul(out: torch.Tensor, a_bf: torch.Tensor, mul64: torch.Tensor, what: str = "dgelu") -> float:
    """EPI_DGELU / EPI_DMUL output against RNE_bf16(acc) * mul64 per element, within
    ``GELU_REL`` |ref| + ``DGELU_ABS`` |RNE_bf16(acc)|."""
    assert out.dtype == BF16 and a_bf.dtype == BF16 and out.shape == a_bf.shape
    ref = a_bf.double() * mul64.double()
    r, i = worst_ratio(out, ref, GELU_REL * ref.abs() + DGELU_ABS * a_bf.double().abs() + 1e-300)
    print(f"{what}: worst |err| / bound = {r:.4f} at acc = {float(a_bf.flatten()[i])}, mul = "
          f"{float(mul64.flatten()[i])}, out = {float(out.flatten()[i])}")
    assert r <= 1.0, (what, r)
    return r


def assert_colsum(dbias: torch.Tensor, dbias0: torch.Tensor, out: torch.Tensor, what: str = "dbias") -> None:
    """dbias - dbias0 against the float64 column sums of the kernel's own rounded output, within the
    worst-case fp32 summation bound M 2**-24 sum_m |out[m, n]| (+ one rounding of the final add)."""
    o = out.double()
    ref = dbias0.double() + o.sum(0)
    bound = out.shape[0] * 2.0 ** -24 * o.abs().sum(0) + 2.0 ** -24 * ref.abs() + 1e-300
    r, i = worst_ratio(dbias, ref, bound)
    assert r <= 1.0, (what, r, i)


def gd_check(dq, dref):
    """uint8 gelu' codes of the fused FF1 forward (csrc/common.h gd_code) against the fp32 derivative
    of the same bf16 pre-activation: the torch mirror's code up to one step (fma vs two roundings at
    exact ties), the decoded value within half a step.  Returns the decoded fp32 gelu'."""
    from jumbo_mae_tpu_amd.ops import prims as P
    assert dq.dtype == torch.uint8 and dq.shape == dref.shape
    assert (dq.int() - P.gd_encode(dref).int()).abs().max().item() <= 1
    d = P.gd_decode(dq, dtype=torch.float32)
    assert (d - dref).abs().max().item() <= 0.5 / P.GD_Q + 1e-4
    return d
