"""tests/gemm_ref.py checked on the CPU: the operands really are exactly summable, the float64 GELU
references really are the accurate ones, and the bounds that the GPU tests assert are met by an fp32
evaluation of csrc/common.h's formulas with correctly rounded exp / reciprocal -- so a GPU failure of
those bounds is the kernel's, not the reference's."""

import pytest
import torch

import gemm_ref as R


def test_exactness_assertion_fires():
    R.check_exact(384, 2, 2)
    R.check_exact(1024, 1, 2, rows=4352)
    with pytest.raises(AssertionError, match="exactly summable"):
        R.check_exact(2 ** 16, 2, 2)
    with pytest.raises(AssertionError, match="exactly summable"):
        R.check_exact(1024, 2, 2, rows=4352)  # column sums over 4352 rows need a_max = 1
    with pytest.raises(AssertionError, match="exactly summable"):
        R.exact_operands(8, 2 ** 16, 8, 0)
    with pytest.raises(AssertionError, match="bf16 integers"):
        R.check_exact(64, 257, 1)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("M,K,N,a_max", [(37, 384, 29, 2), (19, 1024, 23, 1), (33, 64, 17, 2)])
def test_operands_are_on_the_grid_and_order_independent(M, K, N, a_max, strided):
    """An fp32 matmul in two summation orders (torch's own, and K split 3 ways then summed, the splits in
    reverse) equals the float64 product bit for bit, with and without the bias."""
    op = R.exact_operands(M, K, N, R.seed_of("cpu", M, K, N), a_max=a_max, strided=strided)
    assert op.A.dtype == op.B.dtype == torch.bfloat16 and op.bias.dtype == torch.float32
    assert op.A.shape == (M, K) and op.B.shape == (N, K) and op.bias.shape == (N,)
    assert op.A.is_contiguous() != strided and op.B.is_contiguous() != strided
    a, b = op.A.double(), op.B.double() * 2.0 ** op.s
    assert torch.equal(a, a.round()) and a.abs().max() <= a_max and a.abs().max() == a_max
    assert torch.equal(b, b.round()) and b.abs().max() == 2
    bi = op.bias.double() * 2.0 ** (op.s + R.BIAS_FRAC)
    assert torch.equal(bi, bi.round()) and bi.abs().max() <= R.BIAS_MAX * 2 ** R.BIAS_FRAC
    h64 = op.h64()
    # the bf16 rounding of h is not a no-op (the finer bias grid), that of the bare product is
    assert float((R.rne_bf16(h64).double() != h64).double().mean()) > 0.5
    assert torch.equal(R.rne_bf16(op.acc64()).double(), op.acc64()) or K > 512
    assert 1.0 <= float(op.acc64().std()) < 2.0 or min(M, N) < 20
    A32, B32 = op.A.float(), op.B.float()
    assert torch.equal((A32 @ B32.t() + op.bias).double(), h64)
    cuts = [0, K // 3 // 8 * 8, 2 * K // 3 // 8 * 8, K]
    parts = [A32[:, lo:hi] @ B32[:, lo:hi].t() for lo, hi in zip(cuts[:-1], cuts[1:])]
    split = (parts[2] + parts[1]) + parts[0]
    assert torch.equal((split + op.bias).double(), h64)
    assert torch.equal(split.double(), op.acc64())
    # the bf16 rounding of the reference is that of the fp32 value (no double rounding through fp64)
    assert torch.equal(R.rne_bf16(h64), (A32 @ B32.t() + op.bias).bfloat16())


def test_grid_scale_matches_the_measured_spread():
    assert R.grid_scale(384, 2, 2) == 5
    op = R.exact_operands(512, 384, 512, 1, strided=False)
    acc = op.acc64()
    assert 1.0 <= float(acc.std()) < 2.0 and float(acc.abs().max()) < 8.0


def test_poisoned_view_surroundings():
    t = torch.arange(6 * 64, dtype=torch.float32).view(6, 64).bfloat16()
    v = R.poisoned_view(t)
    assert torch.equal(v, t) and v.stride(0) % 64 == 0 and v.stride(0) > 64
    assert v.storage_offset() == R.POISON_ROWS * v.stride(0) + R.POISON_COL0 and R.POISON_COL0 % 64 == 0
    buf = torch.empty(0, dtype=t.dtype).set_(v.untyped_storage()).view(-1, v.stride(0))
    assert buf.shape[0] == 6 + 2 * R.POISON_ROWS
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[R.POISON_ROWS:R.POISON_ROWS + 6, R.POISON_COL0:R.POISON_COL0 + 64] = True
    assert bool(torch.isnan(buf.float()[~inside]).all()) and int(inside.sum()) == t.numel()


@pytest.mark.parametrize("form", ["exp", "exp2"])
def test_gelu64_bounds_the_fp32_evaluation(form):
    """Every finite bf16 |x| <= 12: the fp32 evaluation of common.h's GELU, rounded to bf16, stays within
    the bound that the GPU tests assert against ``gelu64`` -- the reference alone does not use it up (worst
    case just under a bf16 half ulp, 2**-8 |ref|) -- and its fp32 gelu' within ``DGELU_ABS``."""
    x = R.all_bf16(12.0)
    assert x.numel() > 33000
    g32, d32 = R.gelu32_emul(x, form)
    ref = R.gelu64(x)
    err = (g32.bfloat16().double() - ref).abs()
    bound = R.GELU_REL * ref.abs() + R.GELU_FLOOR
    assert int((err > bound).sum()) == 0
    nz = ref.abs() > 1e-30
    worst = float((err[nz] / ref[nz].abs()).max()) * 2 ** 9
    print(f"worst bf16(gelu32) error: {worst:.3f} x 2^-9 |ref|")
    assert worst < 2.0
    # before the bf16 rounding the fp32 value is far inside the 2**-12 margin
    assert float(((g32.double() - ref).abs()[nz] / ref[nz].abs()).max()) < 2.0 ** -12 / 8
    derr = float((d32.double() - R.dgelu64(x)).abs().max())
    print(f"worst fp32 gelu' error: {derr:.3e}")
    assert 1e-7 < derr <= R.DGELU_ABS
    assert float(R.dgelu64(x).abs().max()) < 1.13


def test_tanh_form_is_the_inaccurate_one():
    """Why the references use the sigmoid form: 0.5 x (1 + tanh u) in float64 is off by more than a bf16
    ulp (2**-7 relative) on dozens of bf16 values of the negative tail."""
    x = R.all_bf16(12.0).double()
    u = R.GELU_C * (x + R.GELU_A * x ** 3)
    tanh_form = 0.5 * x * (1.0 + torch.tanh(u))
    ref = R.gelu64(x)
    nz = ref.abs() > 1e-300
    bad = ((tanh_form - ref).abs()[nz] > 2.0 ** -7 * ref[nz].abs())
    assert int(bad.sum()) >= 40
    assert float(x[nz][bad].max()) < -6.5


def test_saturation_at_16():
    """+-16: fp32 gelu' is exactly 1 / 0 (and gelu exactly x / 0) in both evaluation forms, the codes are
    229 / 34 and decode to exactly 0 and to a factor that leaves every bf16 value in place."""
    from jumbo_mae_tpu_amd.ops import prims as P

    pre = R.saturated_pre(64, 40, 3)
    assert pre.dtype == torch.bfloat16 and bool((pre.float().abs() == R.SAT).all())
    assert 0.3 < float((pre > 0).float().mean()) < 0.7
    for form in ("exp", "exp2"):
        g, d = R.gelu32_emul(pre, form)
        assert torch.equal(d, (pre > 0).float())
        assert torch.equal(g, torch.where(pre > 0, pre.float(), torch.zeros(())))
    assert float((R.dgelu64(pre) - (pre > 0).double()).abs().max()) < 1e-30
    q = R.saturated_codes(pre)
    assert torch.equal(q, P.gd_encode((pre > 0).float()))
    assert P.GD_Z == 34 and set(q.unique().tolist()) == {34, 229}
    s = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(195.0, dtype=torch.float32)
    one = float(torch.tensor(195.0, dtype=torch.float32) * s)
    assert (34.0 - P.GD_Z) * float(s) == 0.0 and abs(one - 1.0) < 1e-7
    v = R.all_bf16(3e38).float()
    assert torch.equal((v * torch.tensor(one, dtype=torch.float32)).bfloat16(), v.bfloat16())


def test_column_sums_stay_exact_under_the_rows_condition():
    """The x M condition: fp32 column sums of the bf16-rounded outputs, in two orders, equal float64."""
    M, K, N = 4352, 1024, 16
    op = R.exact_operands(M, K, N, 9, a_max=1, colsum_rows=M, strided=False)
    out = R.rne_bf16(op.acc64())
    d0 = op.grid((N,), 10)
    ref = d0.double() + out.double().sum(0)
    o32 = out.float()
    assert torch.equal((d0 + o32.sum(0)).double(), ref)
    assert torch.equal((d0 + o32.view(17, 256, N).sum(1).flip(0).sum(0)).double(), ref)
