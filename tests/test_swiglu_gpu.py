"""csrc/swiglu.hip (``jm_swiglu_fwd`` / ``jm_swiglu_bwd``) against ``swiglu_torch`` / ``swiglu_bwd_torch``
(ops/swiglu.py) in fp64 on the same bf16 bits.  The reference is never the kernel.

Bounds, per element, in units of u = 2^-24 (one fp32 rounding, relative), derived from the kernel's operation
order; a hardware or library transcendental counts at its documented error: ``expf`` <= 1 ulp (HIP math API
accuracy table; its argument reduction is exact, so the error does not grow with |g|) = 2 u, ``v_rcp_f32`` 1 ulp
(CDNA ISA guide) = 2 u.  Second-order terms (< 2^-40) are covered by rounding every count up.

  sigma = rcp(1 + e), e = expf(-g):  e carries 2 u and enters sigma as e / (1 + e) <= 1 of it: 2; the add 1; the
      reciprocal 2                                                                            -> sigma: 5 u
  forward a = (g sigma) u:  sigma 5, two products 2; second order 1                            -> C_FWD = 8
      |got - ref| <= half a bf16 ulp of |ref| + 8 u |ref|
  t = 1 - sigma (g < 0: sigma <= 1/2 <= t, so sigma's 5 u sigma <= 5 u t, plus the subtraction 1) or e sigma
      (g >= 0: e 2, the add and the reciprocal inside sigma 3, the product 1)                  -> t: 6 u
  f = 1 + g t:  the product 7 u |g| t, the add 1 u |f| <= u (1 + |g| t)                        -> f: 8 u (1 + |g| t)
  gate half ((da u) sigma) f:  da u 1, sigma 5 and its product 1, f 8 and its product 1        -> C_GATE = 16
      of the magnitude |da| |u| sigma (1 + |g| (1 - sigma)) -- not of |ref|, which cancels near g = -1.278
  up half da (g sigma):  sigma 5, two products 2                                               -> C_UP = 7
      of |da| |silu(g)|
  dropout: the kept value (forward) / da (backward) times the fp32 1 / keep: that constant's own rounding 1, the
      product 1 (the reference uses the exact 1 / keep)                                        -> C_DROP = 2 more

Bias gradient, per column: |got - sum_rows ref64| <= sum_rows(element bound) + M u sum_rows |ref| (the fp32 sums of
the rounded dpre over slots, slabs and the column-sum pass: fewer than M additions)."""

import pytest
import torch

import swiglu_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (1, 128) smallest; (3, 136) Hs % 8 == 0 with 17 column groups: an idle lane in the workgroup; (257, 384) crosses
# a row slab, partial last slab; (5, 2816) more than one 2048-column chunk; (640, 768) many partial rows
SHAPES = [(1, 128), (3, 136), (257, 384), (5, 2816), (640, 768)]
RATE = 0.25


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


_CACHE = {}


def _case(M, Hs):
    """inputs and fp64 references of a shape, computed once and left unchanged"""
    if (M, Hs) not in _CACHE:
        pre, da = R.inputs(M, Hs, seed=M * 7 + Hs, device=DEV)
        seed = torch.tensor([1234567 + M], dtype=torch.int64, device=DEV)
        mask = R.mask64(seed, M, Hs, RATE, DEV)
        _CACHE[(M, Hs)] = dict(pre=pre, da=da, seed=seed, mask=mask, fwd=R.fwd_ref(pre), fwd_d=R.fwd_ref(pre, mask),
                               bwd=R.bwd_ref(pre, da), bwd_d=R.bwd_ref(pre, da, mask))
    return _CACHE[(M, Hs)]


def _fwd(pre, seed=None, rate=0.0):
    """one forward launch, twice: status 0 and identical bits"""
    rc, a = _ext().swiglu_fwd(pre, seed, rate)
    rc2, a2 = _ext().swiglu_fwd(pre, seed, rate)
    assert rc == 0 and rc2 == 0 and torch.equal(_bits(a), _bits(a2))
    return a


def _bwd(pre, da, bias=None, seed=None, rate=0.0):
    """one backward launch, twice, each on its own copy of ``bias``: status 0, identical bits"""
    b1 = None if bias is None else bias.clone()
    b2 = None if bias is None else bias.clone()
    rc, d = _ext().swiglu_bwd(pre, da, b1, seed, rate)
    rc2, d2 = _ext().swiglu_bwd(pre, da, b2, seed, rate)
    assert rc == 0 and rc2 == 0 and torch.equal(_bits(d), _bits(d2))
    if bias is not None:
        assert torch.equal(_bits(b1), _bits(b2))
    return d, b1


def _within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst err / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all(), what
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("M,Hs", SHAPES)
def test_forward(M, Hs):
    c = _case(M, Hs)
    a = _fwd(c["pre"])
    assert a.dtype == torch.bfloat16 and tuple(a.shape) == (M, Hs) and a.is_contiguous()
    _within(a, *c["fwd"], f"fwd {M}x{Hs}")


@pytest.mark.parametrize("M,Hs", SHAPES)
def test_backward_and_bias_gradient(M, Hs):
    c = _case(M, Hs)
    pre, da = c["pre"], c["da"]
    ref, bound = c["bwd"]
    zero = torch.zeros(2 * Hs, device=DEV)
    d, bg = _bwd(pre, da, zero)
    assert d.dtype == torch.bfloat16 and tuple(d.shape) == (M, 2 * Hs) and d.is_contiguous()
    _within(d[:, :Hs], ref[:, :Hs], bound[:, :Hs], f"bwd gate {M}x{Hs}")
    _within(d[:, Hs:], ref[:, Hs:], bound[:, Hs:], f"bwd up {M}x{Hs}")
    # the bias gradient: all 2 Hs columns
    cb = bound.sum(0) + M * R.U24 * ref.abs().sum(0)
    _within(bg, ref.sum(0), cb, f"bias grad {M}x{Hs}")
    # ... and it is the column sum of the rounded dpre, the values the GEMMs consume
    assert (bg.double() - d.double().sum(0)).abs().max().item() <= (M * R.U24 * d.double().abs().sum(0)).max().item()
    # the kernel accumulates: from a non-zero start the result is the one fp32 addition start + sum
    start = torch.linspace(-3.0, 5.0, 2 * Hs, device=DEV)
    d2, bg2 = _bwd(pre, da, start)
    assert torch.equal(_bits(d2), _bits(d))
    assert torch.equal(_bits(bg2), _bits(start + bg))
    # no bias gradient: nothing but dpre is written, and dpre keeps its bits
    d3, _ = _bwd(pre, da, None)
    assert torch.equal(_bits(d3), _bits(d))


@pytest.mark.parametrize("M,Hs", SHAPES)
def test_dropout(M, Hs):
    c = _case(M, Hs)
    pre, da, seed, mask = c["pre"], c["da"], c["seed"], c["mask"]
    keep = mask != 0
    a = _fwd(pre, seed, RATE)
    ref, bound = c["fwd_d"]
    _within(a, ref, bound, f"fwd drop {M}x{Hs}")
    # the zero pattern is the mirror's mask exactly (where the undropped value is not itself zero)
    live = c["fwd"][0] != 0
    assert torch.equal((a != 0) & live, keep & live) and bool((a[~keep] == 0).all())
    d, bg = _bwd(pre, da, torch.zeros(2 * Hs, device=DEV), seed, RATE)
    rb, bb = c["bwd_d"]
    _within(d, rb, bb, f"bwd drop {M}x{Hs}")
    for half, r0 in ((d[:, :Hs], c["bwd"][0][:, :Hs]), (d[:, Hs:], c["bwd"][0][:, Hs:])):
        live = r0 != 0
        assert torch.equal((half != 0) & live, keep & live) and bool((half[~keep] == 0).all())
    _within(bg, rb.sum(0), bb.sum(0) + M * R.U24 * rb.abs().sum(0), f"bias grad drop {M}x{Hs}")
    # the kept share: within 5 binomial standard deviations of 0.75
    n = M * Hs
    assert abs(keep.double().mean().item() - (1 - RATE)) <= 5 * (RATE * (1 - RATE) / n) ** 0.5
    # rate 0: the bits of the call without dropout
    assert torch.equal(_bits(_fwd(pre, seed, 0.0)), _bits(_fwd(pre)))
    assert torch.equal(_bits(_bwd(pre, da, None, seed, 0.0)[0]), _bits(_bwd(pre, da)[0]))


def test_statuses_and_the_wrappers_fallback():
    """Hs % 8 != 0: the negative status, and ops/prims.py then gives the mirror's result."""
    from jumbo_mae_tpu_amd.ops import prims as P
    from jumbo_mae_tpu_amd.ops.swiglu import swiglu_bwd_torch, swiglu_torch
    ext = _ext()
    g = torch.Generator().manual_seed(3)
    pre = torch.randn(6, 2 * 12, generator=g).to(torch.bfloat16).to(DEV)
    da = torch.randn(6, 12, generator=g).to(torch.bfloat16).to(DEV)
    assert ext.swiglu_fwd(pre)[0] < 0 and ext.swiglu_bwd(pre, da)[0] < 0
    assert ext.swiglu_ws_floats(6, 12) == 0 and ext.swiglu_ws_floats(0, 128) == 0 and ext.swiglu_ws_floats(6, 128) > 0
    assert torch.equal(_bits(P.swiglu_fwd(pre)), _bits(swiglu_torch(pre.float()).to(torch.bfloat16)))
    dpre, done = P.swiglu_bwd(pre, da)
    assert not done and torch.equal(_bits(dpre), _bits(swiglu_bwd_torch(pre.float(), da.float()).to(torch.bfloat16)))
    # a shape the kernels take goes to them: the wrapper returns their bits
    c = _case(3, 136)
    assert torch.equal(_bits(P.swiglu_fwd(c["pre"])), _bits(_fwd(c["pre"])))
    assert torch.equal(_bits(P.swiglu_fwd(c["pre"], (c["seed"], RATE))), _bits(_fwd(c["pre"], c["seed"], RATE)))
    assert ext.debug_lines().get("swiglu", 0) == 0
