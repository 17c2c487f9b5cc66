"""The attention kernels of csrc/attention.hip per element on structured inputs (tests/attn_ref.py): a
one-hot P with exact equalities (A), a uniform P against bounds derived from the reference's own terms
(B, its mirror), uniform negative scores against the key mask (C), and a per-element bound on the
random-input forward (R) (MI355X).

Each test id names the instantiation its shape reaches: head dim, S, B, H, the dispatch_sp bucket SP
("ex": the EX = S > SP - 32 variant; "stream": the tile-streamed kernels), the forward kind (fwd_ml: 4 (b, h)
pairs per workgroup, fwd: one pair, fwd_long) and the backward kind (bwd2, bwd3x4 / bwd3x8: 4 / 8 waves,
bwd_dq+bwd_dkv).  tests/test_attn_ref.py asserts that the list holds every reachable row of
dispatch_sp x {EX, not EX} x {hd 32, 64} and the tile-streamed kernels at all five head dims:

  HD      SP   EX     forward   backward        S in the list
  32      32   yes    fwd_ml    bwd3x4          17
  32      64   yes    fwd_ml    bwd3x4          33 64
  32      128  no     fwd       bwd3x4          72
  32      128  yes    fwd       bwd3x4          97 128
  32      224  no     fwd       bwd3x4          160
  32      224  yes    fwd       bwd3x4          197 208 209 224
  64      32   yes    fwd_ml    bwd2            19 30            (B = 9: bwd2 groups of 8 + 1)
  64      64   yes    fwd_ml    bwd2            52 64            (B = 9, and S 52 at B = 16)
  64      128  no     fwd       bwd3x8          80
  64      128  yes    fwd       bwd3x8          100 128
  64      224  no     fwd       bwd3x8          160
  64      224  yes    fwd       bwd3x8          199 224
  32 64   -    -      fwd_long  bwd_dq+bwd_dkv  225 259 321
  80 96 128 -  -      fwd_long  bwd_dq+bwd_dkv  1 52 64 65 259
(SP 32 and 64 have no EX = no row: every S they take is above SP - 32.)

qkv, dO and o reach the kernels through NaN-backed buffers and every output is asserted finite.
"""

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.shape_id(s) for s in R.SHAPES]
IDS_C = [R.shape_id(s) for s in R.SHAPES_C]
IDS_R = [R.shape_id(s) for s in R.SHAPES_R]


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _forward(ext, case):
    B, S, H, hd = case.shape
    qkv = R._nan_backed(case.qkv())
    o, lse = ext.attn_fwd(qkv, H)
    assert o.shape == (B, S, H * hd) and lse.shape == (B, H, S)
    return qkv, o, lse


def _backward(ext, case, qkv, o, lse, dbias=None):
    H = case.H
    do = R._nan_backed(case.dO_packed())
    on = R._nan_backed(o)
    dqkv = ext.attn_bwd(do, qkv, on, lse, H) if dbias is None else ext.attn_bwd(do, qkv, on, lse, H, dbias)
    assert dqkv.shape == qkv.shape
    return R.unpack_qkv(dqkv, H)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_selector_forward(ext, shape):
    """A: every query reads exactly its own key in every tile, at logits of hundreds of nats (in the
    tile-streamed kernel a later tile can raise the running maximum by as much): o == v[pi] bit for bit,
    lse within 4 fp32 ulps."""
    case = R.make_case("A", shape, "cuda")
    _, o, lse = _forward(ext, case)
    R.check_selector_fwd(case, R.unpack_o(o, case.H), lse)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_selector_backward(ext, shape):
    """A: dv[pi(i)] == dO[i] bit for bit and dq == dk == 0 (dO . v is an exact integer in any order, o
    equals v[pi], so delta == dP at the selected key; P is 1 or 0 in bf16); with the fused bias gradient
    the v part of a dbias filled with 0.5 is 0.5 + sum(dO) and the q / k parts stay 0.5.

    This test found the bf16 pre-scaled Q of the whole-sequence backward: attn_bwd2_kernel and
    attn_bwd3_kernel staged Q as bf16(q * scale * log2(e)), a relative 2**-8 rounding of the logits that
    the forward does not have.  With q = +-8 at hd 64, 8 * 0.18034 = 1.44270 became 1.4453125, the selected
    key's score of 738.66 (log2 domain) became 740.0 and P = 2**1.34: dv[pi(i)] was 2.53 dO[i] at hd 64 and
    3.21 dO[i] at hd 32 on all 22 whole-sequence shapes.  They now scale the fp32 score, as the forward
    and the tile-streamed backward do."""
    B, S, H, hd = shape
    case = R.make_case("A", shape, "cuda")
    qkv, o, lse = _forward(ext, case)
    dq, dk, dv = _backward(ext, case, qkv, o, lse)
    R.check_selector_bwd(case, dq, dk, dv)
    if ext.attn_fused_bias(S, hd):
        dbias = torch.full((3 * H * hd,), 0.5, device="cuda")
        dq2, dk2, dv2 = _backward(ext, case, qkv, o, lse, dbias)
        assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)
        R.check_selector_dbias(case, dbias)


@pytest.mark.parametrize("kind", ["B", "Bm"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_uniform(ext, shape, kind):
    """B (q = 0) and its mirror (k = 0): all scores 0, so a counted padded key moves lse off ln S; o, dv
    and dq (mirror: dk) per element, the other gradient exactly zero."""
    case = R.make_case(kind, shape, "cuda")
    qkv, o, lse = _forward(ext, case)
    dq, dk, dv = _backward(ext, case, qkv, o, lse)
    R.check_uniform(case, R.unpack_o(o, case.H), lse, dq, dk, dv)


@pytest.mark.parametrize("shape", R.SHAPES_C, ids=IDS_C)
def test_uniform_negative_forward(ext, shape):
    """C: every real score is -4 sqrt(hd) nats; a padded key at score 0 would take all the mass."""
    case = R.make_case("C", shape, "cuda")
    _, o, lse = _forward(ext, case)
    R.check_negative(case, R.unpack_o(o, case.H), lse)


@pytest.mark.parametrize("shape", R.SHAPES_R, ids=IDS_R)
def test_random_forward_per_element(ext, shape):
    """R: the random inputs of test_kernels_gpu.py::test_attention (randn * 1.5), one shape per forward
    instantiation, |o - ref| <= 2**-8 (|ref| + sum_j p_j |v_j|) per element."""
    case = R.make_case("R", shape, "cuda")
    _, o, lse = _forward(ext, case)
    assert torch.isfinite(lse).all()
    R.check_random_fwd(case, R.unpack_o(o, case.H))
