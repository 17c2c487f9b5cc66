"""tests/attn_ref.py checked on the CPU: the selector construction holds for every shape of the GPU list,
the shape list reaches every kernel instantiation, a bf16-emulating composition stays within every bound
that the GPU tests assert, and faults injected into that composition are caught."""

import math

import pytest
import torch

import attn_ref as R

QUIET = lambda s: None
IDS = [R.shape_id(s) for s in R.SHAPES]


def _emul(case, fault=None):
    return R.emulate(case.q, case.k, case.v, case.dO, fault)


def test_shape_list_reaches_every_instantiation():
    """Every row of dispatch_sp x {EX, not EX} x {hd 32, hd 64} that a sequence length can reach (SP 32
    and 64 are always EX: S > SP - 32 for every S they take), every backward kind, and the tile-streamed
    kernels at each of the five head dims, below and above one 64-row tile."""
    got = {(k["HD"], k["SP"], k["EX"]) for k in (R.kernels(S, hd) for _, S, _, hd in R.SHAPES)}
    want = {(hd, sp, ex) for hd in (32, 64) for sp, ex in ((32, True), (64, True), (128, False), (128, True),
                                                          (224, False), (224, True))}
    want |= {(hd, None, None) for hd in (32, 64, 80, 96, 128)}
    assert got == want
    for hd in (32, 64):  # the unreachable rows really are unreachable
        assert not any(R.kernels(S, hd)["EX"] is False for S in range(1, 65))
    assert {R.kernels(S, hd)["bwd"] for _, S, _, hd in R.SHAPES} == {"bwd2", "bwd3x4", "bwd3x8", "bwd_dq+bwd_dkv"}
    assert set(R.SHAPES_C) <= set(R.SHAPES) and set(R.SHAPES_R) <= set(R.SHAPES)
    fwd = lambda s: tuple(R.kernels(s[1], s[3])[n] for n in ("HD", "SP", "EX", "fwd"))
    assert {fwd(s) for s in R.SHAPES_R} == {fwd(s) for s in R.SHAPES}  # one per forward instantiation
    assert len({fwd(s) for s in R.SHAPES_R}) == len(R.SHAPES_R)
    for B, S, H, hd in R.SHAPES:
        assert B >= 2 and H >= 3 and H % 2 == 1


def test_kernels_table_matches_the_bindings_constants():
    assert R.kernels(224, 32)["SP"] == 224 and R.kernels(225, 32)["SP"] is None
    assert R.kernels(64, 64)["bwd"] == "bwd2" and R.kernels(65, 64)["bwd"] == "bwd3x8"
    assert R.kernels(52, 80)["fwd"] == "fwd_long"


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_selector_construction(shape):
    """The three conditions of case A on the reference alone, the gap taken past the point where exp2
    underflows to zero (so the zeros of dq / dk are exact, not merely small), and the inputs are bf16
    numbers with their own data per (batch, head)."""
    B, S, H, hd = shape
    case = R.make_case("A", shape)
    gap, top, exact = R.selector_conditions(case)
    assert gap >= R.MIN_GAP_NATS and gap >= R.ZERO_GAP_NATS, gap
    assert top < 1024, top
    assert exact
    c = R.CODES[hd][0]
    assert math.log2(c) == int(math.log2(c))
    case.qkv(), case.dO_packed()  # assert bf16 representability
    assert case.v.abs().max() <= R.INT_MAX and case.dO.abs().max() <= R.INT_MAX
    for t in (case.k, case.v, case.dO):
        flat = t.reshape(B * H, -1)
        assert len({tuple(r.tolist()) for r in flat}) == B * H  # no two (b, h) share data
    assert torch.equal(torch.sort(case.pi, -1).values, torch.arange(S).expand(B, H, S))


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_bounds_hold_for_the_bf16_composition(shape):
    """Cases A, B, its mirror and C: float64 with the kernels' roundings passes every assertion."""
    for kind in ("A", "B", "Bm") + (("C",) if shape in R.SHAPES_C else ()):
        case = R.make_case(kind, shape)
        o, lse, dq, dk, dv = _emul(case)
        if kind == "A":
            R.check_selector_fwd(case, o, lse, QUIET)
            R.check_selector_bwd(case, dq, dk, dv, QUIET)
            dbias = 0.5 + torch.stack([dq, dk, dv]).double().sum((1, 3)).float()
            R.check_selector_dbias(case, dbias)
        elif kind == "C":
            R.check_negative(case, o, lse, QUIET)
        else:
            R.check_uniform(case, o, lse, dq, dk, dv, QUIET)


@pytest.mark.parametrize("shape", R.SHAPES_R, ids=[R.shape_id(s) for s in R.SHAPES_R])
def test_random_forward_bound_holds_for_the_bf16_composition(shape):
    """|o - ref| <= 2**-8 (|ref| + sum p |v|) with P and o rounded to bf16: the worst ratio observed over
    these inputs is 0.61 of the bound (0.48 .. 0.61 per shape), so the margin stands as derived."""
    case = R.make_case("R", shape)
    r = R.check_random_fwd(case, _emul(case)[0], QUIET)
    assert 0.3 < r < 0.75, r  # a bound the composition never comes near would not be a per-element check


def test_layout_round_trip():
    case = R.make_case("R", (2, 17, 3, 32))
    qkv = case.qkv()
    assert qkv.shape == (2, 17, 3 * 3 * 32) and qkv.dtype == torch.bfloat16
    q, k, v = R.unpack_qkv(qkv, 3)
    assert torch.equal(q.double(), case.q) and torch.equal(k.double(), case.k) and torch.equal(v.double(), case.v)
    x = qkv.view(2, 17, 3, 3, 32)  # [B, S, 3, H, hd]
    assert torch.equal(x[1, 5, 2, 1].double(), case.v[1, 1, 5])
    assert torch.equal(R.unpack_o(case.dO_packed(), 3).double(), case.dO)
    nb = R._nan_backed(qkv)
    assert torch.equal(nb, qkv) and nb.is_contiguous()


# ------------------------------------------------------------------ injected faults
# Which case sees which fault.  The blind spots are by construction, and another case covers each:
#  * a key that a row wrongly drops or a padded key that it wrongly counts moves A only if that key is the
#    row's selected one (a padded key's score 0 is hundreds of nats below the winner): B and C see it in lse;
#  * B and C weigh every key alike and their dv rows are all equal, so keys swapped against their values
#    and shifted dv rows are invisible to them: A pins which row goes where.
CATCHES = {
    "row_ignores_key0": ("B", "Bm", "C"),
    "last_key_masked": ("A", "B", "Bm", "C"),
    "pad_counted": ("B", "Bm", "C"),
    "swap_keys": ("A",),
    "dv_shift": ("A",),
}
FAULT_SHAPE = (2, 197, 3, 32)  # SP 224 with 27 padded keys; a partial last query tile


def _run_checks(case, out):
    o, lse, dq, dk, dv = out
    if case.kind == "A":
        R.check_selector_fwd(case, o, lse, QUIET)
        R.check_selector_bwd(case, dq, dk, dv, QUIET)
    elif case.kind == "C":
        R.check_negative(case, o, lse, QUIET)
    else:
        R.check_uniform(case, o, lse, dq, dk, dv, QUIET)


def test_every_fault_has_a_case():
    assert set(CATCHES) == set(R.FAULTS)


@pytest.mark.parametrize("fault,kind", [(f, k) for f in R.FAULTS for k in CATCHES[f]])
def test_injected_fault_is_caught(fault, kind):
    case = R.make_case(kind, FAULT_SHAPE)
    _run_checks(case, _emul(case))  # clean: passes
    with pytest.raises(AssertionError):
        _run_checks(case, _emul(case, fault))


@pytest.mark.parametrize("fault", ["row_ignores_key0", "last_key_masked", "pad_counted"])
def test_whole_tensor_norm_misses_what_the_bounds_catch(fault):
    """The metric of the random-input tests (one norm ratio, rel(o) < 1e-2) on the same faults at the
    uniform case: a single row's fault disappears in it, the per-element bounds catch it."""
    case = R.make_case("B", FAULT_SHAPE)
    o = _emul(case, fault)[0].double()
    rel = float((o - case.ref.o).norm() / case.ref.o.norm())
    if fault == "row_ignores_key0":
        assert rel < 1e-2
    with pytest.raises(AssertionError):
        _run_checks(case, _emul(case, fault))


def test_single_nan_and_single_element_are_caught():
    case = R.make_case("A", FAULT_SHAPE)
    o, lse, dq, dk, dv = _emul(case)
    bad = dq.clone()
    bad[1, 2, 196, 31] = 2.0 ** -126  # the smallest normal number is not zero
    with pytest.raises(AssertionError):
        R.check_selector_bwd(case, bad, dk, dv, QUIET)
    bad = o.clone()
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        R.check_selector_fwd(case, bad, lse, QUIET)
    R.check_selector_bwd(case, -dq, dk, dv, QUIET)  # -0.0 is allowed
    lse2 = lse.clone()
    lse2[1, 1, 7] = torch.nextafter(torch.nextafter(lse2[1, 1, 7], torch.tensor(1e9)), torch.tensor(1e9)) + 4 * 2.0 ** -15
    with pytest.raises(AssertionError):
        R.check_selector_fwd(case, o, lse2, QUIET)
